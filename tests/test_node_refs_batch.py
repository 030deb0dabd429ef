"""BatchReplayEngine.getRefsBatch through the Node host: one batched call (mtr_get_refs) gives the words the
per-document getRefPositions / getRefStates / getRefKeys give, over an empty document, one without references, one with
65 references and one with references on removed text (tests/node/refs_batch_engine.js)."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NODE_DIR = os.path.join(os.path.dirname(HERE), "fluidframework_amd", "node")


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_batched_references_equal_the_single_calls():
    from fluidframework_amd import build

    if build.build_node_addon() is None:
        pytest.skip("node headers missing")
    r = subprocess.run(["node", os.path.join(HERE, "node", "refs_batch_engine.js")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout)
    assert res["mismatches"] == [], res["mismatches"]
    # the listed clients: 65 references twice, 4 once, two documents without any
    assert res["positions65"] == 65
    assert res["counts"] == {"1": 134, "2": 134, "4": 134}
    assert res["emptyTotal"] == 0 and res["emptyWords"] == 0
    assert "entry 0" in res["refused"] and "mode" in res["badMode"]
    assert res["enumerable"] is False  # (tests/test_node.py pins the enumerable export list)


def test_node_declares_the_batched_reference_query():
    assert "getRefsBatch(clients: BatchReplayClient[], mode: 1 | 2 | 4)" in open(os.path.join(NODE_DIR, "index.d.ts")).read()
    assert "getRefsBatch(clients, mode)" in open(os.path.join(NODE_DIR, "index.js")).read()
    assert '{"getRefsBatch", nullptr, GetRefsBatch' in open(os.path.join(NODE_DIR, "mtr_napi.cc")).read()
