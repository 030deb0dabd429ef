"""Git tree ids through the Node host: BatchReplayEngine.summaryTreeIds() over a document range and
BatchReplayClient.summaryTreeId() (the catch-up blob passed as an extra entry) equal ids computed in JS with crypto
from the tree summarize() returns; the script compares, this test checks what it compared."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]


def _run(args):
    from fluidframework_amd import build

    if build.build_node_addon() is None:
        pytest.skip("node headers missing")
    r = subprocess.run(["node", os.path.join(HERE, "node", "tree_ids_engine.js")] + args, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def _check(res, n):
    assert len(res["docs"]) == len(res["plain"]) == n
    assert all(re_id(r["id"]) for r in res["docs"]) and all(re_id(x) for x in res["plain"])
    assert res["enumerable"] is False, "the addon's new function must not join its enumerable exports"


def re_id(x):
    return len(x) == 40 and set(x) <= set("0123456789abcdef")


def test_v1_tree_id_of_a_reference_log():
    from fixtures import replay_files

    path = [p for p in replay_files() if "len_16-clients_8" in p][0]
    res = _run(["replay", path])
    _check(res, 1)
    assert res["docs"][0]["names"][0] == "header"
    assert res["plain"][0] == res["docs"][0]["id"]  # (V1: no host blob, the two calls name the same tree)


def test_legacy_tree_ids_with_a_catchup_blob(tmp_path):
    from test_catchup import LEGACY, messages_from_batch
    from fluidframework_amd.synth import make_cfg, tables
    from oracle.oracle import generate, options

    cfg = make_cfg(3, 400, writers=8, max_lag=32)
    gb, _, status = generate(cfg, tables(writers=8), 0, 3, threads=3, opts=options(**LEGACY))
    assert (status == 0).all()
    docs = [dict(zip(("observer", "msgs"), messages_from_batch(gb, d))) for d in range(3)]
    f = tmp_path / "docs.json"
    f.write_text(json.dumps(docs))
    res = _run(["catchup", str(f), "113"])
    _check(res, 3)
    assert all(r["names"][0] == "header" and r["names"][-1] == "catchupOps" for r in res["docs"]), res["docs"]
    assert all(p != r["id"] for p, r in zip(res["plain"], res["docs"]))  # (the catch-up entry changes the tree)
