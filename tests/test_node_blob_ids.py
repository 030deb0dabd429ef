"""Git blob ids through the Node host: BatchReplayClient.summaryBlobIds() names every blob of summarize() by the id
hashlib gives its bytes -- the engine's blobs hashed on the device, the legacy catch-up blob hashed in JS."""
import base64
import hashlib
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ADDON = os.path.join(ROOT, "fluidframework_amd", "node", "mtr_napi.node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]


def _run(args):
    from fluidframework_amd import build

    if build.build_node_addon() is None:
        pytest.skip("node headers missing")
    r = subprocess.run(["node", os.path.join(HERE, "node", "blob_ids_engine.js")] + args, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def _check(res):
    for r in res:
        blobs = [base64.b64decode(x) for x in r["blobs"]]
        assert list(r["ids"]) == r["names"], f"doc {r['doc']}: ids name {list(r['ids'])}, the tree {r['names']}"
        for name, b in zip(r["names"], blobs):
            want = hashlib.sha1(b"blob %d\0" % len(b) + b).hexdigest()
            assert r["ids"][name] == want, f"doc {r['doc']} blob {name}"


def test_v1_ids_of_a_reference_log():
    from fixtures import replay_files

    path = [p for p in replay_files() if "len_16-clients_8" in p][0]
    res = _run(["replay", path])
    assert len(res) == 1 and res[0]["names"][0] == "header"
    _check(res)


def test_legacy_ids_with_a_catchup_blob(tmp_path):
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
    assert all(r["names"][0] == "header" and r["names"][-1] == "catchupOps" for r in res), [r["names"] for r in res]
    _check(res)
