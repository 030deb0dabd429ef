"""BatchReplayEngine.replayHandover (mtr_replay_handover through the N-API addon): states, reps, bytes and ids equal
to the serial calls of the Python binding on the same documents, for a batch of remote messages (the pipelined path)
and for one with a pending local insert (the addon's serial calls)."""
import base64
import json
import os
import shutil
import subprocess

import pytest

from fixtures import load_replay, replay_files, replay_log
from fluidframework_amd.batch import Interner, build_batch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE_DIR = os.path.join(ROOT, "fluidframework_amd", "node")

pytestmark = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")

_REF = {}


def _addon():
    from fluidframework_amd import build

    build.build_engine()
    if build.build_node_addon() is None:
        pytest.skip("node headers missing")


def test_addon_exports_replay_handover_and_types_it():
    _addon()
    r = subprocess.run(["node", "-e", "const a=require(process.argv[1]).native();"
                        "console.log(typeof a.replayHandover, Object.keys(a).includes('replayHandover'))", NODE_DIR],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["function", "false"]  # (callable; the enumerable export list stays as it was)
    assert "replayHandover(parts?: number)" in open(os.path.join(NODE_DIR, "index.d.ts")).read()
    assert "replayHandover(parts = 16)" in open(os.path.join(NODE_DIR, "index.js")).read()


def _reference():
    """The Python serial calls over the reference replay logs, once: per blob (id, bytes), each document's first blob
    and the tree ids."""
    if not _REF:
        from fluidframework_amd.engine import Engine

        paths = replay_files()
        it = Interner()
        logs = []
        for p in paths:
            groups = load_replay(p)
            log = replay_log(groups, it)
            for g in groups:
                for m in g["msgs"]:
                    log.message(m, it)
            logs.append(log)
        n = len(paths)
        eng = Engine(n, max_segments=8192, heap_entries=8192, text_units=1 << 18, prop_words=1 << 18,
                     remover_cells=1 << 14)
        eng.apply(build_batch(logs, it))
        eng.summarize()
        assert eng.stats()["bad_docs"] == 0
        buf, off = eng.summaries(0, n)
        blobs = [b for d in range(n) for b in Engine.split_record(buf, int(off[d]), int(off[d + 1]))]
        ids = [x for doc in eng.blob_ids() for x in doc]
        _REF.update(paths=paths, n=n, blobs=blobs, ids=ids, first=[int(x) for x in eng.blob_ids_raw()[1]],
                    trees=eng.tree_ids())
        eng.close()
    return _REF


@pytest.mark.gpu
@pytest.mark.parametrize("parts, mode, held", [(4, "remote", "none"), (7, "remote", "half"), (4, "remote", "all"),
                                              (4, "local", "half")])
def test_replay_handover_through_node_host(parts, mode, held, tmp_path, monkeypatch):
    from fluidframework_amd.gitid import summary_novel

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    ref = _reference()
    distinct = sorted(set(ref["ids"]))
    cache = {"none": [], "half": distinct[::2], "all": distinct}[held]
    f = tmp_path / "held.json"
    f.write_text(json.dumps(cache))
    r = subprocess.run(["node", os.path.join(HERE, "node", "replay_handover.js"), str(parts), mode, str(f)] + ref["paths"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(r.stdout)
    assert res["pipelined"] is (mode == "remote")
    assert res["docFirst"] == ref["first"]
    first = ref["first"]
    docs = [ref["blobs"][first[d]:first[d + 1]] for d in range(ref["n"])]
    want = [row for doc in summary_novel(set(cache), docs) for row in doc]
    got = [(b["id"], b["state"], b["rep"], base64.b64decode(b["bytes"]) if b["state"] == 1 else None)
           for b in res["blobs"]]
    assert got == want
    assert res["treeIds"] == ref["trees"]
