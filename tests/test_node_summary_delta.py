"""The incremental hand-over through the Node host: BatchReplayEngine.markSummaryBaseline / summaryDelta /
clearSummaryBaseline.  Against a marked baseline every entry is null; without one every entry is a Buffer whose
hashlib git id is the id beside it."""
import base64
import hashlib
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]


def test_mark_and_clear_over_a_reference_log():
    from fixtures import replay_files
    from fluidframework_amd import build

    if build.build_node_addon() is None:
        pytest.skip("node headers missing")
    path = [p for p in replay_files() if "len_16-clients_8" in p][0]
    r = subprocess.run(["node", os.path.join(HERE, "node", "summary_delta_engine.js"), path], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout)
    blobs = [base64.b64decode(x) for x in res["blobs"]]
    want = [hashlib.sha1(b"blob %d\0" % len(b) + b).hexdigest() for b in blobs]
    assert len(blobs) >= 1
    for name in ("before", "marked", "cleared"):
        assert res[name]["ids"] == want, name
        assert res[name]["docFirst"] == [0, len(blobs)], name
    assert res["marked"]["changed"] == [None] * len(blobs)
    for name in ("before", "cleared"):
        got = [base64.b64decode(x) for x in res[name]["changed"]]
        assert got == blobs, name
        assert [hashlib.sha1(b"blob %d\0" % len(b) + b).hexdigest() for b in got] == res[name]["ids"]
