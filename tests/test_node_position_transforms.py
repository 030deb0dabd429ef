"""BatchReplayEngine.resolveRemoteClientPositions, BatchReplayClient.resolveRemoteClientPosition and getPosition
through the Node host: one batched call (mtr_transform_positions) gives the positions the per-query composition of
getContainingSegment and getRangeSegments gives, over remote views of every writer of several documents
(tests/node/position_transforms.js)."""
import json
import os
import shutil
import subprocess

import pytest

from fixtures import replay_files

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_batched_positions_equal_the_composition():
    from fluidframework_amd import build

    if build.build_node_addon() is None:
        pytest.skip("node headers missing")
    files = [p for p in replay_files() if "clients_8" in p][:4]
    r = subprocess.run(["node", os.path.join(HERE, "node", "position_transforms.js"), "30"] + files,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout)
    assert res["mismatches"] == [], res["mismatches"]
    assert res["docs"] == len(files) and res["queries"] > 50 * len(files)
    assert res["defined"] > res["undef"] > 2 * len(files) and res["moved"] > 10
    assert res["singles"] == 60 and res["positions"] == 10 * len(files)
    assert res["empty"] == 0 and "query 0" in res["refused"]
