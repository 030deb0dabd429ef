"""BatchReplayEngine.findTiles, BatchReplayClient.findTile and getMarkerFromId through the Node host: one batched call
(mtr_find_markers) gives what a JS walk over getRangeSegments gives, on documents built from applyMsg with marker
inserts carrying referenceTileLabels and markerId (tests/node/find_markers.js)."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_marker_search_equals_the_walk():
    from fluidframework_amd import build

    if build.build_node_addon() is None:
        pytest.skip("node headers missing")
    r = subprocess.run(["node", os.path.join(HERE, "node", "find_markers.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout)
    assert res["mismatches"] == [], res["mismatches"]
    assert res["docs"] == 2 and res["queries"] == 2 * 3 * 14 * 3 * 3
    assert res["found"] > 150 and res["none"] > 150  # (a third of the queries name a label nobody carries)
    assert res["singles"] == 12 and res["ids"] == 18 + 8 and res["hiddenLeaf"] == 5
    assert res["empty"] == 0 and "query 0" in res["refused"]
    assert res["pgValues"] == 2 and res["unknownKey"] is True
