"""BatchReplayEngine.getRangeSegments / getTextRanges and BatchReplayClient.getText(start, end) through the Node host:
one batched call (mtr_get_range_segments) gives the result objects and the text a walk of
BatchReplayClient.getContainingSegment gives, over a mixed batch of ranges of several documents
(tests/node/range_queries.js)."""
import json
import os
import shutil
import subprocess

import pytest

from fixtures import replay_files

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_batched_ranges_equal_the_walk():
    from fluidframework_amd import build

    if build.build_node_addon() is None:
        pytest.skip("node headers missing")
    files = [p for p in replay_files() if "clients_8" in p][:4]
    r = subprocess.run(["node", os.path.join(HERE, "node", "range_queries.js"), "30"] + files,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout)
    assert res["mismatches"] == [], res["mismatches"]
    assert res["docs"] == len(files) and res["queries"] > 10 * len(files)
    assert res["segments"] > 4 * res["queries"] and res["clipped"] > 0 and res["getText"] == 5 * len(files)
    assert res["empty"] == [0, 0] and "query 0" in res["refused"] and "end < start in query 0" in res["bad"]
