"""The Node host's findOverlappingIntervals / previousInterval / nextInterval over mtr_query_intervals
(fluidframework_amd/node/intervals.js) against the Python host's answers on one interval-farm seed
(tests/node/interval_queries.js)."""
import json
import os
import shutil
import subprocess

import pytest

import interval_farm as F
from fluidframework_amd.intervals import IntervalUnsupported

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_collection_queries_equal_the_python_host(tmp_path):
    from fluidframework_amd import build
    from test_interval_live import _engine_executor
    from test_interval_queries_batch import _host

    if build.build_node_addon() is None:
        pytest.skip("node headers missing")
    init, msgs, obs = F.farm(1)
    c = _host(init, msgs, _engine_executor())
    n = len(obs.text())

    def ask(fn, pos):
        try:
            iv = fn([pos])[0]
        except IntervalUnsupported:
            return "refused"
        return iv.id() if iv else None

    labels = {}
    for label in obs.data:
        hc = c.get_interval_collection(label)
        ranges = [(a, min(n - 1, a + 5)) for a in range(0, n, 7)] + [(5, 2), (0, n + 9), (-4, 3)]
        got = hc.find_overlapping_intervals_many(ranges)
        labels[label] = {"overlaps": [[a, b, [iv.id() for iv in ivs]] for (a, b), ivs in zip(ranges, got)],
                         "ends": [[p, ask(hc.previous_intervals_many, p), ask(hc.next_intervals_many, p)]
                                  for p in list(range(0, n + 1, 3)) + [-1, n + 7]]}
    src = tmp_path / "farm.json"
    src.write_text(json.dumps({"init": init, "msgs": msgs, "labels": labels}))
    r = subprocess.run(["node", os.path.join(HERE, "node", "interval_queries.js"), str(src)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout)
    assert res["mismatches"] == [], res["mismatches"][:5]
    assert res["overlaps"] > 10 and res["compared"] > 10 and res["records"] == 0
    assert any(ids for x in labels.values() for _, _, ids in x["overlaps"])
