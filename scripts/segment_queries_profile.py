"""One getContainingSegment query per resident document, batched against the loop (profiles/segment_queries.json).

usage: python scripts/segment_queries_profile.py [--docs N ...] [--runs R]
Per document count N (default 1, 1,000 and 100,000): an engine holding N C3-shaped documents (1,000 messages, 8
writers, lag 32, replayed on the device), and one query per document -- the middle of the document at its current
sequence number in writer 1's view -- in a shuffled document order.  Timed, wall clock around the C calls with
preallocated buffers, one warm-up then R runs (default 10) that alternate between the two legs:
  batched: mtr_get_containing_segments, the size query and the fetch (info, text and properties);
  loop:    per query mtr_get_containing_segment with a text buffer, then mtr_get_props when the segment has a set.
Both legs' answers are compared once before the timing.  Each N's result is written as soon as it is measured.
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidframework_amd import abi  # noqa: E402
from fluidframework_amd.engine import Engine, SegmentInfo, lib  # noqa: E402
from fluidframework_amd.synth import make_cfg, tables  # noqa: E402

OPS, WRITERS, LAG = 1000, 8, 32  # C3 (bench.py PRESETS)
PATH = os.path.join(ROOT, "profiles", "segment_queries.json")


def args(name, default):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name) + 1
    out = []
    while i < len(sys.argv) and not sys.argv[i].startswith("--"):
        out.append(int(sys.argv[i]))
        i += 1
    return out


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def measure(n, runs):
    cfg = make_cfg(n, OPS, writers=WRITERS, max_lag=LAG)
    eng = Engine(n, max_segments=2 * OPS + 128, heap_entries=2 * OPS + 128, text_units=2 * int(cfg.text_cap) + 1024,
                 prop_words=16384, remover_cells=4096)
    eng.generate(cfg, tables(writers=WRITERS))
    assert eng.stats()["bad_docs"] == 0
    order = np.random.default_rng(n).permutation(n)
    lengths = eng.view_lengths([(int(d), OPS, 1) for d in order])
    q = np.zeros(n, dtype=abi.VIEW_QUERY_DTYPE)
    q["doc"], q["pos"], q["ref_seq"], q["client"] = order, np.array(lengths) // 2, OPS, 1
    L, h = lib(), eng.h

    info = (SegmentInfo * n)()
    toff, poff = np.zeros(n + 1, dtype="<i8"), np.zeros(n + 1, dtype="<i8")
    cap = 64 * n + 64
    text, props = np.zeros(cap, dtype="<u2"), np.zeros(cap, dtype="<u4")

    def batched():
        t0 = time.perf_counter()
        r = L.mtr_get_containing_segments(h, q.ctypes.data, n, C.addressof(info), None, 0, toff.ctypes.data, None, 0,
                                          poff.ctypes.data)
        assert r == n and toff[n] <= cap and poff[n] <= cap
        r = L.mtr_get_containing_segments(h, q.ctypes.data, n, C.addressof(info), text.ctypes.data, int(toff[n]),
                                          toff.ctypes.data, props.ctypes.data, int(poff[n]), poff.ctypes.data)
        assert r == n
        return (time.perf_counter() - t0) * 1e3

    one = SegmentInfo()
    ltext, lprops = np.zeros(1 << 12, dtype="<u2"), np.zeros(1 << 12, dtype="<u4")
    queries = [tuple(int(x) for x in row) for row in q]

    def loop(check=False):
        with_props = 0
        t0 = time.perf_counter()
        for i, (doc, pos, ref, client) in enumerate(queries):
            L.mtr_get_containing_segment(h, doc, pos, ref, client, C.byref(one), ltext.ctypes.data, ltext.size)
            words = 0
            if one.leaf >= 0 and one.props != -1:
                words = L.mtr_get_props(h, doc, one.props, lprops.ctypes.data, lprops.size)
                with_props += 1
            if check:
                assert bytes(one) == bytes(info[i]), i
                units = 0 if one.marker or one.leaf < 0 else one.length
                assert np.array_equal(text[toff[i]:toff[i + 1]], ltext[:units]), i
                assert np.array_equal(props[poff[i]:poff[i + 1]], lprops[:words]), i
        return (time.perf_counter() - t0) * 1e3, with_props

    batched()
    _, with_props = loop(check=True)  # (also the loop's warm-up)
    b_ms, l_ms = [], []
    for _ in range(runs):
        b_ms.append(batched())
        l_ms.append(loop()[0])
    res = {"docs": n, "queries": n, "runs": runs, "segments_with_props": with_props, "text_units": int(toff[n]),
           "prop_words": int(poff[n]), "batched_wall_ms": spread(b_ms), "loop_wall_ms": spread(l_ms),
           "loop_over_batched_median": round(statistics.median(l_ms) / statistics.median(b_ms), 2),
           "batched_us_per_query": round(1e3 * statistics.median(b_ms) / n, 3),
           "loop_us_per_query": round(1e3 * statistics.median(l_ms) / n, 3)}
    eng.close()
    return res


def main():
    runs = args("--runs", [10])[0]
    out = json.load(open(PATH)) if os.path.exists(PATH) else {}
    out.update({"workload": f"C3-shaped documents ({OPS} messages, {WRITERS} writers, lag {LAG}), one query per "
                            "document at the middle of its current view", "legs": out.get("legs", [])})
    for n in args("--docs", [1, 1000, 100000]):
        res = measure(n, runs)
        print(json.dumps(res), flush=True)
        out["legs"] = sorted([x for x in out["legs"] if x["docs"] != n] + [res], key=lambda x: x["docs"])
        with open(PATH, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
