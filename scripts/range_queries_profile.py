"""One range query per resident document, batched against the loop it replaces (profiles/range_queries.json).

usage: python scripts/range_queries_profile.py [--docs N ...] [--segments S ...] [--runs R]
Per document count N (default 1, 1,000 and 100,000): an engine holding N C3-shaped documents (1,000 messages, 8
writers, lag 32, replayed on the device).  Per range length S (default about 1, 8 and 64 segments): one query per
document in a shuffled document order, at its current sequence number in writer 1's view, from the middle of the view
over S times the document's mean visible segment length (the segments per query that came out are reported).  Timed,
wall clock around the C calls with preallocated buffers, one warm-up then R runs (default 10) that alternate between
the legs:
  batched:   mtr_get_range_segments, the sizing call, the fetch of rows and text, the fetch of the property words;
  text_only: the sizing call and the fetch of the text alone (no rows, no offsets per segment);
  loop:      per query the walk of mtr_get_containing_segment (with a text buffer) and mtr_get_props that defines it.
The loop runs over the first LOOP_SAMPLE queries only when N is larger, and its time is scaled by N / LOOP_SAMPLE
("loop_sampled": true); its answers are compared with the batch's once before the timing.
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
LOOP_SAMPLE = 200
INT32_MAX = 0x7fffffff
PATH = os.path.join(ROOT, "profiles", "range_queries.json")


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


def measure(eng, n, segs, runs):
    L, h = lib(), eng.h
    fn = L.mtr_get_range_segments
    order = np.random.default_rng(n).permutation(n)
    q = np.zeros(n, dtype=abi.RANGE_QUERY_DTYPE)
    q["doc"], q["start"], q["end"], q["ref_seq"], q["client"] = order, 0, INT32_MAX, OPS, 1
    first, tfirst = np.zeros(n + 1, dtype="<i8"), np.zeros(n + 1, dtype="<i8")
    # the whole views once: their lengths and segment counts give each document's mean visible segment length
    assert fn(h, q.ctypes.data, n, 1, first.ctypes.data, None, 0, None, 0, tfirst.ctypes.data, None, None, 0, None) >= 0
    length, count = np.diff(tfirst), np.maximum(np.diff(first), 1)
    q["start"] = length // 2
    q["end"] = q["start"] + np.maximum(1, np.rint((segs - 0.5) * length / count)).astype("<i4")
    cap = int(fn(h, q.ctypes.data, n, 0, first.ctypes.data, None, 0, None, 0, tfirst.ctypes.data, None, None, 0, None))
    assert cap >= 0
    info = (SegmentInfo * max(cap, 1))()
    toff, poff = np.zeros(cap + 1, dtype="<i8"), np.zeros(cap + 1, dtype="<i8")
    text, props = np.zeros(int(tfirst[n]) + 64, dtype="<u2"), np.zeros(16 * cap + 64, dtype="<u4")

    def batched():
        t0 = time.perf_counter()
        total = fn(h, q.ctypes.data, n, 0, first.ctypes.data, None, 0, None, 0, tfirst.ctypes.data, None, None, 0, None)
        assert total == cap
        r = fn(h, q.ctypes.data, n, 0, first.ctypes.data, C.addressof(info), cap, text.ctypes.data, text.size,
               tfirst.ctypes.data, toff.ctypes.data, None, 0, poff.ctypes.data)
        assert r == total and poff[total] <= props.size
        r = fn(h, q.ctypes.data, n, 0, first.ctypes.data, None, 0, None, 0, None, None, props.ctypes.data, props.size,
               poff.ctypes.data)
        assert r == total
        return (time.perf_counter() - t0) * 1e3

    def text_only():
        t0 = time.perf_counter()
        total = fn(h, q.ctypes.data, n, 0, first.ctypes.data, None, 0, None, 0, tfirst.ctypes.data, None, None, 0, None)
        r = fn(h, q.ctypes.data, n, 0, first.ctypes.data, None, 0, text.ctypes.data, text.size, tfirst.ctypes.data, None,
               None, 0, None)
        assert r == total == cap
        return (time.perf_counter() - t0) * 1e3

    one = SegmentInfo()
    ltext, lprops = np.zeros(1 << 12, dtype="<u2"), np.zeros(1 << 12, dtype="<u4")
    sample = min(n, LOOP_SAMPLE)
    queries = [tuple(int(x) for x in row) for row in q[:sample]]

    def loop(check=False):
        t0 = time.perf_counter()
        for i, (doc, start, end, ref, client) in enumerate(queries):
            p, k = start, int(first[i])
            while p < end:
                L.mtr_get_containing_segment(h, doc, p, ref, client, C.byref(one), ltext.ctypes.data, ltext.size)
                if one.leaf < 0:
                    break
                words = 0
                if one.props != -1:
                    words = L.mtr_get_props(h, doc, one.props, lprops.ctypes.data, lprops.size)
                if check:
                    assert bytes(one) == bytes(info[k]), (i, k)
                    lo, hi = max(start - one.start, 0), min(end - one.start, one.length)
                    units = ltext[lo:hi] if not one.marker else ltext[:0]
                    assert np.array_equal(text[toff[k]:toff[k + 1]], units), (i, k)
                    assert np.array_equal(props[poff[k]:poff[k + 1]], lprops[:words]), (i, k)
                p, k = one.start + one.length, k + 1
            if check:
                assert k == first[i + 1], i
        return (time.perf_counter() - t0) * 1e3 * n / sample

    batched()
    text_only()
    loop(check=True)  # (also the loop's warm-up)
    b_ms, t_ms, l_ms = [], [], []
    for _ in range(runs):
        b_ms.append(batched())
        t_ms.append(text_only())
        l_ms.append(loop())
    return {"docs": n, "queries": n, "target_segments": segs, "segments_per_query": round(cap / n, 2), "runs": runs,
            "text_units": int(tfirst[n]), "prop_words": int(poff[cap]), "batched_wall_ms": spread(b_ms),
            "text_only_wall_ms": spread(t_ms), "loop_wall_ms": spread(l_ms), "loop_sampled": sample < n,
            "loop_sample_queries": sample,
            "loop_over_batched_median": round(statistics.median(l_ms) / statistics.median(b_ms), 2),
            "batched_us_per_segment": round(1e3 * statistics.median(b_ms) / max(cap, 1), 3)}


def main():
    runs = args("--runs", [10])[0]
    out = json.load(open(PATH)) if os.path.exists(PATH) else {}
    out.update({"workload": f"C3-shaped documents ({OPS} messages, {WRITERS} writers, lag {LAG}), one range query per "
                            "document from the middle of its current view", "legs": out.get("legs", [])})
    for n in args("--docs", [1, 1000, 100000]):
        cfg = make_cfg(n, OPS, writers=WRITERS, max_lag=LAG)
        eng = Engine(n, max_segments=2 * OPS + 128, heap_entries=2 * OPS + 128, text_units=2 * int(cfg.text_cap) + 1024,
                     prop_words=16384, remover_cells=4096)
        eng.generate(cfg, tables(writers=WRITERS))
        assert eng.stats()["bad_docs"] == 0
        for segs in args("--segments", [1, 8, 64]):
            res = measure(eng, n, segs, runs)
            print(json.dumps(res), flush=True)
            out["legs"] = sorted([x for x in out["legs"] if (x["docs"], x["target_segments"]) != (n, segs)] + [res],
                                 key=lambda x: (x["docs"], x["target_segments"]))
            with open(PATH, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
        eng.close()


if __name__ == "__main__":
    main()
