"""One position transform per resident document, batched against the loop it replaces (profiles/position_transforms.json).

usage: python scripts/position_transforms_profile.py [--docs N ...] [--runs R] [--out PATH]
Per document count N (default 1, 1,000 and 100,000): an engine holding N C3-shaped documents (1,000 messages, 8
writers, lag 32, replayed on the device).  One query per document in a shuffled document order: the middle position of
writer 1's view 16 sequence numbers back (a lagging remote cursor) mapped into the local view at the current sequence
number.  Timed, wall clock around the C calls with preallocated buffers, one warm-up then R runs (default 10) that
alternate between the legs:
  batched:  mtr_transform_positions over all N queries;
  loop:     per query one mtr_get_containing_segment at the remote view (no text), one info-only
            mtr_get_range_segments over the whole target view (one call: the rows fit the preallocated buffer), and the
            search of the rows for the first leaf not below the segment's.
The loop runs over the first LOOP_SAMPLE queries only when N is larger, and its time is scaled by N / LOOP_SAMPLE
("loop_sampled": true); its answers are compared with the batch's once before the timing.
Not measured: the split of the batched call between its kernel and its two copies, and what leaving the walk in the
round that finds the leaf saves over walking the whole document.
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
BACK = 16  # how far the remote view lags
LOOP_SAMPLE = 200
INT32_MAX = 0x7fffffff
SEGCAP = 2 * OPS + 128
PATH = os.path.join(ROOT, "profiles", "position_transforms.json")


def args(name, default, conv=int):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name) + 1
    out = []
    while i < len(sys.argv) and not sys.argv[i].startswith("--"):
        out.append(conv(sys.argv[i]))
        i += 1
    return out


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def measure(eng, n, runs):
    L, h = lib(), eng.h
    fn = L.mtr_transform_positions
    order = np.random.default_rng(n).permutation(n)
    lengths = eng.view_lengths([(int(d), OPS - BACK, 1) for d in order])
    q = np.zeros(n, dtype=abi.POSITION_QUERY_DTYPE)
    q["doc"], q["pos"], q["ref_seq"], q["client"] = order, np.array(lengths) // 2, OPS - BACK, 1
    q["to_ref_seq"], q["to_client"], q["mode"] = INT32_MAX, -1, abi.POS_FROM_VIEW
    out = np.zeros(n, dtype=abi.POSITION_DTYPE)

    def batched():
        t0 = time.perf_counter()
        assert fn(h, q.ctypes.data, n, out.ctypes.data) == n
        return (time.perf_counter() - t0) * 1e3

    one = SegmentInfo()
    rows = (SegmentInfo * SEGCAP)()
    grid = np.frombuffer(rows, dtype="<i4").reshape(SEGCAP, -1)  # (mtr_segment_info: [0] leaf, [9] start)
    rq = np.zeros(1, dtype=abi.RANGE_QUERY_DTYPE)
    first = np.zeros(2, dtype="<i8")
    sample = min(n, LOOP_SAMPLE)
    queries = [tuple(int(x) for x in row) for row in q[:sample]]

    def loop(check=False):
        t0 = time.perf_counter()
        for i, (doc, pos, ref, client, to_ref, to_client, _, _) in enumerate(queries):
            L.mtr_get_containing_segment(h, doc, pos, ref, client, C.byref(one), None, 0)
            rq[0] = (doc, 0, INT32_MAX, to_ref, to_client)
            total = L.mtr_get_range_segments(h, rq.ctypes.data, 1, 0, first.ctypes.data, C.addressof(rows), SEGCAP,
                                             None, 0, None, None, None, 0, None)
            end = int(grid[total - 1, 9] + grid[total - 1, 2]) if total else 0
            if one.leaf >= 0:
                k = int(np.searchsorted(grid[:total, 0], one.leaf))
                got = (int(grid[k, 9]) if k < total else end) + one.offset
            else:
                got = end if pos == one.start else -1
            if check:
                assert got == out[i]["pos"] and one.leaf == out[i]["leaf"], (i, got, out[i])
        return (time.perf_counter() - t0) * 1e3 * n / sample

    batched()
    loop(check=True)  # (also the loop's warm-up)
    b_ms, l_ms = [], []
    for _ in range(runs):
        b_ms.append(batched())
        l_ms.append(loop())
    flags = out["flags"]
    return {"docs": n, "queries": n, "runs": runs, "batched_wall_ms": spread(b_ms), "loop_wall_ms": spread(l_ms),
            "loop_sampled": sample < n, "loop_sample_queries": sample,
            "found": int((flags & abi.POS_FOUND != 0).sum()), "moved": int((out["pos"] != q["pos"]).sum()),
            "loop_over_batched_median": round(statistics.median(l_ms) / statistics.median(b_ms), 2),
            "batched_us_per_query": round(1e3 * statistics.median(b_ms) / n, 3)}


def main():
    runs = args("--runs", [10])[0]
    path = args("--out", [PATH], str)[0]
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.update({"workload": f"C3-shaped documents ({OPS} messages, {WRITERS} writers, lag {LAG}), one position per "
                            f"document: the middle of writer 1's view {BACK} sequence numbers back, mapped into the "
                            "local view", "legs": out.get("legs", []),
                "not_measured": ["the split of the batched call between the kernel and its two copies",
                                 "what leaving the walk in the round that finds the leaf saves"]})
    for n in args("--docs", [1, 1000, 100000]):
        cfg = make_cfg(n, OPS, writers=WRITERS, max_lag=LAG)
        eng = Engine(n, max_segments=SEGCAP, heap_entries=SEGCAP, text_units=2 * int(cfg.text_cap) + 1024,
                     prop_words=16384, remover_cells=4096)
        eng.generate(cfg, tables(writers=WRITERS))
        assert eng.stats()["bad_docs"] == 0
        res = measure(eng, n, runs)
        print(json.dumps(res), flush=True)
        out["legs"] = sorted([x for x in out["legs"] if x["docs"] != n] + [res], key=lambda x: x["docs"])
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        eng.close()


if __name__ == "__main__":
    main()
