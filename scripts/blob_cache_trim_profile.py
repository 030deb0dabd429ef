"""The blob-id cache's trim at 2,000,000 entries (profiles/blob_cache_trim.json).

usage: python scripts/blob_cache_trim_profile.py [--ids N]
The cache is filled with N distinct random ids spread evenly over 20 generations (blob_cache_import; no replay is
needed).  Per cutoff that keeps 90 %, 50 % and 10 % of the entries: one warm-up then 10 runs, each after
blob_cache_clear + blob_cache_import (not timed), of
  trim:         blob_cache_trim(cutoff): the device time by HIP events (mtr_last_timing out[11]: keep flags, scan,
                compaction, slot rebuild) and the wall time of the call;
  clear + add:  what a host does for the same result without the trim -- it keeps the survivors' ids in host memory
                and calls blob_cache_clear + blob_cache_add(survivors); wall time, in the same run.
Also the device time of blob_cache_ages(1024) and the wall time of blob_cache_export at the full size.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidframework_amd.engine import Engine  # noqa: E402

RUNS = 11  # the first is the warm-up
GENERATIONS = 20


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def wall(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    n = arg("--ids", 2_000_000)
    rng = np.random.default_rng(0x7213)
    ids = rng.integers(0, 256, size=(n, 20), dtype="u1")
    ages = rng.permutation(np.arange(n, dtype="<u4") % GENERATIONS)
    stamps = (GENERATIONS - 1) - ages.astype("i8")
    eng = Engine(1, max_segments=4096, heap_entries=4096, text_units=1 << 16, prop_words=1 << 14, remover_cells=1 << 12)

    def fill():
        eng.blob_cache_clear()
        eng.blob_cache_import(ids, ages)
        assert eng.blob_cache_size() == n and eng.blob_cache_generation() == GENERATIONS - 1

    out = {"ids": n, "generations": GENERATIONS, "runs": RUNS - 1, "legs": []}
    fill()
    ages_ms, export_ms = [], []
    for _ in range(RUNS):
        hist = eng.blob_cache_ages(1024)
        assert hist[:GENERATIONS].tolist() == [n // GENERATIONS] * GENERATIONS
        ages_ms.append(eng.timing()["cache_ages_ms"])
        ms, (x, y) = wall(eng.blob_cache_export)
        assert x.shape == (n, 20) and np.array_equal(y, ages)
        export_ms.append(ms)
    out["ages_1024_device_ms"] = spread(ages_ms[1:])
    out["export_wall_ms"] = spread(export_ms[1:])
    for keep, cutoff in ((90, 2), (50, 10), (10, 18)):
        survivors = np.ascontiguousarray(ids[stamps >= cutoff])
        assert len(survivors) * 100 == keep * n
        dev, trim_wall, host_wall = [], [], []
        for _ in range(RUNS):
            fill()
            ms, removed = wall(lambda: eng.blob_cache_trim(cutoff))
            assert removed == n - len(survivors) and eng.blob_cache_size() == len(survivors)
            trim_wall.append(ms)
            dev.append(eng.timing()["cache_trim_ms"])
            trimmed = eng.blob_cache_export()[0]
            fill()
            ms, _ = wall(lambda: (eng.blob_cache_clear(), eng.blob_cache_add(survivors)))
            host_wall.append(ms)
            assert np.array_equal(eng.blob_cache_export()[0], trimmed)  # (the same set in the same order)
        out["legs"].append({"leg": f"keep {keep} %", "cutoff": cutoff, "kept": len(survivors),
                            "upload_avoided_bytes": len(survivors) * 20, "trim_device_ms": spread(dev[1:]),
                            "trim_wall_ms": spread(trim_wall[1:]), "clear_add_wall_ms": spread(host_wall[1:])})
        print(json.dumps(out["legs"][-1]), flush=True)
    eng.close()
    path = os.path.join(ROOT, "profiles", "blob_cache_trim.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "legs"}))


if __name__ == "__main__":
    main()
