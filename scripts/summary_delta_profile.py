"""The incremental summary hand-over on config C3: delta build and download against the full download
(profiles/summary_delta_c3.json).

usage: python scripts/summary_delta_profile.py [--docs N] [--ops N]
  C3: 100,000 documents x 1,000 messages (bench.py's preset).
The summary is built once and its ids taken; host baselines then have the ids of exactly 0 %, 1 %, 10 %, 50 % and
100 % of the documents altered (seeded choice).  Per fraction, one warm-up then 10 runs (each after set_baseline, which
drops the cached delta): the device time of the delta build by HIP events (mtr_last_timing: flag + scan, gather), the
gather's (bytes read + bytes written) / time, and the wall time of summary_delta_raw into a pinned buffer (build +
download).  The comparison leg is what a host does without the delta, on the same engine state in the same run:
blob_ids_raw(0, n) plus summaries(0, n) into a pinned buffer.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidframework_amd.engine import Engine, pinned  # noqa: E402
from fluidframework_amd.synth import make_cfg, tables  # noqa: E402

HBM_GBPS = 8000.0  # MI355X peak HBM bandwidth


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


n, ops = arg("--docs", 100000), arg("--ops", 1000)
cfg = make_cfg(n, ops, writers=8, max_lag=32)
eng = Engine(n, max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=2 * int(cfg.text_cap) + 1024,
             prop_words=16384, remover_cells=4096, ops_per_launch=48)
eng.generate(cfg, tables(writers=8))
assert eng.stats()["bad_docs"] == 0
eng.summarize()
ids, first = eng.blob_ids_raw(0, n)
total = eng.summary_bytes()
out = pinned(total + 16, "u1")


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def full_download():
    t0 = time.perf_counter()
    eng.blob_ids_raw(0, n)
    eng.summaries(0, n, out)
    return (time.perf_counter() - t0) * 1e3


full = [full_download() for _ in range(11)][1:]
res = {"config": "C3", "docs": n, "ops_per_doc": ops, "blobs": int(len(ids)), "summary_bytes": int(total),
       "full_download_wall_ms": spread(full), "fractions": []}
rng = np.random.default_rng(0xde17a)
order = rng.permutation(n)
for pct in (0, 1, 10, 50, 100):
    docs = order[:n * pct // 100]
    base = ids.copy()
    for d in docs:
        base[first[d]:first[d + 1], 0] ^= 0x5a
    scan_ms, gather_ms, wall_ms = [], [], []
    for _ in range(11):
        eng.set_baseline((base, first))
        t0 = time.perf_counter()
        buf, flags, off, _ = eng.summary_delta_raw(0, n, out)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        t = eng.timing()
        scan_ms.append(t["delta_ms"] - t["delta_gather_ms"])
        gather_ms.append(t["delta_gather_ms"])
    changed = np.zeros(n, dtype=bool)
    changed[docs] = True
    want = np.repeat(changed, np.diff(first)).astype("u1")
    assert np.array_equal(flags, want), "flags differ from the altered documents"
    nbytes = int(off[-1])
    g = statistics.median(gather_ms[1:])
    res["fractions"].append({
        "documents_altered_pct": pct, "changed_blobs": int(flags.sum()), "changed_bytes": nbytes,
        "flag_scan_ms": spread(scan_ms[1:]), "gather_ms": spread(gather_ms[1:]),
        "gather_GBps": round(2 * nbytes / g / 1e6, 1) if g > 0 else None,
        "gather_fraction_of_8TBps": round(2 * nbytes / g / 1e6 / HBM_GBPS, 4) if g > 0 else None,
        "delta_wall_ms": spread(wall_ms[1:]),
    })
    print(json.dumps(res["fractions"][-1]), flush=True)
full2 = [full_download() for _ in range(5)]
res["full_download_wall_ms_after"] = spread(full2)
out_dir = os.environ.get("MTR_PROFILE_DIR", os.path.join(ROOT, "profiles"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "summary_delta_c3.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), flush=True)
