"""mtr_replay_handover on config C3 against the full download followed by the filtering
(profiles/replay_handover_c3.json).

usage: python scripts/replay_handover_profile.py [--docs N] [--ops N] [--parts N] [--pipelined-only]
  C3: 100,000 documents x 1,000 messages (bench.py's preset), 16 ranges.
The batch is recorded once and downloaded into page-locked memory; a serial summary gives the ids.  Per leg the cache
holds the ids of a seeded 0 %, 50 %, 90 % and 100 % of the documents.  One warm-up, then 10 runs, each from mtr_reset,
wall time by the host clock:
  handover:   replay_handover into a pinned buffer (ids, states, reps and offsets included); with it the summed device
              times of its per-range id passes and classify + scan + gather passes (mtr_last_timing).  Every run must
              have run its ranges (handover_ranges = 1, handover_ids_ms > 0): a run that took the serial calls inside
              is an error here, not a data point.
  download+filter: replay_pipelined into a pinned buffer (every record), then blob_ids_raw and summary_novel_raw -- what
              a host that wants both the pipeline and the filtering does without the new call; same build, same state.
  pipelined:  replay_pipelined alone, for the cost the new stages add when nothing is held.
--pipelined-only runs the last measurement alone and uses nothing this call added, so the same script gives the figure
of an earlier build (its output is then printed, not written to the profile).
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

RUNS = 11  # the first is the warm-up


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


n, ops, parts = arg("--docs", 100000), arg("--ops", 1000), arg("--parts", 16)
only = "--pipelined-only" in sys.argv
cfg = make_cfg(n, ops, writers=8, max_lag=32)
eng = Engine(n, max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=2 * int(cfg.text_cap) + 1024,
             prop_words=16384, remover_cells=4096, ops_per_launch=48)
eng.generate(cfg, tables(writers=8))
assert eng.stats()["bad_docs"] == 0
hb = eng.download(0, n, pinned_memory=True)
eng.reset()
eng.submit(hb)
eng.run()
eng.summarize()
ids, first = eng.blob_ids_raw(0, n)
ids = ids.copy()
nb, total = len(ids), eng.summary_bytes()
records = pinned(total + 4096, "u1")
res = {"config": "C3", "docs": n, "ops_per_doc": ops, "parts": parts, "runs": RUNS - 1, "summary_bytes": int(total),
       "blobs": int(nb), "legs": []}

if only:
    wall = []
    for _ in range(RUNS):
        eng.reset()
        wall.append(timed(lambda: eng.replay_pipelined(hb, records, parts))[0])
    print(json.dumps({"pipelined_only_wall_ms": spread(wall[1:]), **{k: res[k] for k in ("docs", "ops_per_doc", "parts")}}))
    sys.exit(0)

out = pinned(total + 16, "u1")
order = np.random.default_rng(0xcac4e).permutation(n)
for pct in (0, 50, 90, 100):
    held = np.zeros(n, dtype=bool)
    held[order[:n * pct // 100]] = True
    add = np.ascontiguousarray(ids[np.repeat(held, np.diff(first))])
    eng.blob_cache_clear()
    eng.blob_cache_add(add)
    hand, t_ids, t_novel, filt, pipe = [], [], [], [], []
    for _ in range(RUNS):
        eng.reset()
        ms, (_, state, rep, off, _, got_ids) = timed(lambda: eng.replay_handover(hb, out, parts, cap_blobs=nb))
        t = eng.timing()
        assert t["handover_ranges"] == 1 and t["handover_ids_ms"] > 0, "the hand-over took the serial calls inside"
        assert t["handover_copied_bytes"] == float(off[-1]) and np.array_equal(got_ids, ids)
        hand.append(ms)
        t_ids.append(t["handover_ids_ms"])
        t_novel.append(t["handover_novel_ms"])
        eng.reset()

        def full():
            eng.replay_pipelined(hb, records, parts)
            eng.blob_ids_raw(0, n, cap=nb)
            return eng.summary_novel_raw(0, n, out)

        ms, (_, state2, rep2, off2, _) = timed(full)
        filt.append(ms)
        assert np.array_equal(state, state2) and np.array_equal(rep, rep2) and np.array_equal(off, off2)
        eng.reset()
        pipe.append(timed(lambda: eng.replay_pipelined(hb, records, parts))[0])
    row = {"leg": f"cache of {pct} % of the documents", "cache_ids": eng.blob_cache_size(),
           "first_occurrences": int((state == 1).sum()), "repeats": int((state == 2).sum()),
           "novel_bytes": int(off[-1]), "handover_wall_ms": spread(hand[1:]),
           "download_then_filter_wall_ms": spread(filt[1:]), "pipelined_alone_wall_ms": spread(pipe[1:]),
           "ids_passes_ms": spread(t_ids[1:]), "classify_scan_gather_passes_ms": spread(t_novel[1:])}
    print(json.dumps(row), flush=True)
    res["legs"].append(row)
eng.close()

out_dir = os.environ.get("MTR_PROFILE_DIR", os.path.join(ROOT, "profiles"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "replay_handover_c3.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), flush=True)
