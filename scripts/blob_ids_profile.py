"""Git blob ids of a whole summary: device time against host hashing (profiles/blob_ids_<config>.json).

usage: python scripts/blob_ids_profile.py [C3|C5] [--ops N]
  C3: 100,000 documents x 1,000 messages; C5: 1,000 documents pre-grown to 200,000 segments (bench.py's presets).
Device time: HIP events around the blob-table kernels and the id kernel (mtr_last_timing's blob_ids_ms), one warm-up,
then the median of 10 computations (each after a fresh summarize, which drops the cached ids).  Host time:
hashlib.sha1 over the same downloaded blobs, on one thread and on a pool of 16 threads with a contiguous sixteenth of
the blobs each (hashlib releases the GIL while it hashes a blob of 2 KB or more).  Every
device id is compared with the host's.
"""
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidframework_amd.engine import Engine  # noqa: E402
from fluidframework_amd.gitid import git_blob_id  # noqa: E402
from fluidframework_amd.synth import make_cfg, tables  # noqa: E402

config = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else "C3"
ops_arg = int(sys.argv[sys.argv.index("--ops") + 1]) if "--ops" in sys.argv else None
if config == "C5":
    n, ops, writers, lag, grow = 1000, ops_arg or 20000, 64, 4096, 200000
    cfg = make_cfg(n, ops, writers=writers, max_lag=lag, text_cap=2 * grow + 18 * ops + 16)
    eng = Engine(n, max_segments=grow + grow // 14 + 2 * ops + 128, heap_entries=grow + 2 * ops + 128,
                 text_units=4 * int(cfg.text_cap) + 16384, prop_words=65536, remover_cells=65536, ops_per_launch=48)
else:
    n, ops, writers, lag, grow = 100000, ops_arg or 1000, 8, 32, 0
    cfg = make_cfg(n, ops, writers=writers, max_lag=lag)
    eng = Engine(n, max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=2 * int(cfg.text_cap) + 1024,
                 prop_words=16384, remover_cells=4096, ops_per_launch=48)
eng.generate(cfg, tables(writers=writers), grow=grow)
assert eng.stats()["bad_docs"] == 0

dev_ms, sum_ms = [], []
for _ in range(11):
    eng.summarize()
    sum_ms.append(eng.timing()["summary_ms"])
    eng.blob_ids_raw(0, 1)  # the first call after a summary hashes every document's blobs
    dev_ms.append(eng.timing()["blob_ids_ms"])
dev_ms, sum_ms = dev_ms[1:], sum_ms[1:]
ids, first = eng.blob_ids_raw(0, n)
buf, off = eng.summaries(0, n)

spans = []  # (start, end) of every blob in buf, in id order
for d in range(n):
    a = int(off[d])
    nb = int(np.frombuffer(buf[a:a + 4].tobytes(), "<u4")[0])
    lens = np.frombuffer(buf[a + 4:a + 4 + 4 * nb].tobytes(), "<u4")
    p = a + 4 + 4 * nb
    for ln in lens:
        spans.append((p, p + int(ln)))
        p += int(ln)
assert len(spans) == len(ids)
hashed = sum(b - a for a, b in spans)
mv = memoryview(buf)


def one(s):
    return git_blob_id(mv[s[0]:s[1]])


t0 = time.perf_counter()
host1 = [one(s) for s in spans]
t1 = time.perf_counter() - t0
shards = [spans[k * len(spans) // 16:(k + 1) * len(spans) // 16] for k in range(16)]  # one contiguous run a thread
with ThreadPoolExecutor(16) as pool:
    t0 = time.perf_counter()
    host16 = [x for part in pool.map(lambda sh: [one(s) for s in sh], shards) for x in part]
    t16 = time.perf_counter() - t0
wrong = sum(ids[i].tobytes().hex() != host1[i] for i in range(len(spans)))
assert host16 == host1

med = statistics.median(dev_ms)
res = {
    "config": config, "docs": n, "ops_per_doc": ops, "grow": grow,
    "blobs": len(spans), "bytes_hashed": hashed, "max_blob_bytes": max(b - a for a, b in spans),
    "device_ms_median": round(med, 3), "device_ms_runs": [round(x, 3) for x in dev_ms],
    "device_GBps": round(hashed / med / 1e6, 2),
    "host_1_thread_ms": round(t1 * 1e3, 1), "host_16_threads_ms": round(t16 * 1e3, 1),
    "summary_ms_median": round(statistics.median(sum_ms), 3),
    "ids_differing_from_hashlib": wrong,
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
out_dir = os.environ.get("MTR_PROFILE_DIR", os.path.join(ROOT, "profiles"))
with open(os.path.join(out_dir, f"blob_ids_{config.lower()}.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), flush=True)
sys.exit(1 if wrong else 0)
