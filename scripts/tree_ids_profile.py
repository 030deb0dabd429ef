"""Git tree ids of every document's summary tree: device time against what a host does without them
(profiles/tree_ids_<config>.json).

usage: python scripts/tree_ids_profile.py [C3|C5] [--ops N]
  C3: 100,000 documents x 1,000 messages; C5: 1,000 documents pre-grown to 200,000 segments (bench.py's presets).
Device leg: HIP events around the tree-id kernels (size, scan, write, id: mtr_last_timing's tree_ids_ms) with the blob
ids already on the device, one warm-up, then 10 runs of tree_ids_raw(0, n): the median and the min-max.  The wall time
of the same call (upload of nothing, kernels, download of 20 bytes a document) is reported beside it.
Host leg, on the same engine state: blob_ids_raw(0, n) (the download of every blob id; its wall time is reported on
its own) followed by gitid.summary_tree_id-style hashing with hashlib of each document's tree object from those ids,
on one thread and on a pool of 16 threads with a contiguous sixteenth of the documents each.  Every device id is
compared with the host's.
"""
import hashlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidframework_amd.engine import Engine  # noqa: E402
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
eng.summarize()
eng.blob_ids_raw(0, 1)  # the blob ids are made once; the tree ids below start from them

dev_ms, wall_ms = [], []
for _ in range(11):
    t0 = time.perf_counter()
    dev = eng.tree_ids_raw(0, n)
    wall_ms.append((time.perf_counter() - t0) * 1e3)
    dev_ms.append(eng.timing()["tree_ids_ms"])
dev_ms, wall_ms = dev_ms[1:], wall_ms[1:]

t0 = time.perf_counter()
ids, first = eng.blob_ids_raw(0, n)
t_download = time.perf_counter() - t0
raw = ids.tobytes()
first = [int(x) for x in first]


def tree_of(d):
    """The id of document d's tree from its blob ids (SnapshotV1 names; no host-made entries in these workloads)."""
    a, b = first[d], first[d + 1]
    rows = [(b"header" if k == a else b"body_%d" % (k - a - 1), raw[20 * k:20 * k + 20]) for k in range(a, b)]
    body = b"".join(b"100644 " + name + b"\0" + oid for name, oid in sorted(rows))
    return hashlib.sha1(b"tree %d\0" % len(body) + body).digest()


t0 = time.perf_counter()
host1 = [tree_of(d) for d in range(n)]
t1 = time.perf_counter() - t0
shards = [range(k * n // 16, (k + 1) * n // 16) for k in range(16)]  # one contiguous run a thread
with ThreadPoolExecutor(16) as pool:
    t0 = time.perf_counter()
    host16 = [x for part in pool.map(lambda sh: [tree_of(d) for d in sh], shards) for x in part]
    t16 = time.perf_counter() - t0
assert host16 == host1
wrong = sum(dev[d].tobytes() != host1[d] for d in range(n))

med = statistics.median(dev_ms)
per_doc = [first[d + 1] - first[d] for d in range(n)]
res = {
    "config": config, "docs": n, "ops_per_doc": ops, "grow": grow,
    "blobs": first[-1], "max_blobs_per_document": max(per_doc), "min_blobs_per_document": min(per_doc),
    "device_ms_median": round(med, 4), "device_ms_min": round(min(dev_ms), 4), "device_ms_max": round(max(dev_ms), 4),
    "device_ms_runs": [round(x, 4) for x in dev_ms],
    "device_call_wall_ms_median": round(statistics.median(wall_ms), 3),
    "host_blob_id_download_ms": round(t_download * 1e3, 3),
    "host_1_thread_ms": round(t1 * 1e3, 2), "host_16_threads_ms": round(t16 * 1e3, 2),
    "host_16_threads_over_device_kernels": round((t_download + t16) * 1e3 / med, 1),
    "host_16_threads_over_device_call_wall": round((t_download + t16) * 1e3 / statistics.median(wall_ms), 1),
    "ids_differing_from_hashlib": wrong,
}
out_dir = os.environ.get("MTR_PROFILE_DIR", os.path.join(ROOT, "profiles"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"tree_ids_{config.lower()}.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), flush=True)
sys.exit(1 if wrong else 0)
