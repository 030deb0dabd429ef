"""The blob-id cache on config C3: the novel build and hand-over against the host's set and the positional delta
(profiles/blob_cache_c3.json).

usage: python scripts/blob_cache_profile.py [--docs N] [--ops N] [--template-docs N]
  C3: 100,000 documents x 1,000 messages (bench.py's preset).
The summary is built once and its ids taken.  Per leg the cache holds the ids of a seeded 0 %, 1 %, 10 %, 50 % and
100 % of the documents; one warm-up then 10 runs, each after blob_cache_clear + blob_cache_add (which drop the cached
result; not timed): the device time of the novel build by HIP events (mtr_last_timing: classify + state, scan, gather)
and the wall time of summary_novel_raw into a pinned buffer (build + download).  Two references on the same engine
state in the same run:
  host set:  blob_ids_raw(0, n) and a Python set / dict over the 20-byte ids -- what a host does today before it
             downloads anything; it mostly measures Python;
  delta:     summary_delta_raw against the equivalent positional baseline (the ids of the other documents altered).
The template-fleet leg replays one small golden log into every document of a second engine (8-unit chunks), so the
distinct blobs are a handful, and runs the same three measurements with no cache.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fluidframework_amd.batch import Batch, Interner, build_batch  # noqa: E402
from fluidframework_amd.engine import Engine, pinned  # noqa: E402
from fluidframework_amd.synth import make_cfg, tables  # noqa: E402

RUNS = 11  # the first is the warm-up
DUMMY = np.full((1, 20), 0xd5, dtype="u1")


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def host_set(eng, n, cache):
    """The host's way: download the ids, then a set and a dict in Python.  Returns (wall ms, states)."""
    t0 = time.perf_counter()
    ids, _ = eng.blob_ids_raw(0, n)
    keys = ids.view("S20").ravel() if len(ids) else []
    first, states = {}, np.zeros(len(ids), dtype="u1")
    for k, key in enumerate(keys):
        if key in cache:
            continue
        states[k] = 1 if first.setdefault(key, k) == k else 2
    return (time.perf_counter() - t0) * 1e3, states


def leg(eng, n, ids, first, cached_docs, out, label):
    """One leg: the cache holds the ids of `cached_docs` (an array of documents)."""
    held = np.zeros(n, dtype=bool)
    held[cached_docs] = True
    held_blobs = np.repeat(held, np.diff(first))
    add = np.ascontiguousarray(ids[held_blobs])
    base = ids.copy()
    base[~held_blobs, 0] ^= 0x5a  # the positional baseline that calls the same documents unchanged
    cache = set(add.view("S20").ravel().tolist()) if len(add) else set()
    cls, scan, gather, wall, host, delta = [], [], [], [], [], []
    for _ in range(RUNS):
        eng.blob_cache_add(DUMMY)  # (a changed set drops the cached result, also where the leg's cache is empty)
        eng.blob_cache_clear()
        eng.blob_cache_add(add)
        t0 = time.perf_counter()
        buf, state, rep, off, _ = eng.summary_novel_raw(0, n, out)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = eng.timing()
        cls.append(t["novel_classify_ms"])
        gather.append(t["novel_gather_ms"])
        scan.append(t["novel_ms"] - t["novel_classify_ms"] - t["novel_gather_ms"])
        ms, states = host_set(eng, n, cache)
        host.append(ms)
        assert np.array_equal(states, state), "the device states differ from the host set's"
        eng.set_baseline((base, first))
        t0 = time.perf_counter()
        _, flags, doff, _ = eng.summary_delta_raw(0, n, out)
        delta.append((time.perf_counter() - t0) * 1e3)
    row = {"leg": label, "cache_ids": eng.blob_cache_size(), "blobs": int(len(state)),
           "first_occurrences": int((state == 1).sum()), "repeats": int((state == 2).sum()),
           "novel_bytes": int(off[-1]), "classify_ms": spread(cls[1:]), "scan_ms": spread(scan[1:]),
           "gather_ms": spread(gather[1:]), "novel_wall_ms": spread(wall[1:]),
           "host_set_wall_ms": spread(host[1:]), "delta_changed_blobs": int(flags.sum()),
           "delta_bytes": int(doff[-1]), "delta_wall_ms": spread(delta[1:])}
    print(json.dumps(row), flush=True)
    return row


n, ops, tn = arg("--docs", 100000), arg("--ops", 1000), arg("--template-docs", 100000)
res = {"config": "C3", "docs": n, "ops_per_doc": ops, "runs": RUNS - 1, "legs": []}
if n:
    cfg = make_cfg(n, ops, writers=8, max_lag=32)
    eng = Engine(n, max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=2 * int(cfg.text_cap) + 1024,
                 prop_words=16384, remover_cells=4096, ops_per_launch=48)
    eng.generate(cfg, tables(writers=8))
    assert eng.stats()["bad_docs"] == 0
    eng.summarize()
    ids, first = eng.blob_ids_raw(0, n)
    ids = ids.copy()
    res["summary_bytes"] = total = eng.summary_bytes()
    out = pinned(total + 16, "u1")
    order = np.random.default_rng(0xcac4e).permutation(n)
    for pct in (0, 1, 10, 50, 100):
        res["legs"].append(leg(eng, n, ids, first, order[:n * pct // 100], out, f"C3, cache of {pct} % of the documents"))
    eng.close()
    del out

if tn:
    from fixtures import load_replay, replay_files, replay_log

    groups = load_replay([p for p in replay_files() if "len_8-clients_2" in p][0])
    it = Interner()
    log = replay_log(groups, it)
    for g in groups[:16]:
        for m in g["msgs"]:
            log.message(m, it)
    one = build_batch([log], it)
    docs = np.repeat(one.docs, tn)  # every document: its own copy of the one log's records and text
    docs["op_begin"] = np.arange(tn, dtype="<u8") * len(one.ops)
    docs["text_base"] = np.arange(tn, dtype="<u8") * len(one.text)
    fleet = Batch(docs, np.tile(one.ops, tn), np.tile(one.text, tn), one.propop_off, one.propop_kv, one.key_off,
                  one.key_bytes, one.key_index, one.val_off, one.val_bytes, one.val_eq, one.client_off,
                  one.client_bytes)
    eng = Engine(tn, chunk_size=8, max_segments=1024, heap_entries=1024, text_units=1 << 12, prop_words=1 << 10,
                 remover_cells=1 << 10)
    eng.apply(fleet)
    assert eng.stats()["bad_docs"] == 0
    eng.summarize()
    ids, first = eng.blob_ids_raw(0, tn)
    ids = ids.copy()
    total = eng.summary_bytes()
    res["template"] = {"docs": tn, "messages_per_doc": int(len(one.ops)), "summary_bytes": int(total),
                       "distinct_blobs": int(len(np.unique(ids.view("S20"))))}
    out = pinned(total + 16, "u1")
    res["legs"].append(leg(eng, tn, ids, first, np.zeros(0, dtype="i8"), out, "template fleet, no cache"))
    eng.close()

out_dir = os.environ.get("MTR_PROFILE_DIR", os.path.join(ROOT, "profiles"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "blob_cache_c3.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), flush=True)
