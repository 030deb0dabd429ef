"""Local references of many documents: one mtr_get_refs call against the loop of mtr_get_ref_states calls
(profiles/refs_batch.json).

usage: python scripts/refs_batch_profile.py [--docs N] [--wide-docs N]
Two shapes, each on one engine state that both legs read:
  many   N documents (default 20,000) of one segment with 4 references each: the summarizer's interval headers
  wide   N documents (default 16) of 200 leaves with 512 references each: a document after long interval churn
Wall clock around the C calls, which end in a stream synchronisation, with preallocated buffers: the loop leg is one
mtr_get_ref_states call per document into a buffer that is large enough (no size query); the batched leg is the size
query and the fetch.  One warm-up of both legs, then 10 runs alternating between them; median and range in ms.  The
two legs' words are compared before anything is timed.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidframework_amd import abi  # noqa: E402
from fluidframework_amd.batch import DocLog, Interner, build_batch  # noqa: E402
from fluidframework_amd.engine import Engine, lib  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def msg(op, seq):
    return {"clientId": "w", "sequenceNumber": seq, "referenceSequenceNumber": seq - 1, "minimumSequenceNumber": 0,
            "type": "op", "contents": op}


def document(it, leaves, refs):
    log = DocLog()
    log.start_collab("me")
    for i in range(leaves):  # (a trailing newline: the segments stay apart)
        log.message(msg({"type": 0, "pos1": 2 * i, "seg": "a\n"}, i + 1), it)
    for r in range(refs):
        log.create_ref((r * 7) % (2 * leaves), abi.REFTYPE_SLIDE_ON_REMOVE)
    return log


def measure(name, n, leaves, refs, caps):
    it = Interner()
    eng = Engine(n, **caps)
    eng.apply(build_batch([document(it, leaves, refs) for _ in range(n)], it))
    assert all(eng.status(d)[0] == 0 for d in range(0, n, max(1, n // 64)))
    L, h = lib(), eng.h
    one = np.zeros(2 * refs, dtype="<i4")
    looped = np.zeros(2 * refs * n, dtype="<i4")
    first = np.zeros(n + 1, dtype="<i8")
    out = np.zeros(2 * refs * n, dtype="<i4")

    def loop():
        t0 = time.perf_counter()
        for d in range(n):
            k = L.mtr_get_ref_states(h, d, one.ctypes.data, one.size)
            looped[2 * refs * d:2 * refs * d + 2 * k] = one[:2 * k]
        return (time.perf_counter() - t0) * 1e3

    def batched():
        t0 = time.perf_counter()
        total = L.mtr_get_refs(h, None, n, abi.REFS_STATES, None, 0, first.ctypes.data)
        got = L.mtr_get_refs(h, None, n, abi.REFS_STATES, out.ctypes.data, out.size, first.ctypes.data)
        ms = (time.perf_counter() - t0) * 1e3
        assert total == got == n * refs, (total, got)
        return ms

    loop()
    batched()  # the warm-up, and the comparison
    assert np.array_equal(looped, out) and first[n] == n * refs
    lo, ba = [], []
    for _ in range(10):
        lo.append(loop())
        ba.append(batched())
    eng.close()

    def stat(x):
        return {"median_ms": round(statistics.median(x), 3), "min_ms": round(min(x), 3), "max_ms": round(max(x), 3)}

    return {"shape": name, "docs": n, "leaves_per_doc": leaves, "refs_per_doc": refs, "loop_of_single_calls": stat(lo),
            "batched_with_size_query": stat(ba),
            "loop_over_batched": round(statistics.median(lo) / statistics.median(ba), 1)}


res = {"mode": "MTR_REFS_STATES", "runs": 10, "shapes": [
    measure("many", arg("--docs", 20000), 1, 4,
            dict(max_segments=128, heap_entries=128, text_units=512, prop_words=256, remover_cells=256, ref_slots=64)),
    measure("wide", arg("--wide-docs", 16), 200, 512,
            dict(max_segments=1024, heap_entries=1024, text_units=4096, prop_words=256, remover_cells=256,
                 ref_slots=1024)),
]}
out_dir = os.environ.get("MTR_PROFILE_DIR", os.path.join(ROOT, "profiles"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "refs_batch.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), flush=True)
