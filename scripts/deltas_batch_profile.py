"""Delta records of many documents: one mtr_get_deltas_batch call against the loop of mtr_get_deltas calls, plus a
mtr_get_props call per MTR_DELTA_REGEN_X record where there are any (profiles/deltas_batch.json).

usage: python scripts/deltas_batch_profile.py [--docs N] [--ops N] [--wide-docs N] [--wide-ops N]
Two shapes, each on one engine state that both legs read:
  many   N documents (default 20,000) of the bench recipe (C3's writers and lag), a short batch of --ops (default 2)
         messages each, every insert / remove / annotate flagged MTR_F_DELTA: a legacy catch-up batch
  wide   N documents (default 4) with --wide-ops (default 1,024) pending local inserts with properties, each
         regenerated: two records per member, a property set per MTR_DELTA_REGEN_X record
Wall clock around the C calls with preallocated buffers: the loop leg is one mtr_get_deltas call per document into a
buffer that is large enough (no size query) and, in the wide shape, one mtr_get_props call per REGEN_X record with
len >= 0; the batched leg is the size query and the fetch (with the props part in the wide shape).  One warm-up of both
legs, then 10 runs alternating between them; median and range in ms.  The two legs' records and words are compared
before anything is timed.
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
from fluidframework_amd.synth import make_cfg, tables  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def many_engine(n, ops):
    cfg = make_cfg(n, ops, writers=8, max_lag=32)
    eng = Engine(n, max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=2 * int(cfg.text_cap) + 1024,
                 prop_words=16384, remover_cells=4096)
    eng.generate(cfg, tables(writers=8))
    b = eng.download(0, n)
    flagged = np.isin(b.ops["type"], [abi.OP_INSERT, abi.OP_REMOVE, abi.OP_ANNOTATE])
    b.ops["flags"][flagged] |= abi.F_DELTA
    eng.reset()
    eng.apply(b)
    return eng


def wide_engine(n, ops):
    it = Interner()
    logs = []
    for _ in range(n):
        log = DocLog()
        log.start_collab("local user")
        sent = [{"type": 0, "pos1": 2 * k, "seg": {"text": "ab", "props": {"k": k % 4}}} for k in range(ops)]
        for op in sent:
            log.local_op(op, it)
        for op in sent:
            log.regenerate(op)
        logs.append(log)
    eng = Engine(n, max_segments=2 * ops, heap_entries=2 * ops, text_units=8 * ops + 1024,
                 prop_words=16 * ops + 1024, remover_cells=16 * ops + 1024)  # (the pending groups' cells are remover cells)
    eng.apply(build_batch(logs, it))
    return eng


def measure(name, eng, n, with_props):
    for d in range(0, n, max(1, n // 64)):
        st, op = eng.status(d)
        assert st == 0, f"{name}: document {d}: status {st:#x} at op {op}"
    L, h = lib(), eng.h
    first = np.zeros(n + 1, dtype="<i8")
    total = int(L.mtr_get_deltas_batch(h, None, n, None, 0, first.ctypes.data, None, 0, None))
    assert total > 0, total
    cap_doc = int(np.diff(first).max())
    one = np.zeros(cap_doc, dtype=abi.DELTA_DTYPE)
    looped = np.zeros(total, dtype=abi.DELTA_DTYPE)
    out = np.zeros(total, dtype=abi.DELTA_DTYPE)
    poff = np.zeros(total + 1, dtype="<i8")
    set_words = np.zeros(64, dtype="<u4")
    words_cap = 0
    if with_props:
        assert L.mtr_get_deltas_batch(h, None, n, out.ctypes.data, total, first.ctypes.data, None, 0,
                                      poff.ctypes.data) == total
        words_cap = int(poff[total])
    words = np.zeros(max(words_cap, 1), dtype="<u4")
    looped_words = np.zeros(max(words_cap, 1), dtype="<u4")

    def loop():
        t0 = time.perf_counter()
        at = w = 0
        for d in range(n):
            k = L.mtr_get_deltas(h, d, one.ctypes.data, cap_doc)
            looped[at:at + k] = one[:k]
            if with_props:
                for r in one[:k]:
                    if r["kind"] == abi.DELTA_REGEN_X and r["len"] >= 0:
                        c = L.mtr_get_props(h, d, int(r["len"]), set_words.ctypes.data, set_words.size)
                        looped_words[w:w + c] = set_words[:c]
                        w += c
            at += k
        ms = (time.perf_counter() - t0) * 1e3
        assert at == total and w == words_cap, (at, w)
        return ms

    def batched():
        t0 = time.perf_counter()
        size = L.mtr_get_deltas_batch(h, None, n, None, 0, first.ctypes.data, None, 0, None)
        got = L.mtr_get_deltas_batch(h, None, n, out.ctypes.data, total, first.ctypes.data,
                                     words.ctypes.data if with_props else None, words_cap,
                                     poff.ctypes.data if with_props else None)
        ms = (time.perf_counter() - t0) * 1e3
        assert size == got == total, (size, got)
        return ms

    loop()
    batched()  # the warm-up, and the comparison
    assert np.array_equal(looped, out) and first[n] == total
    assert not with_props or (words_cap > 0 and np.array_equal(looped_words, words))
    lo, ba = [], []
    for _ in range(10):
        lo.append(loop())
        ba.append(batched())
    eng.close()

    def stat(x):
        return {"median_ms": round(statistics.median(x), 3), "min_ms": round(min(x), 3), "max_ms": round(max(x), 3)}

    return {"shape": name, "docs": n, "records": total, "max_records_per_doc": cap_doc, "property_words": words_cap,
            "loop_of_single_calls": stat(lo), "batched_with_size_query": stat(ba),
            "loop_over_batched": round(statistics.median(lo) / statistics.median(ba), 1)}


n_many, n_wide = arg("--docs", 20000), arg("--wide-docs", 4)
res = {"runs": 10, "shapes": [
    measure("many", many_engine(n_many, arg("--ops", 2)), n_many, False),
    measure("wide", wide_engine(n_wide, arg("--wide-ops", 1024)), n_wide, True),
]}
out_dir = os.environ.get("MTR_PROFILE_DIR", os.path.join(ROOT, "profiles"))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "deltas_batch.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), flush=True)
