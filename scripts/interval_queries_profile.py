"""Viewport overlap queries of live clients: the batched device call against the Transient path it replaces
(profiles/interval_queries.json).

usage: python scripts/interval_queries_profile.py [--runs R] [--out PATH] [--shapes many one]
       python scripts/interval_queries_profile.py --trace B T     (for a kernel / copy trace: see below)
Two shapes, each a LiveSession on one engine, every client a collaborating SharedString of PIECES separately inserted
pieces of text with one interval collection of SlideOnRemove intervals a few units long:
  many:  256 resident documents with 32 intervals each, 4 viewport queries (40 units wide) a document: 1,024 queries;
  one:   one document with 4,096 intervals, 64 viewport queries.
Timed, wall clock around calls that end in a stream synchronise, one warm-up then R runs (default 10) that alternate
between the legs:
  batched:      LiveSession.query_intervals -- one mtr_query_intervals for every client's queries, then the host's sort
                of each query's hits into compare order;
  batched_call: Engine.query_intervals alone (the C call and its buffers, no host ordering), timed in the same rounds;
  transient:    today's path, for all clients in one step: two Transient MTR_OP_REF_CREATE records a query, one sync (one
                batch build and apply for every client), one ref_keys_many download of every reference key, then per
                collection the cmp_to_key sort and per query the filter over the whole collection; the ids released.
                This is find_overlapping_intervals_many's body run over all clients at once, so that it pays one apply
                where a loop over the clients would pay one each.
The answers of the two legs (interval ids per query, in order) are compared once before the timing.  Apply launches a
call are read from mtr_debug_launch_counts around one call of each leg.
--trace B T runs the `one` shape, then B batched_call calls and T transient calls and exits, for rocprofv3
--kernel-trace --memory-copy-trace: the difference between two such runs that differ in B (or T) by one is one call's
kernels and copies.
Not measured: the split of the batched call between its kernels and its copies, and sets larger than one wave walks
well (one wave takes a set 64 intervals a round).
"""
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidframework_amd import abi  # noqa: E402
from fluidframework_amd.intervals import _ref_key  # noqa: E402
from fluidframework_amd.live import EngineExecutor, LiveSession  # noqa: E402

PIECES, PIECE = 96, 12  # text of a document: 96 pieces of 12 units
SLIDE = 2               # IntervalType.SlideOnRemove
WIDTH = 40              # a viewport, in units
SHAPES = {"many": dict(docs=256, intervals=32, queries=4), "one": dict(docs=1, intervals=4096, queries=64)}
PATH = os.path.join(ROOT, "profiles", "interval_queries.json")


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


def session(executor, docs, intervals, seed=7):
    """-> (session, the clients' collections); every interval add applied."""
    rnd = random.Random(seed)
    s = LiveSession(executor)
    colls = []
    for d in range(docs):
        c = s.client(f"c{d}")
        for p in range(PIECES):
            c.log.local_insert(rnd.randrange(PIECE * p + 1), "".join(chr(97 + (p + u) % 26) for u in range(PIECE)), s.it)
        c.connect(f"c{d}")
        hc = c.get_interval_collection("comments")
        for k in range(intervals):
            a = rnd.randrange(PIECES * PIECE - 8)
            hc.add(a, a + rnd.randrange(1, 8), SLIDE, {"intervalId": f"i{k:05d}"})
        colls.append(hc)
    s.sync()
    return s, colls


def viewports(colls, queries, seed=11):
    rnd = random.Random(seed)
    return [(hc, a, a + WIDTH) for hc in colls for a in (rnd.randrange(PIECES * PIECE - WIDTH) for _ in range(queries))]


def transient(s, requests):
    """Today's path for every request of every client in one step (module docstring)."""
    per, made = {}, {}
    for hc, a, b in requests:
        per.setdefault(id(hc), (hc, []))[1].append((a, b))
    for key, (hc, ranges) in per.items():
        log = hc.client.log
        made[key] = [(log.create_ref(a, abi.REFTYPE_TRANSIENT), log.create_ref(b, abi.REFTYPE_TRANSIENT)) for a, b in ranges]
    keys_all = s.ref_keys_many([hc.client for hc, _ in per.values()])
    out = {}
    for (key, (hc, ranges)), keys in zip(per.items(), keys_all):
        ordered = hc.coll.ordered(keys)
        for (a, b), (ts, te) in zip(ranges, made[key]):
            ks, ke = _ref_key(keys, ts), _ref_key(keys, te)
            out[(key, a, b)] = [iv for iv in ordered if _ref_key(keys, iv.start) <= ke and _ref_key(keys, iv.end) >= ks]
        for ts, te in reversed(made[key]):
            hc.client.log.release_ref(te, remove=False)
            hc.client.log.release_ref(ts, remove=False)
    return [out[(id(hc), a, b)] for hc, a, b in requests]


def raw_inputs(colls, requests):
    """The sets, reference ids and queries LiveSession.query_intervals sends for `requests`."""
    sets, refs, index = [], [], {}
    for hc in colls:
        members = list(hc.coll.by_id.values())
        index[id(hc)] = len(sets)
        sets.append((hc.client.doc, len(refs), len(members)))
        refs += [(iv.start, iv.end) for iv in members]
    return sets, np.array(refs, dtype="<u4"), [(index[id(hc)], a, b, abi.IVQ_OVERLAP) for hc, a, b in requests]


def engine_for(shape):
    from fluidframework_amd.engine import Engine

    return Engine(shape["docs"], max_segments=1024, heap_entries=1024, text_units=1 << 13, prop_words=1 << 10,
                  remover_cells=1 << 10, ref_slots=2 * shape["intervals"] + 2 * shape["queries"] + 64)


def measure(name, runs):
    shape = SHAPES[name]
    eng = engine_for(shape)
    s, colls = session(EngineExecutor(eng), shape["docs"], shape["intervals"])
    requests = viewports(colls, shape["queries"])
    device = [(hc, a, b, abi.IVQ_OVERLAP) for hc, a, b in requests]
    sets, refs, queries = raw_inputs(colls, requests)

    def timed(fn):
        t0 = time.perf_counter()
        res = fn()
        return (time.perf_counter() - t0) * 1e3, res

    legs = {"batched": lambda: s.query_intervals(device), "batched_call": lambda: eng.query_intervals(sets, refs, queries),
            "transient": lambda: transient(s, requests)}
    got, want = legs["batched"](), legs["transient"]()  # (also the warm-up)
    assert [[iv.id() for iv in x] for x in got] == [[iv.id() for iv in x] for x in want]
    legs["batched_call"]()
    applies = {}
    for leg in ("batched", "transient"):
        before = eng.launch_counts()["launches"]
        legs[leg]()
        applies[leg] = eng.launch_counts()["launches"] - before
    ms = {leg: [] for leg in legs}
    for _ in range(runs):
        for leg, fn in legs.items():
            ms[leg].append(timed(fn)[0])
    res = {"shape": name, **shape, "total_queries": len(requests), "hits": sum(len(x) for x in got), "runs": runs,
           "apply_launches_per_call": applies}
    res.update({leg + "_wall_ms": spread(v) for leg, v in ms.items()})
    res["transient_over_batched_median"] = round(statistics.median(ms["transient"]) / statistics.median(ms["batched"]), 2)
    eng.close()
    return res


def trace(b, t):
    shape = SHAPES["one"]
    eng = engine_for(shape)
    s, colls = session(EngineExecutor(eng), shape["docs"], shape["intervals"])
    requests = viewports(colls, shape["queries"])
    sets, refs, queries = raw_inputs(colls, requests)
    for _ in range(b):
        eng.query_intervals(sets, refs, queries)
    for _ in range(t):
        transient(s, requests)
    eng.close()


def main():
    if "--trace" in sys.argv:
        trace(*args("--trace", [1, 1]))
        return
    runs = args("--runs", [10])[0]
    path = args("--out", [PATH], str)[0]
    out = {"workload": f"live SharedString clients ({PIECES} pieces of {PIECE} units), one collection of SlideOnRemove "
                       f"intervals a document, viewport overlap queries {WIDTH} units wide", "legs": [],
           "not_measured": ["the split of the batched call between its kernels and its copies",
                            "sets beyond what one wave walks well"]}
    for name in args("--shapes", ["many", "one"], str):
        res = measure(name, runs)
        print(json.dumps(res), flush=True)
        out["legs"].append(res)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
