"""mtr_query_intervals: findOverlappingIntervals, previousInterval and nextInterval of many interval collections of many
documents in one read-only call.

The call is defined by the calls that exist (include/mtr.h): K(r) from Engine.ref_keys of the document, T(p) the key of
a real Transient reference created at p through the existing path (MTR_OP_REF_CREATE at the local view) on a copy of
the same log, applied on a second engine.  `compose` states the three predicates over those keys once (the filter of
LiveIntervalCollection.find_overlapping_intervals_many, the floor / ceil of previous_interval / next_interval), and
every check compares all eight words of every hit, hit_first and status with it, exactly.  The batch is never compared
with itself.

Documents: hand-made ones of exactly 1, 63, 64, 65 and 130 leaves (test_position_transforms' _edge_log: two whole
leaves removed late) with references of every kind created before that removal -- sliding ones leave the removed
leaves, simple ones are let go (key -1), StayOnRemove ones stay on the removed, still linked leaves --, test_refs_batch's
130-reference document (zamboni unlinked segments under references: key -2), the hole-layout HBM document, and the
interval farm through the live host.
"""
import copy
import os
import random
import re

import numpy as np
import pytest

import interval_farm as F
from fluidframework_amd import abi
from fluidframework_amd.batch import DocLog, Interner, build_batch
from fluidframework_amd.intervals import IntervalUnsupported

gpu = pytest.mark.gpu

OVERLAP, PREVIOUS, NEXT = abi.IVQ_OVERLAP, abi.IVQ_PREVIOUS, abi.IVQ_NEXT
PATTERN = 0x5a5a5a5a
EDGE_LEAVES = (1, 63, 64, 65, 130)
SET_SIZES = (0, 1, 31, 32, 33, 63, 64, 65, 130)
SLIDE, SIMPLE, STAY, TRANSIENT = (abi.REFTYPE_SLIDE_ON_REMOVE, abi.REFTYPE_SIMPLE, abi.REFTYPE_STAY_ON_REMOVE,
                                  abi.REFTYPE_TRANSIENT)


# ---------------------------------------------------------------- the reference: the composition of include/mtr.h
def ref_key(row):
    """intervals._ref_key of one Engine.ref_keys row (position, state bits, key, offset); -2 has no place in the order."""
    assert row[2] != -2
    return (0, 0, 0) if row[2] == -1 else (1, row[2], row[3])


def compose(keys, ivs, ts, te, mode, in_order=True):
    """(status, hits) of one query by the contract.  keys: Engine.ref_keys of the set's document; ivs: the set's
    (start ref, end ref) pairs; ts, te: T(start), T(end) as tuples; in_order: end >= start."""
    if any(keys[r][2] == -2 for iv in ivs for r in iv):
        return abi.IVQ_UNLINKED, []

    def row(k, flags=0):
        s, e = ivs[k]
        return (k, keys[s][0], keys[e][0], keys[s][2], keys[s][3], keys[e][2], keys[e][3], flags)

    if mode == OVERLAP:
        if not in_order:
            return 0, []
        return 0, [row(k) for k, (s, e) in enumerate(ivs) if ref_key(keys[s]) <= te and ref_key(keys[e]) >= ts]
    ends = [ref_key(keys[e]) for _, e in ivs]
    cand = [x for x in ends if (x <= ts if mode == PREVIOUS else x >= ts)]
    if not cand:
        return 0, []
    best = max(cand) if mode == PREVIOUS else min(cand)
    return 0, [row(ends.index(best), abi.IVQ_TIE if ends.count(best) > 1 else 0)]


def test_composition_on_a_hand_computed_example():
    """The yardstick itself.  Four references: 0 detached, 1 at (leaf 2, offset 1), 2 at (leaf 5, 0), 3 at (leaf 5, 0)
    again; intervals 0 = [0, 1], 1 = [1, 2], 2 = [1, 3]."""
    keys = [(-1, 0, -1, 0), (7, 3, 2, 1), (15, 3, 5, 0), (15, 3, 5, 0)]
    ivs = [(0, 1), (1, 2), (1, 3)]
    hit = lambda k, f=0: (k,) + {0: (-1, 7, -1, 0, 2, 1), 1: (7, 15, 2, 1, 5, 0), 2: (7, 15, 2, 1, 5, 0)}[k] + (f,)  # noqa: E731
    at = lambda leaf, off: (1, leaf, off)  # noqa: E731
    assert compose(keys, ivs, at(0, 0), at(1, 2), OVERLAP) == (0, [hit(0)])       # ends before intervals 1, 2 start
    assert compose(keys, ivs, at(2, 1), at(2, 1), OVERLAP) == (0, [hit(0), hit(1), hit(2)])
    assert compose(keys, ivs, at(2, 2), at(9, 0), OVERLAP) == (0, [hit(1), hit(2)])
    assert compose(keys, ivs, at(5, 1), (0, 0, 0), OVERLAP) == (0, [])            # starts past every end
    assert compose(keys, ivs, (0, 0, 0), (0, 0, 0), OVERLAP) == (0, [hit(0)])     # no segment: only a detached start
    assert compose(keys, ivs, at(2, 1), at(2, 1), OVERLAP, in_order=False) == (0, [])
    assert compose(keys, ivs, at(2, 1), None, PREVIOUS) == (0, [hit(0)])
    assert compose(keys, ivs, at(2, 0), None, PREVIOUS) == (0, [])
    assert compose(keys, ivs, at(9, 0), None, PREVIOUS) == (0, [hit(1, abi.IVQ_TIE)])  # two intervals end at (5, 0)
    assert compose(keys, ivs, at(2, 2), None, NEXT) == (0, [hit(1, abi.IVQ_TIE)])
    assert compose(keys, ivs, (0, 0, 0), None, NEXT) == (0, [hit(0)])
    assert compose(keys, ivs, at(5, 1), None, NEXT) == (0, [])
    keys[2] = (-1, 1, -2, 0)
    assert compose(keys, ivs, at(0, 0), at(9, 0), OVERLAP) == (abi.IVQ_UNLINKED, [])


def test_abi_mirror_matches_the_header():
    """abi.py's three dtypes against the layouts include/mtr.h declares (parsed from the header's own struct bodies),
    and the constants."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "include", "mtr.h")).read()
    for name, dtype, size in (("mtr_interval_set", abi.INTERVAL_SET_DTYPE, 12),
                              ("mtr_interval_query", abi.INTERVAL_QUERY_DTYPE, 16),
                              ("mtr_interval_hit", abi.INTERVAL_HIT_DTYPE, 32)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            m = re.match(r"\s*(u?int32_t)\s+(.*)", decl.strip(), re.S)
            if m:
                fields += [(f.strip(), m.group(1)) for f in m.group(2).split(",")]
        assert [f for f, _ in fields] == list(dtype.names), (name, fields)
        assert dtype.itemsize == size == 4 * len(fields)
        for k, (f, ty) in enumerate(fields):
            assert dtype.fields[f][1] == 4 * k and dtype.fields[f][0] == np.dtype("<u4" if ty == "uint32_t" else "<i4")
    for macro, value in (("MTR_IVQ_OVERLAP", OVERLAP), ("MTR_IVQ_PREVIOUS", PREVIOUS), ("MTR_IVQ_NEXT", NEXT),
                         ("MTR_IVQ_TIE", abi.IVQ_TIE), ("MTR_IVQ_UNLINKED", abi.IVQ_UNLINKED)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, src).group(1)) == value


def test_abi_mirror_matches_the_compiled_layout(tmp_path):
    """abi.py's three dtypes against sizeof / offsetof of the structs as a C++ compiler lays them out from
    include/mtr.h (the header test above reads the header's text alone)."""
    import shutil
    import subprocess

    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    structs = (("mtr_interval_set", abi.INTERVAL_SET_DTYPE), ("mtr_interval_query", abi.INTERVAL_QUERY_DTYPE),
               ("mtr_interval_hit", abi.INTERVAL_HIT_DTYPE))
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "mtr.h"', "int main() {"]
    for name, dtype in structs:
        lines.append(f'    std::printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    std::printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in dtype.names]
    src = tmp_path / "layout.cc"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "layout")
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(root, "include"), "-o", exe, str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for name, dtype in structs:
        assert int(got[name]) == dtype.itemsize, name
        for f in dtype.names:
            assert int(got[f"{name}.{f}"]) == dtype.fields[f][1] and dtype.fields[f][0].itemsize == 4, (name, f)


def test_oracle_executor_keeps_the_transient_path():
    """An executor without query_intervals (the oracle's) answers as before, through Transient references, and the new
    previous_intervals_many / next_intervals_many fall back to the single queries."""
    from fluidframework_amd.live import LiveSession
    from mock_runtime import OracleExecutor

    init, msgs, obs = F.farm(1)
    ex = OracleExecutor()
    assert not hasattr(ex, "query_intervals")
    s = LiveSession(ex)
    c = s.client("observer")
    c.log.local_insert(0, init, s.it)
    c.connect("observer")
    for m in msgs:
        c.process(dict(m), False)
    n, created, create = len(obs.text()), [], c.log.create_ref
    compared = refused = 0
    c.log.create_ref = lambda *a, **k: (created.append(a), create(*a, **k))[1]
    for label in obs.data:
        hc, oc = c.get_interval_collection(label), obs.data[label]
        for a in range(0, n, 7):
            b = min(n - 1, a + 5)
            queued = len(created)
            got = [iv.id() for iv in hc.find_overlapping_intervals_many([(a, b)])[0]]
            assert got == [iv.interval_id() for iv in oc.find_overlapping(a, b)]
            if hc.coll.by_id and b >= a:  # (two Transient records were queued)
                assert [x[1] for x in created[queued:]] == [abi.REFTYPE_TRANSIENT] * 2
        for many, one in ((hc.previous_intervals_many, hc.previous_interval), (hc.next_intervals_many, hc.next_interval)):
            try:
                want = [one(0), one(n // 2)]
            except IntervalUnsupported:  # (the whole-collection refusal: the fall-back refuses with it)
                with pytest.raises(IntervalUnsupported):
                    many([0, n // 2])
                refused += 1
                continue
            assert many([0, n // 2]) == want
            compared += 1
    print(f"previous / next: compared {compared}, refused {refused}")
    assert created and compared > 0


# ---------------------------------------------------------------- the raw call
def _lib():
    from fluidframework_amd.engine import lib
    return lib()


def _err():
    return _lib().mtr_last_error().decode()


def raw(eng, sets, refs, qs, hits=True, cap=None):
    """mtr_query_intervals into patterned buffers: a size query, then the fetch into a buffer of exactly the size (or
    `cap` rows) -> (return value, hit_first, status, rows [total, 8])."""
    s = np.array([tuple(x) for x in sets], dtype=abi.INTERVAL_SET_DTYPE).reshape(-1)
    r = np.ascontiguousarray(refs, dtype="<u4").reshape(-1)
    q = np.array([tuple(x) for x in qs], dtype=abi.INTERVAL_QUERY_DTYPE).reshape(-1)
    n = int(q.size)
    first = np.full(n + 1, PATTERN, dtype="<i8")
    status = np.full(max(n, 1), PATTERN, dtype="<i4")

    def call(out, c):
        return int(_lib().mtr_query_intervals(eng.h, s.ctypes.data if s.size else None, s.size,
                                              r.ctypes.data if r.size else None, r.size // 2,
                                              q.ctypes.data if n else None, n, first.ctypes.data, status.ctypes.data,
                                              None if out is None else out.ctypes.data, c))

    total = call(None, 0)
    if total < 0 or not hits:
        return total, first, status, np.zeros((0, 8), dtype="<i4")
    size = first.copy()
    rows = np.full((max(total if cap is None else cap, 0) + 1, 8), PATTERN, dtype="<i4")
    rc = call(rows, total if cap is None else cap)
    assert np.array_equal(first, size)
    if rc >= 0:
        assert rc == total and (rows[total:] == PATTERN).all()  # (nothing past the rows)
        rows = rows[:total]
    return rc, first, status, rows


# ---------------------------------------------------------------- the documents
def _msg(client, op, seq, ref, msn=0):
    return {"clientId": client, "sequenceNumber": seq, "referenceSequenceNumber": ref, "minimumSequenceNumber": msn,
            "type": "op", "contents": op}


def _edge_doc(it, leaves, rnd, n_refs=48):
    """test_position_transforms' _edge_log with n_refs references of every kind created before its late removal of
    leaves 8 and 9 (every fourth reference on those leaves) -> (log, the local view's length after the removal)."""
    from test_position_transforms import _edge_log

    if leaves < 10:  # (nothing to remove: one marker-free leaf)
        log = DocLog()
        log.start_collab("me")
        log.message(_msg("w", {"type": 0, "pos1": 0, "seg": {"text": "abc" * leaves}}, 1, 0), it)
        for r in range(n_refs):
            log.create_ref(r % 3, (SLIDE, SIMPLE, STAY)[r % 3])
        return log, 3 * leaves
    log, lens = _edge_log(it, leaves)
    last_insert = max(k for k, op in enumerate(log.ops) if op[0] == abi.OP_INSERT)
    tail = log.ops[last_insert + 1:]  # the removal's records
    del log.ops[last_insert + 1:]
    total, gone = sum(lens), sum(lens[:8])
    for r in range(n_refs):
        pos = gone + rnd.randrange(lens[8] + lens[9]) if r % 4 == 0 else rnd.randrange(total)
        pos = {1: total - 1, 2: 0}.get(r, pos)  # (the last leaf and the first hold a reference)
        log.create_ref(pos, (SLIDE, SIMPLE, STAY)[r % 3])
    log.ops.extend(tail)
    return log, total - lens[8] - lens[9]


def _transient_keys(logs, it, positions, **caps):
    """T(p) for every (doc, p) of `positions`: real Transient references at the local view, created through the
    existing path on a copy of the logs and applied on an engine of their own."""
    from fluidframework_amd.engine import Engine

    logs = copy.deepcopy(logs)  # (with their records: copied before a batch was built from them)
    ids = {(d, p): logs[d].create_ref(p, TRANSIENT) for d, p in sorted(positions)}
    eng = Engine(len(logs), **caps)
    eng.apply(build_batch(logs, it))
    keys = []
    for d in range(len(logs)):
        st, op = eng.status(d)
        assert st == 0, f"document {d}: status {st:#x} at op {op}"
        keys.append(eng.ref_keys(d))
    eng.close()
    return {(d, p): ref_key(keys[d][r]) for (d, p), r in ids.items()}


def _positions(n):
    """Query positions of a view of length n: the ends, outside it, and places in different 64-leaf rounds."""
    return sorted({-3, -1, 0, 1, 2, n // 3, n // 2, n - 2, n - 1, n, n + 1, n + 40,
                   min(n, 64 * 3 - 40), min(n, 64 * 3 - 39), min(n, 64 * 3 - 20)})


def _queries(si, n):
    ps = _positions(n)
    qs = [(si, p, p, mode) for p in ps for mode in (PREVIOUS, NEXT)]
    qs += [(si, p, p, OVERLAP) for p in ps]                                  # start and end in one leaf
    qs += [(si, a, b, OVERLAP) for a in ps[::2] for b in ps[1::3]]           # different rounds, end < start included
    qs += [(si, 0, n, OVERLAP), (si, 0, 0x7fffffff, OVERLAP), (si, -0x80000000, n, OVERLAP)]
    return qs


class _Fleet:
    pass


CAPS = dict(max_segments=4096, heap_entries=4096, text_units=1 << 14, prop_words=1 << 12, remover_cells=1 << 12,
            ops_per_launch=64)
UNLINKED_DOC = len(EDGE_LEAVES)


@pytest.fixture(scope="module")
def fleet():
    from fluidframework_amd.engine import Engine
    from test_refs_batch import _big_doc

    rnd = random.Random(0x1e7)
    it = Interner()
    f = _Fleet()
    built = [_edge_doc(it, n, rnd) for n in EDGE_LEAVES]
    f.logs = [b[0] for b in built] + [_big_doc(it)]
    pristine = copy.deepcopy(f.logs)  # (building a batch takes the records out of a log)
    f.eng = Engine(len(f.logs) + 1, ref_slots=256, **CAPS)
    f.eng.apply(build_batch(f.logs, it))
    for d in range(len(f.logs)):
        st, op = f.eng.status(d)
        assert st == 0, f"document {d}: status {st:#x} at op {op}"
    f.keys = [f.eng.ref_keys(d) for d in range(len(f.logs))]  # K, read once
    # the sets: every size on some document, two sets on one document, listed in another order than the documents'
    f.sets, f.refs = [], []
    order = [(d, size) for d, size in zip((3, 0, 4, 1, 2, 4, 0, 3, 4), SET_SIZES)] + [(1, 40), (UNLINKED_DOC, 65)]
    for d, size in order:
        if d == UNLINKED_DOC:
            ivs = [(2 * k, 2 * k + 1) for k in range(size)]
        else:
            ivs = [(rnd.randrange(48), rnd.randrange(48)) for _ in range(size)]
        f.sets.append((d, len(f.refs), size))
        f.refs += ivs
    f.qs = []
    for si, (d, _, _) in enumerate(f.sets):
        n = built[d][1] if d < len(built) else 140
        f.qs += _queries(si, n)
    rnd.shuffle(f.qs)
    f.t = _transient_keys(pristine, it, {(f.sets[s][0], p) for s, a, b, _ in f.qs for p in (a, b)}, ref_slots=512, **CAPS)
    yield f
    f.eng.close()


def _expected(f, q):
    s, a, b, mode = q
    d, first, count = f.sets[s]
    return compose(f.keys[d], f.refs[first:first + count], f.t[(d, a)], f.t[(d, b)], mode, b >= a)


def _compare(f, qs):
    rc, first, status, rows = raw(f.eng, f.sets, f.refs, qs)
    assert rc >= 0, _err()
    at = 0
    for i, q in enumerate(qs):
        st, want = _expected(f, q)
        assert first[i] == at and status[i] == st, f"query {i} {q}: hit_first {first[i]} status {status[i]}, not {at}, {st}"
        got = [tuple(int(x) for x in r) for r in rows[at:at + len(want)]]
        assert got == want and first[i + 1] == at + len(want), f"query {i} {q}: {got} != {want}"
        at += len(want)
    assert rc == at == first[len(qs)]
    return rows, status, first


@gpu
def test_fleet_holds_the_states_the_queries_must_answer(fleet):
    keys = [np.array(k).reshape(-1, 4) for k in fleet.keys]
    assert any((k[:, 2] == -1).any() for k in keys[1:UNLINKED_DOC])                       # let go: no segment
    assert any(((k[:, 1] & abi.REF_ST_REMOVED) != 0).any() for k in keys[1:UNLINKED_DOC])  # on a removed, linked leaf
    assert (keys[UNLINKED_DOC][:, 2] == -2).any()
    assert max(k[:, 2].max() for k in keys) >= 128                                         # a third leaf round
    ts = [t for t in fleet.t.values()]
    assert (0, 0, 0) in ts and max(t[1] for t in ts) >= 128 and any(t[2] > 0 for t in ts)


@gpu
def test_every_query_against_the_composition(fleet):
    rows, status, first = _compare(fleet, fleet.qs)
    assert len(rows) > len(fleet.qs) and (rows[:, 7] == abi.IVQ_TIE).any() and (status == abi.IVQ_UNLINKED).any()
    answered = {fleet.sets[q[0]][2] for i, q in enumerate(fleet.qs) if first[i + 1] > first[i]}
    assert answered >= set(SET_SIZES) - {0}  # (every set size had hits to place)


@gpu
def test_one_set_many_times_and_single_queries(fleet):
    """One set asked many times in one call, and every query of it alone: the same rows either way."""
    si = SET_SIZES.index(65)
    qs = [q for q in fleet.qs if q[0] == si]
    rows, _, _ = _compare(fleet, qs * 3)
    assert len(rows) % 3 == 0 and np.array_equal(rows[:len(rows) // 3], rows[len(rows) // 3:2 * len(rows) // 3])
    for q in qs[:12]:
        _compare(fleet, [q])


@gpu
def test_unlinked_set_does_not_hide_the_others(fleet):
    bad = len(fleet.sets) - 1
    of = lambda s: [q for q in fleet.qs if q[0] == s]  # noqa: E731
    qs = of(bad)[:3] + of(2)[:20] + of(bad)[3:6] + of(5)[:20]
    rows, status, _ = _compare(fleet, qs)
    assert status.tolist().count(abi.IVQ_UNLINKED) == 6 and len(rows) > 0


@gpu
def test_hole_layout_document():
    """test_refs_batch's hole-layout document (more slots than leaves past 8,192): T's leaf is a slot index, as
    ref_query's key is, not containing's live-leaf ordinal -- the two differ behind the holes."""
    from fluidframework_amd.engine import Engine
    from test_local_refs import ins, rem

    rnd = random.Random(0x8e5)
    it = Interner()
    log = DocLog()
    log.start_collab("me")
    leaves = 8192 + 160
    for i in range(leaves):
        log.message(_msg("w", ins(rnd.randint(0, i), "x"), i + 1, i), it)
    for r in range(70):
        log.create_ref((r * 119) % leaves, (SLIDE, SIMPLE, STAY, TRANSIENT)[r % 4])
    log.message(_msg("w", rem(100, 400), leaves + 1, leaves), it)
    log.local_op(rem(5000, 5100), it)
    caps = dict(max_segments=16384, heap_entries=16384, text_units=1 << 15, prop_words=1 << 10, remover_cells=1 << 12,
                ref_slots=256)
    pristine = copy.deepcopy(log)
    eng = Engine(1, **caps)
    eng.apply(build_batch([log], it))
    assert eng.status(0)[0] == 0 and eng.launch_counts()["global_mode"] > 0
    assert eng.stats()["max_leaves"] > len(eng.export(0)[0]) > 8192  # more slots than leaves: holes
    f = _Fleet()
    f.eng, f.keys = eng, [eng.ref_keys(0)]
    f.sets, f.refs = [(0, 0, 35), (0, 35, 20)], [(2 * k, 2 * k + 1) for k in range(35)] + [(k, 69 - k) for k in range(20)]
    n = leaves - 400
    ps = [0, 50, 99, 100, 101, 3000, 4000, 4900, 4999, 5000, 5001, 7000, n - 1, n, n + 3, -1]
    f.qs = [(s, p, p, mode) for s in (0, 1) for p in ps for mode in (PREVIOUS, NEXT)] + \
        [(s, a, b, OVERLAP) for s in (0, 1) for a in ps[::2] for b in ps[::3]]
    f.t = _transient_keys([pristine], it, {(0, p) for p in ps}, **caps)
    _compare(f, f.qs)
    # (positions ahead of the pending local remove: any client's view at the last sequence number names the same leaf)
    ordinals = {p: eng.containing_segment(0, p, leaves + 1, -1)["leaf"] for p in (3000, 4000, 4900)}
    assert any(f.t[(0, p)][1] != o for p, o in ordinals.items())  # a slot index that is no ordinal
    eng.close()


# ---------------------------------------------------------------- the live host on the interval farm
def _host(init, msgs, executor):
    from fluidframework_amd.live import LiveSession

    s = LiveSession(executor)
    c = s.client("observer")
    c.log.local_insert(0, init, s.it)
    c.connect("observer")
    for m in msgs:
        c.process(dict(m), False)
    return c


def _ask(fn, *args):
    try:
        return fn(*args)
    except IntervalUnsupported as e:
        return e


@gpu
def test_live_queries_on_the_interval_farm():
    """Seeds 1-3 (as test_interval_queries): overlaps from the device path equal the oracle's; previous / next equal the
    oracle's trees where the end tree is whole and no tie is flagged, and equal today's host wherever that answers.
    The device path leaves out no more probes (TIE) than today's whole-collection refusal does."""
    from test_interval_live import _engine_executor

    compared = ties = refused = probes = 0
    for seed in (1, 2, 3):
        init, msgs, obs = F.farm(seed)
        c = _host(init, msgs, _engine_executor())
        n = len(obs.text())
        for label in obs.data:
            oc, hc = obs.data[label], c.get_interval_collection(label)
            ranges = [(a, min(n - 1, a + 5)) for a in range(0, n, 7)]
            created, create = [], c.log.create_ref
            c.log.create_ref = lambda *a, _f=create, **k: (created.append(a), _f(*a, **k))[1]
            c.sync()  # (everything pending is applied: what the log holds now is what the query may not add to)
            records, ids = len(c.log.ops), c.log.n_refs
            got = hc.find_overlapping_intervals_many(ranges)
            c.log.create_ref = create
            assert len(c.log.ops) == records and c.log.n_refs == ids and not created  # (the log has no new record)
            for (a, b), ivs in zip(ranges, got):
                assert [iv.id() for iv in ivs] == [iv.interval_id() for iv in oc.find_overlapping(a, b)], (label, a, b)
            whole = len(oc.end_tree.nodes()) == len(oc.tree.keys())
            for pos in range(0, n + 1, 3):
                for many, one, oracle_q in ((hc.previous_intervals_many, hc.previous_interval, oc.previous_interval),
                                            (hc.next_intervals_many, hc.next_interval, oc.next_interval)):
                    new, old = _ask(many, [pos]), _ask(one, pos)
                    probes += 1
                    ties += isinstance(new, IntervalUnsupported)
                    refused += isinstance(old, IntervalUnsupported)
                    if isinstance(new, IntervalUnsupported):
                        continue
                    if not isinstance(old, IntervalUnsupported):
                        assert (new[0].id() if new[0] else None) == (old.id() if old else None), (label, pos)
                    if whole:
                        want = oracle_q(pos)
                        compared += 1
                        assert (new[0].id() if new[0] else None) == (want.interval_id() if want else None), (label, pos)
    print(f"probes {probes}: compared {compared}, left out as TIE {ties}, refused by the whole-collection rule {refused}")
    assert ties <= refused and compared > 0


@gpu
def test_read_only_and_exact_reference_table():
    """ref_slots sized exactly to the live references: the call answers (the Transient path stops the document with
    MTR_ERR_CAPACITY), and hashes, delta records and reference keys are what they were."""
    from fluidframework_amd.engine import Engine

    rnd = random.Random(5)
    it = Interner()
    log, n = _edge_doc(it, 65, rnd, n_refs=16)
    caps = dict(CAPS, ref_slots=16)
    pristine = copy.deepcopy(log)
    eng = Engine(1, **caps)
    eng.apply(build_batch([log], it))
    assert eng.status(0)[0] == 0
    eng.summarize()

    def state():
        return eng.hashes().copy(), [x.copy() for x in eng.deltas_batch([0])], eng.ref_keys(0), eng.launch_counts()

    before = state()
    f = _Fleet()
    f.eng, f.keys, f.sets, f.refs = eng, [before[2]], [(0, 0, 8)], [(2 * k, 2 * k + 1) for k in range(8)]
    f.qs = [(0, 4, 90, OVERLAP), (0, 30, 30, PREVIOUS), (0, 30, 30, NEXT), (0, 0, n, OVERLAP)]
    f.t = _transient_keys([pristine], it, {(0, p) for p in (4, 90, 30, 0, n)}, **dict(caps, ref_slots=64))
    rows, _, _ = _compare(f, f.qs)
    assert len(rows) > 0
    after = state()
    assert np.array_equal(before[0], after[0]) and before[2] == after[2] and before[3] == after[3]
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    eng.close()
    full = copy.deepcopy(pristine)  # the Transient path on the same table: no slot for the query's references
    full.create_ref(4, TRANSIENT)
    eng = Engine(1, **caps)
    eng.apply(build_batch([full], it))
    assert eng.status(0)[0] == abi.MTR_ERR_CAPACITY
    eng.close()
