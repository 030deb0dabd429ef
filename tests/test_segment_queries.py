"""mtr_get_containing_segments: many getContainingSegment views in one launch, with the segments' text and properties.

The batched call is defined by the calls that exist, so every check here is word for word against a loop of
mtr_get_containing_segment plus mtr_get_props on the same engine state: the 14 info words, the text units the single
call writes into a large enough buffer (found by calling it on two buffers filled with different patterns: a unit it
wrote is the same in both), and the property words.  One fleet is also checked against the oracle's nodeMap
(OracleDoc.containing / length, as test_gpu_scale.test_containing_segment_matches_oracle does).

The fleet (one engine, one batch): 8 SharedString documents of 300 synthetic messages whose one-unit inserts were
turned into Tile markers (a marker is one unit long, so every recorded position stays valid), and one document that
is HBM-resident with hole slots: holes start at kGapMin = 8,192 leaves, so it is test_launch_invariance's "gap-min"
crossing document, the smallest recipe of the suite that reaches them (grown past 8,192 leaves, then scoured by
removals).  A query past those removals runs Eng::containing's count_live branch.
"""
import ctypes as C
import random

import numpy as np
import pytest

from fluidframework_amd import abi
from fluidframework_amd.synth import make_cfg, with_docs
from oracle.oracle import OracleDoc, generate, options

pytestmark = pytest.mark.gpu

INT32_MAX = 0x7fffffff
INFO_WORDS = 14  # mtr_segment_info
WRITERS = 8
NON_WRITER = 13  # a short client id no document's log holds
N_SMALL = 8
HOLED = N_SMALL  # the holed document's index in the fleet
PATTERN = 0x5a


# ---------------------------------------------------------------- the raw calls
def _lib():
    from fluidframework_amd.engine import lib
    return lib()


def _err():
    return _lib().mtr_last_error().decode()


def _queries(qs):
    q = np.zeros(max(len(qs), 1), dtype=abi.VIEW_QUERY_DTYPE)
    for i, x in enumerate(qs):
        q[i] = x
    return q


class _Out:
    """The caller's buffers of one mtr_get_containing_segments call, pre-filled with a pattern."""

    def __init__(self, n, text_units, prop_words):
        self.info = np.full((max(n, 1), INFO_WORDS), PATTERN, dtype="<i4")
        self.text = np.full(max(text_units, 1), PATTERN, dtype="<u2")
        self.props = np.full(max(prop_words, 1), PATTERN, dtype="<u4")
        self.toff = np.full(n + 1, PATTERN, dtype="<i8")
        self.poff = np.full(n + 1, PATTERN, dtype="<i8")

    def untouched(self):
        return all((a == PATTERN).all() for a in (self.info, self.text, self.props, self.toff, self.poff))


def _call(eng, qs, out, text=True, props=True, toff=True, poff=True, text_cap=None, props_cap=None):
    q = _queries(qs)
    return int(_lib().mtr_get_containing_segments(
        eng.h, q.ctypes.data, len(qs), out.info.ctypes.data,
        out.text.ctypes.data if text else None, out.text.size if text_cap is None else text_cap,
        out.toff.ctypes.data if toff else None,
        out.props.ctypes.data if props else None, out.props.size if props_cap is None else props_cap,
        out.poff.ctypes.data if poff else None))


def _batched(eng, qs):
    """The size query, then the fetch -> (info [n][14], per query its text units, per query its property words)."""
    n = len(qs)
    size = _Out(n, 0, 0)
    assert _call(eng, qs, size, text=False, props=False) == n, _err()
    assert (size.text == PATTERN).all() and (size.props == PATTERN).all()  # (a size query writes no units or words)
    out = _Out(n, int(size.toff[n]), int(size.poff[n]))
    assert _call(eng, qs, out, text_cap=int(size.toff[n]), props_cap=int(size.poff[n])) == n, _err()
    assert np.array_equal(out.toff, size.toff) and np.array_equal(out.poff, size.poff)
    assert np.array_equal(out.info[:n], size.info[:n])
    assert out.toff[0] == 0 and out.poff[0] == 0 and (np.diff(out.toff) >= 0).all() and (np.diff(out.poff) >= 0).all()
    return (out.info[:n], [out.text[out.toff[i]:out.toff[i + 1]] for i in range(n)],
            [out.props[out.poff[i]:out.poff[i + 1]] for i in range(n)])


class _Reference:
    """The loop of single calls, one query at a time, each distinct query asked once."""

    def __init__(self, eng, text_cap=1 << 15, matrix_docs=()):
        # (matrix_docs: the documents that are matrix vectors.  Their info.props is a tracking id, which
        # mtr_get_props cannot be asked about: include/mtr.h gives them no property words)
        self.eng, self.cap, self.memo, self.matrix_docs = eng, text_cap, {}, set(matrix_docs)

    def __call__(self, query):
        if query not in self.memo:
            self.memo[query] = self._ask(*query)
        return self.memo[query]

    def _ask(self, doc, pos, ref, client):
        from fluidframework_amd.engine import SegmentInfo

        info, bufs = SegmentInfo(), []
        for fill in (0x0000, 0xffff):
            t = np.full(self.cap, fill, dtype="<u2")
            rc = _lib().mtr_get_containing_segment(self.eng.h, doc, pos, ref, client, C.byref(info), t.ctypes.data, t.size)
            assert rc == 0, _err()
            bufs.append(t)
        same = bufs[0] == bufs[1]
        units = int(same.sum())
        assert same[:units].all() and units < self.cap  # (what it wrote is a prefix, and the buffer was large enough)
        words = np.zeros(0, dtype="<u4")
        if info.leaf >= 0 and info.props != -1 and doc not in self.matrix_docs:
            one = np.zeros(1, dtype="<u4")
            need = int(_lib().mtr_get_props(self.eng.h, doc, info.props, one.ctypes.data, 1))
            assert need != -1, _err()
            words = np.zeros(abs(need), dtype="<u4")
            assert _lib().mtr_get_props(self.eng.h, doc, info.props, words.ctypes.data, words.size) == words.size
        row = np.frombuffer(bytes(info), dtype="<i4").copy()
        assert row.size == INFO_WORDS
        return row, bufs[0][:units].copy(), words


def _compare(eng, ref, qs):
    """mtr_get_containing_segments(qs) against the reference loop; returns what the batched call gave."""
    info, text, props = _batched(eng, qs)
    for i, query in enumerate(qs):
        row, units, words = ref(query)
        assert np.array_equal(info[i], row), f"query {i} {query}: info {info[i].tolist()} != {row.tolist()}"
        assert np.array_equal(text[i], units), f"query {i} {query}: text units differ"
        assert np.array_equal(props[i], words), f"query {i} {query}: property words {props[i].tolist()} != {words.tolist()}"
    return info, text, props


def _views_and_positions(eng, doc, refs, clients):
    """The positions the issue names, at every (ref, client) view of a document: -1, 0, a mid-segment offset, the last
    position, the view length and INT32_MAX."""
    out = []
    for ref in refs:
        for client in clients:
            L = eng.view_length(doc, ref, client)
            mid = L // 2
            for p in range(L // 2, min(L, L // 2 + 8)):  # (a position inside a segment, not at its start)
                got = eng.containing_segment(doc, p, ref, client)
                if got is not None and got["offset"] > 0:
                    mid = p
                    break
            out += [(doc, p, ref, client) for p in (-1, 0, mid, L - 1, L, INT32_MAX)]
    return out


def _interleave(per_doc):
    """Round-robin over the documents' query lists: neighbours in the batch name different documents."""
    out = []
    for k in range(max(len(x) for x in per_doc)):
        out += [x[k] for x in per_doc if k < len(x)]
    return out


# ---------------------------------------------------------------- the fleet
class _Fleet:
    pass


@pytest.fixture(scope="module")
def fleet():
    from test_launch_invariance import _caps_for_leaves, _concat, _engine, _tabs, crossing_recipe

    cfg = make_cfg(N_SMALL, 300, writers=WRITERS, max_lag=32, weights=(50, 30, 20), seed=0x5e6)
    small, _, st = generate(cfg, _tabs(), 0, N_SMALL, threads=8, opts=options())
    assert (st == 0).all()
    ops = small.ops.copy()
    one_unit = np.nonzero((ops["type"] == abi.OP_INSERT) & (ops["payload2"] == 1) & (ops["flags"] & abi.F_PROPS == 0))[0]
    assert len(one_unit) >= 2 * N_SMALL
    ops["flags"][one_unit] |= abi.F_MARKER
    ops["payload"][one_unit] = abi.REFTYPE_TILE
    ops["payload2"][one_unit] = 0
    small = with_docs(_tabs(), small.docs.copy(), ops, small.text)
    big, _ = crossing_recipe("gap-min")
    big = with_docs(_tabs(), big.docs[:1].copy(), big.ops, big.text)
    b = _concat([small, big])
    n = len(b.docs)
    f = _Fleet()
    f.b, f.n = b, n
    f.eng = _engine(n, **_caps_for_leaves(8192 + 1024, int(b.docs["text_count"].max())))
    f.eng.apply(b)
    for d in range(n):
        assert f.eng.status(d)[0] == 0
    # the holed document ran HBM-resident (mtr_debug_launch_counts out[19]) and holds more slots than leaves
    counts = f.eng.launch_counts()
    assert counts["global_mode"] > 0, counts
    assert f.eng.stats()["max_leaves"] > len(f.eng.export(HOLED)[0])
    f.orcs = []
    for d in range(n):
        o = OracleDoc(options())
        assert o.apply(b, d) == 0
        f.orcs.append(o)
    f.ref = _Reference(f.eng)
    per_doc = []
    for d in range(n):
        st = f.orcs[d].state()
        low, cur = int(st[0]), int(st[1])  # (the MSN and the current sequence number)
        per_doc.append(_views_and_positions(f.eng, d, (0, cur // 2, low, cur), (1 + d % WRITERS, NON_WRITER, -1, -2)))
    f.queries = list(dict.fromkeys(_interleave(per_doc)))  # (each distinct query once)
    assert len(f.queries) >= 500
    yield f
    f.eng.close()


def test_mixed_fleet_equals_single_calls_and_oracle(fleet):
    """Every query of the fleet in one batch (interleaved across the 8 small documents and the holed HBM one): info,
    text and props equal the single calls'; where the view is one the oracle answers (a writer at a reference sequence
    number inside the collaboration window, a position in [0, length]) leaf, offset, length and start equal its
    nodeMap."""
    qs = fleet.queries
    info, text, props = _compare(fleet.eng, fleet.ref, qs)
    kinds = {"none": 0, "marker": 0, "text": 0, "props": 0, "removed": 0, "holed": 0}
    checked = 0
    for i, (doc, pos, ref, client) in enumerate(qs):
        leaf, marker = int(info[i][0]), int(info[i][6])
        kinds["none"] += leaf < 0
        kinds["marker"] += leaf >= 0 and marker == 1
        kinds["text"] += len(text[i]) > 0
        kinds["props"] += len(props[i]) > 1
        kinds["removed"] += leaf >= 0 and int(info[i][10]) == 1
        kinds["holed"] += doc == HOLED and leaf > 0
        if leaf >= 0 and marker:
            assert len(text[i]) == 0
        if leaf >= 0 and not marker:
            assert len(text[i]) == int(info[i][2])
        o = fleet.orcs[doc]
        st = o.state()
        if not (1 <= client <= WRITERS and int(st[0]) <= ref <= int(st[1])):
            continue
        L = o.length(ref, client)
        if pos == INT32_MAX:
            assert leaf < 0 and int(info[i][9]) == L, (doc, ref, client)
            checked += 1
        elif 0 <= pos <= L:
            exp = o.containing(pos, ref, client)
            if exp[0] < 0:
                assert leaf < 0, (doc, pos, ref, client)
            else:
                got = (leaf, int(info[i][1]), int(info[i][2]), int(info[i][9]))
                assert got == exp, (doc, pos, ref, client)
            checked += 1
    print(f"{len(qs)} queries: {kinds}; {checked} checked against the oracle")
    assert checked >= 60
    assert all(v > 0 for v in kinds.values()), kinds


def test_holed_document_past_its_removals(fleet):
    """The holed HBM document: the leaf ordinal of a query near the end of the view counts the live slots before it
    (Eng::containing's count_live), so it equals the oracle's, and is below the slot the leaf sits in."""
    o = fleet.orcs[HOLED]
    cur = int(o.state()[1])
    L = o.length(cur, 1)
    qs = _interleave([[(HOLED, p, cur, 1) for p in (L - 1, L - 2, (3 * L) // 4, L // 2, L)],
                      [(d, 1, cur, 1) for d in range(4)]])
    info, _, _ = _compare(fleet.eng, fleet.ref, qs)
    slots = fleet.eng.stats()["max_leaves"]
    leaves = len(fleet.eng.export(HOLED)[0])
    assert slots > leaves
    for i, (doc, pos, ref, client) in enumerate(qs):
        if doc == HOLED and pos < L:
            exp = o.containing(pos, ref, client)
            assert (int(info[i][0]), int(info[i][1]), int(info[i][2]), int(info[i][9])) == exp
            assert 0 < int(info[i][0]) < leaves


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_query_counts(fleet, n):
    """A grid of one workgroup, a wave-sized count, one past it, and 1,000 queries in which every query appears twice."""
    if n == 1000:
        qs = fleet.queries[:500] * 2
        random.Random(n).shuffle(qs)
        assert len(set(qs)) == 500
    else:
        qs = fleet.queries[:n]
    assert len(qs) == n
    _compare(fleet.eng, fleet.ref, qs)


def test_no_queries(fleet):
    out = _Out(0, 0, 0)
    assert _call(fleet.eng, [], out) == 0
    assert out.toff[0] == 0 and out.poff[0] == 0
    assert (out.info == PATTERN).all() and (out.text == PATTERN).all() and (out.props == PATTERN).all()


def test_caps_size_queries_and_skipped_halves(fleet):
    qs = fleet.queries[:200]
    n = len(qs)
    info, text, props = _compare(fleet.eng, fleet.ref, qs)
    nt, npw = sum(len(x) for x in text), sum(len(x) for x in props)
    assert nt > 1 and npw > 1
    want_toff = np.concatenate([[0], np.cumsum([len(x) for x in text])])
    want_poff = np.concatenate([[0], np.cumsum([len(x) for x in props])])
    # one unit, one word short: MTR_SUMMARY_TOO_SMALL, info and both offset arrays complete, no units or words
    for tc, pc in ((nt - 1, npw), (nt, npw - 1), (nt - 1, npw - 1)):
        out = _Out(n, nt, npw)
        assert _call(fleet.eng, qs, out, text_cap=tc, props_cap=pc) == abi.MTR_SUMMARY_TOO_SMALL
        assert np.array_equal(out.info[:n], info)
        assert np.array_equal(out.toff, want_toff) and np.array_equal(out.poff, want_poff)
        assert (out.text == PATTERN).all() and (out.props == PATTERN).all()
    # NULL text: that half is a size query, the other is fetched; and the other way round
    out = _Out(n, nt, npw)
    assert _call(fleet.eng, qs, out, text=False) == n
    assert np.array_equal(out.toff, want_toff) and (out.text == PATTERN).all()
    assert np.array_equal(out.props[:npw], np.concatenate(props))
    out = _Out(n, nt, npw)
    assert _call(fleet.eng, qs, out, props=False) == n
    assert np.array_equal(out.poff, want_poff) and (out.props == PATTERN).all()
    assert np.array_equal(out.text[:nt], np.concatenate(text))
    # a NULL offsets pointer skips its half entirely, whatever its buffer and cap are
    out = _Out(n, nt, npw)
    assert _call(fleet.eng, qs, out, toff=False, text_cap=0) == n
    assert (out.toff == PATTERN).all() and (out.text == PATTERN).all()
    assert np.array_equal(out.poff, want_poff) and np.array_equal(out.props[:npw], np.concatenate(props))
    out = _Out(n, nt, npw)
    assert _call(fleet.eng, qs, out, poff=False, props_cap=0) == n
    assert (out.poff == PATTERN).all() and (out.props == PATTERN).all()
    assert np.array_equal(out.toff, want_toff) and np.array_equal(out.text[:nt], np.concatenate(text))
    out = _Out(n, nt, npw)
    assert _call(fleet.eng, qs, out, toff=False, poff=False) == n
    assert np.array_equal(out.info[:n], info) and (out.text == PATTERN).all() and (out.props == PATTERN).all()


@pytest.mark.parametrize("where", ["first", "last"])
def test_bad_document_is_refused_with_its_index(fleet, where):
    """doc = max_docs (the single call's bound) at index 0 and at index n - 1: -1, the message names the index, and
    nothing is written."""
    qs = list(fleet.queries[:40])
    k = 0 if where == "first" else len(qs) - 1
    qs[k] = (fleet.n, 0, 0, 1)
    from fluidframework_amd.engine import SegmentInfo

    info = SegmentInfo()
    assert _lib().mtr_get_containing_segment(fleet.eng.h, fleet.n, 0, 0, 1, C.byref(info), None, 0) == -1
    assert _lib().mtr_get_containing_segment(fleet.eng.h, fleet.n - 1, 0, 0, 1, C.byref(info), None, 0) == 0
    out = _Out(len(qs), 1 << 16, 1 << 16)
    assert _call(fleet.eng, qs, out) == -1
    assert f"query {k}" in _err(), _err()
    assert out.untouched()


def test_python_binding(fleet):
    """Engine.containing_segments / view_lengths: containing_segment's and view_length's results, plus the decoded
    properties."""
    qs = fleet.queries[:150]
    got = fleet.eng.containing_segments(qs)
    assert len(got) == len(qs)
    n_props = 0
    for query, g in zip(qs, got):
        want = fleet.eng.containing_segment(*query)
        if want is None:
            assert g is None
            continue
        assert {k: v for k, v in g.items() if k != "properties"} == want, query
        assert g["properties"] == (None if want["props"] == -1 else fleet.eng.props(query[0], want["props"])), query
        n_props += bool(g["properties"])
    assert n_props > 0
    views = sorted({(d, r, c) for d, _, r, c in qs})
    assert fleet.eng.view_lengths(views) == [fleet.eng.view_length(*v) for v in views]
    assert fleet.eng.containing_segments([]) == [] and fleet.eng.view_lengths([]) == []


def test_read_only(fleet):
    """The call only reads document state: the counters, the launch census, the kept summary's hashes and the blob
    cache are what they were."""
    eng = fleet.eng
    eng.summarize()
    eng.blob_cache_add_summary()

    def state():
        return eng.stats(), eng.launch_counts(), eng.hashes(fleet.n).copy(), eng.blob_cache_size(), eng.summary(0)

    before = state()
    _batched(eng, fleet.queries[:300])
    after = state()
    assert before[0] == after[0] and before[1] == after[1] and np.array_equal(before[2], after[2])
    assert before[3] == after[3] > 0 and before[4] == after[4]


# ---------------------------------------------------------------- other kinds of state
def test_matrix_vectors():
    """A SharedMatrix pair (mtr_set_matrix through the record-mode generator): the vectors' segments carry no text in
    either call; everything else equals the single calls, in one batch."""
    from fluidframework_amd.engine import Engine
    from fluidframework_amd.synth import tables

    ops = 300
    cfg = make_cfg(1, ops, writers=WRITERS, max_lag=16, weights=(12, 8, 80), max_text=4, max_range=3)
    eng = Engine(2, max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=1 << 15, prop_words=1024,
                 remover_cells=4096, ops_per_launch=64)
    try:
        eng.generate_matrix(cfg, tables(writers=WRITERS))  # matrix 0 = documents (0 rows, 1 cols)
        assert [eng.status(d)[0] for d in (0, 1)] == [0, 0]
        per_doc = [_views_and_positions(eng, d, (0, ops // 2, ops), (1, NON_WRITER, -1, -2)) for d in (0, 1)]
        qs = _interleave(per_doc)
        info, text, props = _compare(eng, _Reference(eng, matrix_docs=(0, 1)), qs)
        assert sum(int(r[0]) >= 0 for r in info) > 10
        assert all(len(t) == 0 for t in text) and all(len(w) == 0 for w in props)
    finally:
        eng.close()


def test_tracked_matrix_vectors():
    """Matrix vectors whose segments carry tracking ids (an undo farm, built as test_matrix_undo builds them, in a
    72-word property arena): info.props is then the tracking id, as the single call reports it, and the arena word
    there is a group bit set, not a count.  The batched call gives such segments no property words and fails no
    query over them, with the properties half asked for or skipped."""
    from test_matrix_undo import farm

    pcap = 72
    s = farm(0, engine=True, rounds=30, prop_words=pcap)
    eng = s.eng
    try:
        docs = range(2 * len(s.clients))
        tracked = {d: {int(x[3]): int(x[4]) & 0xffffffff for x in eng.leaves(d) if int(x[3]) >= 0} for d in docs}
        # (ids whose bit set, read as a property count, would reach past the arena)
        past = {(d, t) for d in docs for t, bits in tracked[d].items() if t + 1 + 2 * bits > pcap}
        assert past, tracked
        per_doc = []
        for d in docs:
            L = eng.view_length(d, s.seq, -1)
            per_doc.append([(d, p, s.seq, -1) for p in list(range(L + 1)) + [INT32_MAX]])
        qs = _interleave(per_doc)
        info, text, props = _compare(eng, _Reference(eng, matrix_docs=docs), qs)
        assert all(len(t) == 0 for t in text) and all(len(w) == 0 for w in props)
        seen = {(q[0], int(r[8])) for q, r in zip(qs, info) if int(r[0]) >= 0 and int(r[8]) >= 0}
        assert seen & past, (seen, past)
        out = _Out(len(qs), 1, 1)
        assert _call(eng, qs, out, poff=False) == len(qs), _err()
        assert np.array_equal(out.info[:len(qs)], info)
        got = eng.containing_segments(qs)
        assert [g is not None for g in got] == [int(r[0]) >= 0 for r in info]
        assert all(g["properties"] is None and g["props"] == int(r[8]) for g, r in zip(got, info) if g is not None)
    finally:
        eng.close()


def test_pending_local_segments():
    """Writers holding pending local inserts and removes mid-group (built as test_local_ops does): local_seq,
    local_removed_seq and groups come out of the LOCAL_BASE decoding both calls share."""
    from fixtures import Perspective, load_replay, original_summary, replay_files, replay_writers
    from fluidframework_amd.batch import Interner, build_batch
    from fluidframework_amd.engine import Engine

    it = Interner()
    views = []
    for p in [p for p in replay_files() if "clients_4" in p][:3]:
        groups = load_replay(p)
        summary = original_summary(groups)
        k = next(i for i, g in enumerate(groups) if len(g["msgs"]) >= 32)  # (the early groups hold one message)
        for w in replay_writers(groups):
            v = Perspective(w, summary, it)
            for g in groups[:k]:
                v.feed(g, it)
            v.feed(groups[k], it, 0, len(groups[k]["msgs"]) // 2, drain=False)  # (its own ops of this half pend)
            views.append((groups, v))
    b = build_batch([v.log for _, v in views], it)
    eng = Engine(len(views), max_segments=8192, heap_entries=8192, text_units=1 << 18, prop_words=1 << 18,
                 remover_cells=1 << 14, ops_per_launch=64)
    try:
        eng.apply(b)
        per_doc = []
        for d in range(len(views)):
            assert eng.status(d)[0] == 0
            L = eng.view_length(d, INT32_MAX, -1)
            cur = max(int(x) for x in b.ops["seq"][int(b.docs["op_begin"][d]):][:int(b.docs["op_count"][d])])
            per_doc.append([(d, p, ref, c) for ref in (cur, INT32_MAX) for c in (-1, 1, NON_WRITER)
                            for p in list(range(0, L, max(1, L // 80))) + [L, INT32_MAX]])
        qs = _interleave(per_doc)
        info, _, _ = _compare(eng, _Reference(eng), qs)
        live = info[info[:, 0] >= 0]
        # (mtr_segment_info: [11] local_seq, [12] local_removed_seq, [13] groups)
        print(f"{len(qs)} queries: {int((live[:, 11] >= 0).sum())} pending inserts, "
              f"{int((live[:, 12] >= 0).sum())} pending removes, {int((live[:, 13] > 0).sum())} in a segment group")
        assert (live[:, 11] >= 0).any() and (live[:, 12] >= 0).any() and (live[:, 13] > 0).any()
    finally:
        eng.close()


def test_buffers_are_released_with_the_engine():
    """The work buffers are the engine's own: mtr_debug_live_bytes grows with a batched call and is back to its prior
    value after mtr_engine_destroy."""
    from fluidframework_amd.engine import Engine, live_bytes
    from fluidframework_amd.synth import tables

    before = live_bytes()
    eng = Engine(4, max_segments=1024, heap_entries=1024, text_units=1 << 14, prop_words=1 << 14, remover_cells=1 << 12)
    cfg = make_cfg(4, 100, writers=WRITERS, max_lag=16)
    eng.generate(cfg, tables(writers=WRITERS))
    idle = live_bytes()
    got = eng.containing_segments([(d, p, 100, 1) for d in range(4) for p in range(0, 40, 3)])
    assert any(g is not None and g["text"] for g in got)
    assert live_bytes() > idle
    eng.close()
    assert live_bytes() == before
