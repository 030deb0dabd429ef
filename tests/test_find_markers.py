"""mtr_find_markers: SharedString.findTile and getMarkerFromId + getPosition for many (document, view) pairs in one call.

The call is defined by the calls that exist (include/mtr.h).  With R(doc, rs, cl) the rows of the range [0, INT32_MAX)
at a view and W(doc, ref) the pairs mtr_get_props returns: a row matches a label when it is a marker and the label's key
is MTR_LABEL_ANY or W(doc, row.props) holds (key, v) with v among the label's values; PRECEDING is the matching row with
the greatest start <= pos, FOLLOWING the one with the least start >= pos.  That composition is written here once
(compose), over Engine.range_segments and Engine.props on the same engine state, and every check compares all six output
words of every query with it, exactly.  BY_ID is compared with mtr_transform_positions' MTR_POS_FROM_LEAF for the leaf the
test knows the marker to be, and with the fields mtr_get_containing_segments reports for it.  The batch is never compared
with itself.

Documents: test_segment_queries' fleet (8 oracle-generated SharedStrings with Tile markers and the hole-layout HBM
document; its recipe gives the markers no referenceTileLabels -- the one-unit inserts it turns into markers are those
without properties, and later annotates put other keys on some -- so its legs run with MTR_LABEL_ANY and with every
(key, value) pair its markers do carry, taken as a label), hand-made documents of exactly 63, 64, 65 and 130 leaves with a
marker every 7th leaf whose labels cycle through ["Eop"], ["pg"], ["Eop","pg"] and none and whose ids are "m<leaf>"
(two whole leaves removed late, one of them a marker, so that an older view still shows them), a document whose removed
marker zamboni took away, and a matrix vector pair.
"""
import os
import random
import re

import numpy as np
import pytest

from fluidframework_amd import abi
from fluidframework_amd.batch import DocLog, Interner, build_batch

gpu = pytest.mark.gpu

INT32_MAX = 0x7fffffff
PATTERN = 0x5a5a5a5a
NON_WRITER = 13  # a short client id no document's log holds (test_segment_queries.NON_WRITER)
EDGE_LEAVES = (63, 64, 65, 130)
PREC, FOLL, BY_ID = abi.MK_PRECEDING, abi.MK_FOLLOWING, abi.MK_BY_ID
FOUND, VISIBLE, ANY = abi.MK_FOUND, abi.MK_VISIBLE, abi.LABEL_ANY
NONE = (-1, -1, 0, -1, 0, 0)
TILE_LABELS = ["Eop"], ["pg"], ["Eop", "pg"], None  # the labels of the hand-made documents' markers, in turn
REMOVED = (8, 9)  # the leaves the hand-made documents remove late; leaf 8 is a marker


# ---------------------------------------------------------------- the reference: the composition of include/mtr.h
def compose(rows, words, labels, vals, pos, mode, label):
    """The six output words of one PRECEDING / FOLLOWING query, by the contract.  rows: the view's R, dicts with start,
    leaf, marker, ref_type, props, seq, in order; words(ref) -> [(key id, value id)] of mtr_get_props; labels: [(key,
    first, count)]; vals: the value ids."""
    key, first, count = labels[label]
    allowed = set(vals[first:first + count])

    def matches(r):
        if r["marker"] != 1:
            return False
        if key == ANY:
            return True
        return r["props"] != -1 and any(k == key and v in allowed for k, v in words(r["props"]))

    hits = [r for r in rows if matches(r) and (r["start"] <= pos if mode == PREC else r["start"] >= pos)]
    if not hits:
        return NONE
    r = max(hits, key=lambda r: r["start"]) if mode == PREC else min(hits, key=lambda r: r["start"])
    return (r["start"], r["leaf"], r["ref_type"], r["props"], r["seq"], FOUND | VISIBLE)


def test_composition_on_a_hand_computed_example():
    """The yardstick itself, on a document worked out by hand.  Eight leaves; keys: 7 = referenceTileLabels, 8 = another
    key; values: 20 = ["Eop"], 21 = ["Eop","pg"], 22 = ["pg"], 23 = "Eop" (a string, under key 8).
      leaf  0 text(3)   1 marker {7: 20}   2 text(2)   3 marker {7: 21}   4 marker {7: 22} -- hidden in this view
      leaf  5 text(4)   6 marker, no set   7 marker {8: 23}
    The view shows every leaf but 4: starts 0, 3, 4, 6, (4 hidden), 7, 11, 12; length 13."""
    sets = {100: [(7, 20)], 110: [(7, 21)], 120: [(7, 22)], 130: [(8, 23)]}
    rows = [dict(start=0, leaf=0, marker=0, ref_type=0, props=-1, seq=1),
            dict(start=3, leaf=1, marker=1, ref_type=1, props=100, seq=2),
            dict(start=4, leaf=2, marker=0, ref_type=0, props=-1, seq=3),
            dict(start=6, leaf=3, marker=1, ref_type=1, props=110, seq=4),
            dict(start=7, leaf=5, marker=0, ref_type=0, props=130, seq=6),  # (a text segment with a set: never a hit)
            dict(start=11, leaf=6, marker=1, ref_type=1, props=-1, seq=7),
            dict(start=12, leaf=7, marker=1, ref_type=2, props=130, seq=8)]
    labels = [(7, 0, 2), (7, 1, 2), (ANY, 0, 0), (7, 3, 0), (8, 0, 2), (8, 3, 1)]  # Eop, pg, any, empty, wrong key, 23
    vals = [20, 21, 22, 23]
    q = lambda pos, mode, label: compose(rows, sets.__getitem__, labels, vals, pos, mode, label)  # noqa: E731
    hit = lambda r: (r["start"], r["leaf"], r["ref_type"], r["props"], r["seq"], FOUND | VISIBLE)  # noqa: E731
    m1, m3, m6, m7 = rows[1], rows[3], rows[5], rows[6]
    # "Eop": leaves 1 and 3
    assert q(2, PREC, 0) == NONE and q(3, PREC, 0) == hit(m1) and q(5, PREC, 0) == hit(m1) and q(6, PREC, 0) == hit(m3)
    assert q(INT32_MAX, PREC, 0) == hit(m3) and q(-1, PREC, 0) == NONE
    assert q(-1, FOLL, 0) == hit(m1) and q(3, FOLL, 0) == hit(m1) and q(4, FOLL, 0) == hit(m3) and q(7, FOLL, 0) == NONE
    # "pg": leaf 3 alone -- leaf 4 carries it too, but the view hides it
    assert q(INT32_MAX, PREC, 1) == hit(m3) and q(0, FOLL, 1) == hit(m3) and q(7, FOLL, 1) == NONE and q(5, PREC, 1) == NONE
    # any marker: the unlabelled ones too
    assert q(11, PREC, 2) == hit(m6) and q(10, PREC, 2) == hit(m3) and q(12, FOLL, 2) == hit(m7) and q(13, FOLL, 2) == NONE
    # no values; a key whose values are others; a string value that is the label's text under another key
    assert q(INT32_MAX, PREC, 3) == NONE and q(0, FOLL, 4) == NONE and q(0, FOLL, 5) == hit(m7)
    # with leaf 4 shown (at 7, the rest one unit later), "pg" finds it
    shown = rows[:4] + [dict(start=7, leaf=4, marker=1, ref_type=1, props=120, seq=5)] + \
        [dict(r, start=r["start"] + 1) for r in rows[4:]]
    assert compose(shown, sets.__getitem__, labels, vals, 7, FOLL, 1)[:2] == (7, 4)
    assert compose(shown, sets.__getitem__, labels, vals, INT32_MAX, PREC, 1)[:2] == (7, 4)


def test_abi_mirror_matches_the_header():
    """abi.py's three dtypes and the macros against include/mtr.h (parsed from the header's own struct bodies)."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "include", "mtr.h")).read()
    for name, dtype, size in (("mtr_marker_label", abi.MARKER_LABEL_DTYPE, 12),
                              ("mtr_marker_query", abi.MARKER_QUERY_DTYPE, 24),
                              ("mtr_marker_hit", abi.MARKER_HIT_DTYPE, 24)):
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
    for macro, value in (("MTR_MK_PRECEDING", PREC), ("MTR_MK_FOLLOWING", FOLL), ("MTR_MK_BY_ID", BY_ID),
                         ("MTR_MK_FOUND", FOUND), ("MTR_MK_VISIBLE", VISIBLE)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, src).group(1)) == value
    assert int(re.search(r"#define MTR_LABEL_ANY\s+(0x[0-9a-f]+)u", src).group(1), 16) == ANY
    assert "mtr_find_markers" in abi.MARKER_QUERY_SIGNATURES and len(abi.MARKER_QUERY_SIGNATURES["mtr_find_markers"][1]) == 8


def test_interner_label_values():
    it = Interner()
    assert it.label_values("referenceTileLabels", "pg") == (None, []) and it.keys == {}  # (an unknown key creates nothing)
    it.propop({"referenceTileLabels": ["pg"], "other": "pg"})
    it.propop({"referenceTileLabels": ["pg2"]})
    it.propop({"referenceTileLabels": ["Eop", "pg"]})
    it.propop({"referenceTileLabels": "[\"pg\"]"})  # (a string holding the label's text: no array)
    it.propop({"referenceTileLabels": {"pg": ["x"]}})
    n_keys, n_vals = len(it.keys), len(it.val_bytes)
    key, ids = it.label_values("referenceTileLabels", "pg")
    assert key == it.keys["referenceTileLabels"]
    assert ids == sorted(ids) == [it.value(["pg"]), it.value(["Eop", "pg"])]
    assert it.label_values("referenceTileLabels", "pg2")[1] == [it.value(["pg2"])]
    assert it.label_values("referenceTileLabels", "p")[1] == [] and it.label_values("referenceTileLabels", "x")[1] == []
    assert it.label_values("missing", "pg") == (None, [])
    assert (len(it.keys), len(it.val_bytes)) == (n_keys, n_vals)  # (the tables are read, never written)
    it.propop({"referenceTileLabels": ["a", "pg", "b"]})  # (the value table grew after the first call)
    assert it.label_values("referenceTileLabels", "pg")[1] == ids + [it.value(["a", "pg", "b"])]
    assert it.label_values("other", "pg") == (it.keys["other"], ids + [it.value(["a", "pg", "b"])])  # (any key)


# ---------------------------------------------------------------- the raw call and the reference on an engine
def _lib():
    from fluidframework_amd.engine import lib
    return lib()


def _err():
    return _lib().mtr_last_error().decode()


def raw(eng, labels, vals, qs, n=None):
    """mtr_find_markers into a patterned buffer -> (return value, the rows [len(qs), 6])."""
    lb = np.zeros(max(len(labels), 1), dtype=abi.MARKER_LABEL_DTYPE)
    for i, x in enumerate(labels):
        lb[i] = tuple(x)
    v = np.array(list(vals) + [0], dtype="<u4")
    q = np.zeros(max(len(qs), 1), dtype=abi.MARKER_QUERY_DTYPE)
    for i, x in enumerate(qs):
        q[i] = tuple(x)
    out = np.full((max(len(qs), 1), 6), PATTERN, dtype="<i4")
    rc = int(_lib().mtr_find_markers(eng.h, lb.ctypes.data, len(labels), v.ctypes.data, len(vals), q.ctypes.data,
                                     len(qs) if n is None else n, out.ctypes.data))
    return rc, out


class Reference:
    """compose over one engine's range rows and property sets; each view's rows and each set asked once."""

    def __init__(self, eng):
        self.eng, self.r, self.w = eng, {}, {}

    def rows(self, doc, rs, cl):
        key = (doc, rs, cl)
        if key not in self.r:
            self.r[key] = self.eng.range_segments([(doc, 0, None, rs, cl)])[0]
            starts = [s["start"] for s in self.r[key]]
            assert starts == sorted(starts)
        return self.r[key]

    def words(self, doc):
        def get(ref):
            if (doc, ref) not in self.w:
                self.w[(doc, ref)] = self.eng.props(doc, ref)
            return self.w[(doc, ref)]
        return get

    def length(self, doc, rs, cl):
        r = self.rows(doc, rs, cl)
        return r[-1]["start"] + r[-1]["length"] if r else 0

    def __call__(self, labels, vals, query):
        doc, pos, rs, cl, mode, label = query
        return compose(self.rows(doc, rs, cl), self.words(doc), labels, vals, pos, mode, label)


def compare(eng, ref, labels, vals, qs):
    """The batched call against the composition, all six words of every query -> the rows as tuples."""
    rc, out = raw(eng, labels, vals, qs)
    assert rc == len(qs), _err()
    got = [tuple(int(x) for x in r) for r in out[:len(qs)]]
    for i, (q, g) in enumerate(zip(qs, got)):
        want = ref(labels, vals, q)
        assert g == want, f"query {i} {q}: {g} != {want}"
    return got


# ---------------------------------------------------------------- hand-made documents with exact leaf counts
def _msg(client, op, seq, ref, msn=0):
    return {"clientId": client, "sequenceNumber": seq, "referenceSequenceNumber": ref, "minimumSequenceNumber": msn,
            "type": "op", "contents": op}


def is_marker(j):
    """Every 7th leaf, and leaf 63: the last leaf of round 0 beside leaf 64, the first of round 1."""
    return j % 7 == 1 or j == 63


def marker_props(j):
    labels = TILE_LABELS[(j // 7) % 4]
    props = {"markerId": f"m{j}"}
    if labels is not None:
        props["referenceTileLabels"] = labels
    return props


def edge_log(it, leaves):
    """`leaves` appends by "w" (never merged: the minimum sequence number stays 0): leaf j is a Tile marker with
    marker_props(j) when is_marker(j), else three distinct units; then "v" removes leaves 8 and 9 whole (sequence number
    leaves + 1).  Returns (log, lens): lens[j] = leaf j's length."""
    log = DocLog()
    log.start_collab("me")
    lens, at = [], 0
    for j in range(leaves):
        if is_marker(j):
            seg = {"marker": {"refType": abi.REFTYPE_TILE}, "props": marker_props(j)}
            lens.append(1)
        else:
            seg = {"text": "".join(chr(0x100 + (3 * j + u) % 0x700) for u in range(3))}
            lens.append(3)
        log.message(_msg("w", {"type": 0, "pos1": at, "seg": seg}, j + 1, j), it)
        at += lens[-1]
    a = sum(lens[:REMOVED[0]])
    log.message(_msg("v", {"type": 1, "pos1": a, "pos2": a + sum(lens[j] for j in REMOVED)}, leaves + 1, leaves), it)
    return log, lens


class _Edges:
    pass


@pytest.fixture(scope="module")
def edges():
    from fluidframework_amd.engine import Engine

    it = Interner()
    f = _Edges()
    built = [edge_log(it, n) for n in EDGE_LEAVES]
    f.it, f.logs, f.lens = it, [x[0] for x in built], [x[1] for x in built]
    f.eng = Engine(len(EDGE_LEAVES) + 1, max_segments=1024, heap_entries=1024, text_units=1 << 12, prop_words=1 << 12,
                   remover_cells=1 << 10, ops_per_launch=64)
    f.eng.apply(build_batch(f.logs, it))
    for d in range(len(built)):
        st, op = f.eng.status(d)
        assert st == 0, f"document {d}: status {st:#x} at op {op}"
        assert len(f.eng.export(d)[0]) == EDGE_LEAVES[d]  # (the leaf count is exact: no split, no merge)
    f.ref = Reference(f.eng)
    # the label table of every check: Eop, pg, any marker, a label without values, a key no marker has (with pg's
    # values), markerId as a label key (its values are no arrays: nothing matches), and Eop again sharing its values
    key, eop = it.label_values("referenceTileLabels", "Eop")
    _, pg = it.label_values("referenceTileLabels", "pg")
    assert len(eop) == 2 and len(pg) == 2 and len(set(eop) & set(pg)) == 1  # (["Eop","pg"] carries both)
    f.vals = eop + pg
    f.labels = [(key, 0, 2), (key, 2, 2), (ANY, 0, 0), (key, 1, 0), (it.key("nobody-has-this"), 2, 2),
                (it.keys["markerId"], 0, 2), (key, 0, 2)]
    yield f
    f.eng.close()


def edge_views(n):
    """Views of an edge document of n leaves: the current one (leaves 8 and 9 removed), the one before the removal (all
    n leaves), one that has seen 40 leaves, one that has seen 2, the local view and NonCollabClient."""
    return [(n + 1, NON_WRITER), (n, NON_WRITER), (40, NON_WRITER), (2, NON_WRITER), (INT32_MAX, -1), (n + 1, -2)]


@gpu
@pytest.mark.parametrize("k", range(len(EDGE_LEAVES)))
def test_round_edges(edges, k):
    """Documents of 63, 64, 65 and 130 leaves, every label of the table, both directions, six views.  Positions: one
    unit before, on and one unit after every marker (pos exactly on a marker in both modes; on leaf 8, a marker the
    current view hides), the view's ends and INT32_MAX.  Leaf 63 is a marker (the last leaf of round 0; the last leaf
    of the 64-leaf document) and so is leaf 64 (the first of round 1; the only candidate of the 65-leaf document's
    second round); both carry ["pg"] alone, so an "Eop" search crosses the round boundary between leaves 57 and 71."""
    n, lens = EDGE_LEAVES[k], edges.lens[k]
    pre = np.concatenate([[0], np.cumsum(lens)])  # leaf starts in the view that shows everything
    gap = sum(lens[j] for j in REMOVED)
    qs = []
    for rs, cl in edge_views(n):
        L = edges.ref.length(k, rs, cl)
        ps = {int(pre[j]) + o for j in range(n) if is_marker(j) for o in (-1, 0, 1)}
        ps |= {p - gap for p in ps} | {-1, 0, 1, L - 1, L, L + 1, INT32_MAX}  # (the same leaves where 8 and 9 are hidden)
        for label in range(len(edges.labels)):
            qs += [(k, p, rs, cl, mode, label) for p in sorted(ps) if p <= L + 1 or p == INT32_MAX for mode in (PREC, FOLL)]
    got = compare(edges.eng, edges.ref, edges.labels, edges.vals, qs)
    by_q = dict(zip(qs, got))
    assert any(g == NONE for g in got) and sum(1 for g in got if g[5] == FOUND | VISIBLE) > 200
    assert all(g == NONE for q, g in by_q.items() if q[5] in (3, 4, 5))  # no values, a foreign key, no array values
    assert all(by_q[q] == by_q[q[:5] + (0,)] for q in qs if q[5] == 6)    # (two labels sharing their values)
    cur, old = (n + 1, NON_WRITER), (n, NON_WRITER)
    m8 = int(pre[8])
    # pos on the hidden marker: the old view answers leaf 8 itself, the current one its neighbours (1 and 15)
    assert by_q[(k, m8, *old, PREC, 2)][:2] == (m8, 8) and by_q[(k, m8, *old, FOLL, 2)][:2] == (m8, 8)
    assert by_q[(k, m8, *cur, PREC, 2)][1] == 1 and by_q[(k, m8, *cur, FOLL, 2)][1] == 15
    # leaf 8 carries ["pg"]: the old view finds it by label, the current one finds no "pg" at or before it
    assert by_q[(k, m8, *old, PREC, 1)][1] == 8 and by_q[(k, m8, *cur, PREC, 1)] == NONE
    last = max(j for j in range(n) if is_marker(j))
    assert last == {63: 57, 64: 63, 65: 64, 130: 127}[n]
    assert by_q[(k, INT32_MAX, *old, PREC, 2)][1] == last and by_q[(k, INT32_MAX, *cur, PREC, 2)][1] == last
    if n >= 64:  # the last leaf of round 0, from either side and exactly on it
        p63 = int(pre[63])
        assert by_q[(k, p63, *old, PREC, 2)][1] == 63 and by_q[(k, p63, *old, FOLL, 2)][1] == 63
        assert by_q[(k, p63 - 1, *old, FOLL, 2)][1] == 63 and by_q[(k, p63 - 1, *old, PREC, 2)][1] == 57
    if n >= 65:  # the first leaf of round 1; an answer one round away from pos, in both directions
        p64 = int(pre[64])
        assert by_q[(k, p64, *old, FOLL, 2)][1] == 64 and by_q[(k, p64 + 1, *old, PREC, 2)][1] == 64
        assert by_q[(k, p64 + 1, *old, PREC, 0)][1] == 57          # "Eop" from round 1: the answer lies in round 0
        assert by_q[(k, int(pre[57]) + 1, *old, FOLL, 1)][1] == 63  # "pg" from inside round 0: its last leaf
        assert by_q[(k, p64 - gap, *cur, FOLL, 1)][1] == 64         # (the current view: every prefix 4 units lower)
    if n == 130:
        assert by_q[(k, int(pre[57]) + 1, *old, FOLL, 0)][1] == 71  # "Eop" from round 0: the answer lies in round 1
        assert by_q[(k, int(pre[127]), *old, FOLL, 2)][1] == 127 and by_q[(k, int(pre[127]) + 1, *old, FOLL, 2)] == NONE


@gpu
def test_marker_ids(edges):
    """BY_ID for every marker of the 65- and 130-leaf documents at every view: the position and the visibility
    mtr_transform_positions gives for MTR_POS_FROM_LEAF at the marker's leaf (marker "m<j>" is leaf j: the leaf count
    is exact), ref_type, props and seq as mtr_get_containing_segments reports the marker in the view that shows every
    leaf.  Leaf 8 is removed but still in the tree: FOUND without VISIBLE at the current view, VISIBLE before the
    remove.  Ordinals never mapped, negative ones included, answer none."""
    for k in (2, 3):
        n, log, lens = EDGE_LEAVES[k], edges.logs[k], edges.lens[k]
        pre = np.concatenate([[0], np.cumsum(lens)])
        markers = [j for j in range(n) if is_marker(j)]
        ordinal = {j: log.marker_ids[DocLog._id_key(f"m{j}")] for j in markers}
        assert sorted(ordinal.values()) == list(range(len(markers)))
        info = {j: s for j, s in zip(markers, edges.eng.containing_segments([(k, int(pre[j]), n, NON_WRITER) for j in markers]))}
        assert all(info[j]["leaf"] == j and info[j]["marker"] == 1 for j in markers)
        qs, want = [], []
        for rs, cl in edge_views(n):
            pos = edges.eng.transform_positions([(k, j, 0, 0, rs, cl, abi.POS_FROM_LEAF, 0) for j in markers])
            for j, p in zip(markers, pos):
                assert p["flags"] & abi.POS_FOUND
                qs.append((k, ordinal[j], rs, cl, BY_ID, 99))  # (the label is ignored)
                want.append((p["pos"], j, info[j]["ref_type"], info[j]["props"], info[j]["seq"],
                             FOUND | (VISIBLE if p["flags"] & abi.POS_VISIBLE else 0)))
            qs += [(k, len(markers), rs, cl, BY_ID, 0), (k, -1, rs, cl, BY_ID, 0), (k, INT32_MAX, rs, cl, BY_ID, 0)]
            want += [NONE] * 3
        rc, out = raw(edges.eng, [], [], qs)
        assert rc == len(qs), _err()
        got = [tuple(int(x) for x in r) for r in out]
        assert got == want
        by_q = dict(zip(qs, got))
        assert by_q[(k, ordinal[8], n + 1, NON_WRITER, BY_ID, 99)][5] == FOUND
        assert by_q[(k, ordinal[8], n, NON_WRITER, BY_ID, 99)][5] == FOUND | VISIBLE
        assert by_q[(k, ordinal[64], 40, NON_WRITER, BY_ID, 99)][5] == FOUND  # (a view that has not seen it yet)


@gpu
def test_engine_bindings(edges):
    """Engine.find_tiles and Engine.markers_from_ids against the composition and the raw rows."""
    from fluidframework_amd.batch import Unsupported

    eng, n, k = edges.eng, 130, 3
    cur = (n + 1, NON_WRITER)
    qs = [(k, p, *cur, label, prec) for p in (0, 50, 51, 200, INT32_MAX) for label in ("Eop", "pg", "nobody")
          for prec in (True, False)]
    got = eng.find_tiles(edges.it, qs)
    for q, g in zip(qs, got):
        li = {"Eop": 0, "pg": 1, "nobody": 3}[q[4]]
        want = edges.ref(edges.labels, edges.vals, (k, q[1], *cur, PREC if q[5] else FOLL, li))
        assert (g is None and want == NONE) or (g["pos"], g["leaf"], g["ref_type"], g["props"], g["seq"]) == want[:5]
    assert None in got and sum(g is not None for g in got) > 10 and all(g is None for q, g in zip(qs, got) if q[4] == "nobody")
    assert eng.find_tiles(Interner(), [(k, 0, *cur, "pg", False)]) == [None]  # (tables that never saw the key)
    ids = eng.markers_from_ids(edges.logs, [(k, "m1", *cur), (k, "m8", *cur), (k, "m8", n, NON_WRITER), (k, "m4", *cur),
                                            (k, 1, *cur), (2, "m57", 66, NON_WRITER)])
    assert ids[0]["leaf"] == 1 and ids[0]["visible"] and ids[1]["leaf"] == 8 and not ids[1]["visible"]
    assert ids[2]["visible"] and ids[2]["pos"] == ids[1]["pos"] and ids[3] is None and ids[4] is None
    assert ids[5]["leaf"] == 57 and ids[5]["pos"] == sum(edges.lens[2][:57]) - sum(edges.lens[2][j] for j in REMOVED)
    assert eng.find_tiles(edges.it, []) == [] and eng.markers_from_ids(edges.logs, []) == []
    log = DocLog()
    log.marker_ids[DocLog._id_key("a")] = 0
    log.marker_id_annotated = True
    with pytest.raises(Unsupported):
        eng.markers_from_ids([log], [(0, "a", 0, -1)])


@gpu
def test_repeats_order_and_counts(edges):
    """The same query twice, documents in descending order, one query, and no query at all: n = 0 does no device work
    (the launch census and the counters stand) but still checks the labels."""
    ref, lb, vals = edges.ref, edges.labels, edges.vals
    qs = [(d, 40, EDGE_LEAVES[d] + 1, NON_WRITER, mode, label) for d in (3, 2, 1, 0) for mode in (PREC, FOLL)
          for label in (0, 1, 2)]
    got = compare(edges.eng, ref, lb, vals, qs + qs)
    assert got[:len(qs)] == got[len(qs):] and len({g[:2] for g in got}) > 3
    assert compare(edges.eng, ref, lb, vals, qs[5:6]) == got[5:6]
    before = edges.eng.stats(), edges.eng.launch_counts()
    rc, out = raw(edges.eng, lb, vals, [])
    assert rc == 0 and (out == PATTERN).all()
    assert int(_lib().mtr_find_markers(edges.eng.h, None, 0, None, 0, None, 0, None)) == 0
    assert (edges.eng.stats(), edges.eng.launch_counts()) == before
    rc, out = raw(edges.eng, [(ANY, 0, 2)], [5, 4], [])
    assert rc == -1 and "label 0" in _err()


@gpu
def test_read_only(edges):
    """The kept summary's hashes and every document's exported leaves are what they were before the call."""
    eng = edges.eng
    eng.summarize()
    n_docs = len(EDGE_LEAVES)

    def state():
        return eng.hashes(n_docs).copy(), [[np.asarray(x).copy() for x in eng.export(d)[0]] for d in range(n_docs)]

    before = state()
    qs = [(d, p, EDGE_LEAVES[d] + 1, NON_WRITER, mode, label) for d in range(n_docs) for p in (0, 30, INT32_MAX)
          for mode in (PREC, FOLL) for label in (0, 2)] + [(d, 1, INT32_MAX, -1, BY_ID, 0) for d in range(n_docs)]
    compare(edges.eng, edges.ref, edges.labels, edges.vals, [q for q in qs if q[4] != BY_ID])
    assert raw(eng, edges.labels, edges.vals, qs)[0] == len(qs)
    after = state()
    assert np.array_equal(before[0], after[0])
    assert all(np.array_equal(a, b) for x, y in zip(before[1], after[1]) for a, b in zip(x, y))


@gpu
def test_marker_taken_by_zamboni():
    """A marker removed and then dropped from the tree once the minimum sequence number passes the remove: BY_ID
    answers none (the ordinal stays mapped, the segment is gone), a surviving marker is still found."""
    from fluidframework_amd.engine import Engine

    it = Interner()
    log = DocLog()
    log.start_collab("me")
    segs = [{"text": "abc"}, {"marker": {"refType": abi.REFTYPE_TILE}, "props": {"markerId": "gone"}}, {"text": "def"},
            {"marker": {"refType": abi.REFTYPE_TILE}, "props": {"markerId": "stays"}}, {"text": "ghi"}]
    at = 0
    for j, seg in enumerate(segs):
        log.message(_msg("w", {"type": 0, "pos1": at, "seg": seg}, j + 1, j), it)
        at += 1 if "marker" in seg else 3
    log.message(_msg("v", {"type": 1, "pos1": 3, "pos2": 4}, 6, 5), it)
    eng = Engine(1, max_segments=256, heap_entries=256, text_units=1 << 10, prop_words=1 << 10, remover_cells=256)
    try:
        eng.apply(build_batch([log], it))
        assert eng.status(0)[0] == 0 and len(eng.export(0)[0]) == 5
        gone, stays = (log.marker_ids[DocLog._id_key(x)] for x in ("gone", "stays"))
        qs = [(0, gone, 6, NON_WRITER, BY_ID, 0), (0, gone, 5, NON_WRITER, BY_ID, 0), (0, stays, 6, NON_WRITER, BY_ID, 0)]
        rc, out = raw(eng, [], [], qs)
        assert rc == 3 and out[0].tolist()[:2] == [3, 1] and out[0][5] == FOUND and out[1][5] == FOUND | VISIBLE
        assert out[2].tolist()[:2] == [6, 3] and out[2][5] == FOUND | VISIBLE
        # more messages move the minimum sequence number past the remove: zamboni unlinks the marker
        for s in range(7, 13):
            log.message(_msg("w", {"type": 0, "pos1": 0, "seg": {"text": "x"}}, s, s - 1, msn=s - 1), it)
        eng.apply(build_batch([log], it))
        assert eng.status(0)[0] == 0
        rows = eng.range_segments([(0, 0, None, INT32_MAX, -1)])[0]
        assert not any(s["removed"] for s in eng.range_segments([(0, 0, None, 5, NON_WRITER)])[0])  # (it left the tree)
        left = [s for s in rows if s["marker"]]
        assert len(left) == 1
        rc, out = raw(eng, [], [], [(0, gone, 12, NON_WRITER, BY_ID, 0), (0, gone, 5, NON_WRITER, BY_ID, 0),
                                    (0, stays, INT32_MAX, -1, BY_ID, 0)])
        assert rc == 3 and tuple(out[0]) == NONE and tuple(out[1]) == NONE
        assert tuple(out[2]) == (left[0]["start"], left[0]["leaf"], left[0]["ref_type"], left[0]["props"], left[0]["seq"],
                                 FOUND | VISIBLE)
    finally:
        eng.close()


# ---------------------------------------------------------------- the generated fleet
from test_segment_queries import HOLED, N_SMALL, WRITERS, fleet  # noqa: E402, F401


def _fleet_labels(f, ref):
    """MTR_LABEL_ANY, then every (key, value) pair a marker of the fleet carries in its local view, as a label."""
    pairs = set()
    for d in range(f.n):
        for s in ref.rows(d, INT32_MAX, -1):
            if s["marker"] and s["props"] != -1:
                pairs |= set(ref.words(d)(s["props"]))
    pairs = sorted(pairs)
    return [(ANY, 0, 0)] + [(k, i, 1) for i, (k, v) in enumerate(pairs)], [v for k, v in pairs]


@gpu
def test_fleet_views(fleet):  # noqa: F811
    """Oracle-generated documents with several writers, markers and removes, and the hole-layout HBM document: views at
    the minimum sequence number, between it and the current one and at the current one, of a writer and of a client
    that wrote nothing, the local view and NonCollabClient; the positions -1, 0, 1, len - 1, len, len + 1, INT32_MAX and
    20 seeded random ones; both directions; in shuffled document order."""
    ref = Reference(fleet.eng)
    labels, vals = _fleet_labels(fleet, ref)
    rnd = random.Random(0x71e5)
    qs = []
    for d in range(fleet.n):
        st = fleet.orcs[d].state()
        low, cur = int(st[0]), int(st[1])
        views = [(rs, cl) for rs in (low, (low + cur) // 2, cur) for cl in (1 + d % WRITERS, NON_WRITER)] + \
            [(INT32_MAX, -1), (cur, -2)]
        if d == HOLED:
            views = [(cur, 1), (cur // 2, 1), (INT32_MAX, -1)]
        for rs, cl in views:
            L = ref.length(d, rs, cl)
            ps = [-1, 0, 1, L - 1, L, L + 1, INT32_MAX] + [rnd.randint(0, max(L, 1)) for _ in range(20)]
            some = [0] + rnd.sample(range(1, len(labels)), min(2, len(labels) - 1))
            qs += [(d, p, rs, cl, mode, label) for p in ps for mode in (PREC, FOLL) for label in some]
    qs = list(dict.fromkeys(qs))
    rnd.shuffle(qs)
    got = compare(fleet.eng, ref, labels, vals, qs)
    # (coverage of the legs, not a property of the call: hits and misses both occur in number, on every small document)
    found = [g for g in got if g[5]]
    assert len(found) > 1000 and sum(1 for g in got if g == NONE) > 1000
    assert {q[0] for q, g in zip(qs, got) if g[5]} >= set(range(N_SMALL))
    holed = [g for q, g in zip(qs, got) if q[0] == HOLED and g[5]]
    # (the holed document's ordinals count live leaves: they stay below its exported leaf count, well below its slots)
    leaves = len(fleet.eng.export(HOLED)[0])
    assert fleet.eng.stats()["max_leaves"] > leaves
    assert all(g[1] < leaves for g in holed)
    if len(labels) > 1:  # (labelled hits took the property path)
        assert any(g[5] for q, g in zip(qs, got) if q[5] > 0)


@gpu
def test_matrix_vectors():
    """A SharedMatrix pair holds no markers: PRECEDING and FOLLOWING answer none."""
    from fluidframework_amd.engine import Engine
    from fluidframework_amd.synth import make_cfg, tables

    ops = 200
    cfg = make_cfg(1, ops, writers=WRITERS, max_lag=16, weights=(12, 8, 80), max_text=4, max_range=3)
    eng = Engine(2, max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=1 << 15, prop_words=1024,
                 remover_cells=4096, ops_per_launch=64)
    try:
        eng.generate_matrix(cfg, tables(writers=WRITERS))
        assert [eng.status(d)[0] for d in (0, 1)] == [0, 0]
        qs = [(d, p, rs, cl, mode, 0) for d in (0, 1) for p in (-1, 0, 5, INT32_MAX) for rs, cl in ((ops, 1), (INT32_MAX, -1))
              for mode in (PREC, FOLL)]
        rc, out = raw(eng, [(ANY, 0, 0)], [], qs)
        assert rc == len(qs), _err()
        assert all(tuple(r) == NONE for r in out)
        assert eng.view_length(0, INT32_MAX, -1) > 0
    finally:
        eng.close()
