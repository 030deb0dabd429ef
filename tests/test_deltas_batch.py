"""mtr_get_deltas_batch: the delta records of many documents in one launch, with the property sets of their
regenerate records.

The batched call is defined by the calls that exist, so every check here is word for word against Engine.deltas(d)
(mtr_get_deltas) and Engine.props(d, ref) (mtr_get_props) on the same engine state -- themselves pinned to the oracle
by test_catchup.py, test_regenerate.py and test_matrix*.py; the batch is never compared against itself.

The fleet (one engine of 9 documents, one batch of 8):
  0  ops, none flagged                 4  100 two-unit inserts ending in a newline (zamboni appends none), then a
  1  one flagged insert (1 record)        flagged annotate over all 100 leaves and a flagged remove over 70 of them
  2  exactly 64 records                5  pending local ops and a flagged MTR_OP_REGENERATE of each: an insert with
  3  65 records (a second round)          properties (REGEN_X len >= 0), one without (-1), a remove, an annotate
  6, 7  a matrix pair: flagged set-cells, tracked vector inserts, a remote remove whose handles zamboni recycles,
        a flagged vector regenerate (REGEN_X carries a start handle: no words)
  8  inside max_docs, beyond the batch (count 0)
The single calls' own results show that each of these states is present.
"""
import numpy as np
import pytest

from fluidframework_amd import abi, regen
from fluidframework_amd.batch import DocLog, Interner, build_batch
from fluidframework_amd.cells import DELTA_CELL, DELTA_RECYCLE, CellMatrixLog
from fluidframework_amd.sequence import SequenceLog, resolve_all

pytestmark = pytest.mark.gpu

PATTERN = 0x5a5a5a5a
N_FLEET = 9    # the engine's documents
N_BATCH = 8    # ... of which the batch holds the first eight
REGEN_DOC, ROWS_DOC, COLS_DOC = 5, 6, 7
U = abi.HANDLE_UNALLOCATED


def ins(pos, seg):
    return {"type": 0, "pos1": pos, "seg": seg}


def rem(a, b):
    return {"type": 1, "pos1": a, "pos2": b}


def ann(a, b, props):
    return {"type": 2, "pos1": a, "pos2": b, "props": props}


def _msg(client, op, seq, ref, msn=0):
    return {"clientId": client, "sequenceNumber": seq, "referenceSequenceNumber": ref, "minimumSequenceNumber": msn,
            "type": "op", "contents": op}


# ---------------------------------------------------------------- the documents
def _plain_doc(it):
    log = SequenceLog(legacy=True)
    log.start_collab("me")
    log.message(_msg("w", ins(0, "x" * 40), 1, 0), it)
    log.message(_msg("w", ins(20, "--"), 2, 1), it)
    return log


def _lagging_inserts(it, n):
    """n lagging inserts (referenceSequenceNumber != seq - 1: SequenceLog flags each MTR_F_DELTA) -> n records."""
    log = SequenceLog(legacy=True)
    log.start_collab("me")
    log.message(_msg("w", ins(0, "base"), 1, 0), it)
    for k in range(n):
        log.message(_msg("v", ins(k % 4, "ab"[k % 2]), k + 2, 0 if k == 0 else k), it)
    return log


def _wide_doc(it):
    log = SequenceLog(legacy=True)
    log.start_collab("me")
    seq = 0
    for i in range(100):  # 100 leaves of two units; the newline keeps zamboni from appending them
        seq += 1
        log.message(_msg("w", ins(2 * i, "a\n"), seq, seq - 1), it)
    log.message(_msg("v", ann(0, 200, {"k": 1}), seq + 1, seq - 1), it)  # lagging: one record per leaf
    log.message(_msg("v", rem(10, 150), seq + 2, seq), it)               # lagging: one per removed leaf
    return log


REGEN_OPS = [ins(0, {"text": "abcdef", "props": {"prop1": "foo"}}), ins(6, "xyz"), rem(1, 2), ann(2, 4, {"prop2": "bar"})]


def _regen_doc(it):
    """Pending local ops, then regeneratePendingOp of each in queue order (test_regenerate.py's Writer, in one batch).
    Returns (log, firsts): firsts[k] = the first regenerate record of REGEN_OPS[k]."""
    log = DocLog()
    log.start_collab("local user")
    for op in REGEN_OPS:
        log.local_op(op, it)
    return log, [log.regenerate(op) for op in REGEN_OPS]


def _matrix_doc(it):
    m = CellMatrixLog()
    m.start_collab("m")
    seq = 0
    for contents in ({"target": "cols", "type": 0, "pos1": 0, "seg": [2, U]},
                     {"target": "rows", "type": 0, "pos1": 0, "seg": [4, U]},
                     {"type": 2, "row": 1, "col": 0, "value": 5},   # (allocates the rows' and the cols' handles)
                     {"target": "rows", "type": 1, "pos1": 0, "pos2": 2}):
        seq += 1
        m.message(_msg("w", contents, seq, seq - 1, msn=seq - 1), it)
    for _ in range(4):  # the window moves past the remove: zamboni unlinks its rows and recycles their handles
        seq += 1
        m.message(_msg("w", {"target": "rows", "type": 0, "pos1": 0, "seg": [1, U]}, seq, seq - 1, msn=seq - 1), it)
    m.local_vector_op("rows", {"pos1": 1, "seg": [3, U], "type": 0}, track=1)
    m.local_vector_op("cols", {"pos1": 0, "seg": [2, U], "type": 0}, track=2)
    m.local_set_cell(0, 0, 7)
    m.local_set_cell(2, 1, 8)
    m.regenerate_vector("rows", {"pos1": 1, "seg": [3, U], "type": 0})
    return m


def fleet_logs(it):
    """-> (the batch's eight logs, the regenerate document's first record indices)."""
    rlog, firsts = _regen_doc(it)
    m = _matrix_doc(it)
    return [_plain_doc(it), _lagging_inserts(it, 1), _lagging_inserts(it, 64), _lagging_inserts(it, 65), _wide_doc(it),
            rlog, m, m.cols_log()], firsts


def fleet_engine():
    from fluidframework_amd.engine import Engine

    eng = Engine(N_FLEET, max_segments=1024, heap_entries=1024, text_units=1 << 12, prop_words=1 << 10,
                 remover_cells=1 << 10, ops_per_launch=64)
    eng.set_matrix(ROWS_DOC, COLS_DOC)
    return eng


# ---------------------------------------------------------------- the raw calls
def _lib():
    from fluidframework_amd.engine import lib
    return lib()


def err():
    return _lib().mtr_last_error().decode()


def call(eng, docs, n, out, cap, first, props=None, props_cap=0, props_off=None):
    d = None if docs is None else np.ascontiguousarray(docs, dtype="<u4")
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return int(_lib().mtr_get_deltas_batch(eng.h, None if d is None or d.size == 0 else d.ctypes.data, n, p(out), cap,
                                           p(first), p(props), props_cap, p(props_off)))


def batched(eng, docs, n=None, props="fetch"):
    """The size query, then the fetch into buffers of exactly the sizes, guard words behind each.  props: "skip" (no
    props part), "size" (props_off alone) or "fetch".  -> (doc_first, records, props_off | None, words | None)."""
    n = len(docs) if n is None else n
    size = np.full(n + 1, PATTERN, dtype="<i8")
    total = call(eng, docs, n, None, 0, size)
    assert total >= 0, err()
    assert size[0] == 0 and size[n] == total and (np.diff(size) >= 0).all()
    out = np.full(4 * (total + 2), PATTERN, dtype="<u4")
    first = np.full(n + 2, PATTERN, dtype="<i8")
    recs = out[:4 * total].view(abi.DELTA_DTYPE)
    if props == "skip":
        assert call(eng, docs, n, out, total, first) == total, err()
        poff = words = None
    else:
        poff = np.full(total + 3, PATTERN, dtype="<i8")
        assert call(eng, docs, n, out, total, first, None, 0, poff) == total, err()  # (the words' size query)
        assert (poff[total + 1:] == PATTERN).all() and poff[0] == 0 and (np.diff(poff[:total + 1]) >= 0).all()
        nw = int(poff[total])
        poff = poff[:total + 1]
        words = None
        if props == "fetch":
            got_recs = recs.copy()
            out[:] = PATTERN
            w = np.full(nw + 4, PATTERN, dtype="<u4")
            poff2 = np.full(total + 3, PATTERN, dtype="<i8")
            assert call(eng, docs, n, out, total, first, w, nw, poff2) == total, err()
            assert np.array_equal(poff2[:total + 1], poff) and (poff2[total + 1:] == PATTERN).all()
            assert np.array_equal(recs, got_recs)
            assert (w[nw:] == PATTERN).all()  # (nothing past the words)
            words = w[:nw]
    assert np.array_equal(first[:n + 1], size) and first[n + 1] == PATTERN
    assert (out[4 * total:] == PATTERN).all()  # (nothing past the records)
    return size, recs, poff, words


def single_words(eng, d, recs):
    """Per record of document d the words the batch is to bring: mtr_get_props' [n, key id, value id, ...] for a
    REGEN_X record with len >= 0 of a SharedString document, none otherwise."""
    out = []
    for r in recs:
        w = []
        if d not in (ROWS_DOC, COLS_DOC) and int(r["kind"]) == abi.DELTA_REGEN_X and int(r["len"]) >= 0:
            pairs = eng.props(d, int(r["len"]))
            w = [len(pairs)] + [x for kv in pairs for x in kv]
        out.append(np.array(w, dtype="<u4"))
    return out


def compare(f, docs, n=None, props="fetch"):
    """mtr_get_deltas_batch over `docs` against the single calls' results (f.singles, f.words); returns the total."""
    first, recs, poff, words = batched(f.eng, docs, n, props)
    listed = list(range(n)) if docs is None else list(docs)
    at = 0
    for i, d in enumerate(listed):
        want = f.singles[d]
        assert first[i] == at, f"doc_first[{i}] = {first[i]}, the single calls sum to {at}"
        got = recs[at:at + len(want)]
        assert np.array_equal(got, want), f"listed {i} (document {d}): {got.tolist()} != {want.tolist()}"
        if poff is not None:
            for k, w in enumerate(f.words[d]):
                assert poff[at + k + 1] - poff[at + k] == w.size, f"listed {i} (document {d}) record {k}: word count"
                if words is not None:
                    assert np.array_equal(words[poff[at + k]:poff[at + k + 1]], w), f"document {d} record {k}: words"
        at += len(want)
    assert first[len(listed)] == at and len(recs) == at
    return at


class _Fleet:
    pass


@pytest.fixture(scope="module")
def fleet():
    it = Interner()
    f = _Fleet()
    f.it = it
    f.logs, f.firsts = fleet_logs(it)
    f.eng = fleet_engine()
    f.eng.apply(build_batch(f.logs, it))
    for d in range(N_BATCH):
        st, op = f.eng.status(d)
        assert st == 0, f"document {d}: status {st:#x} at op {op}"
    f.singles = [f.eng.deltas(d) for d in range(N_FLEET)]  # the reference, computed once
    f.words = [single_words(f.eng, d, f.singles[d]) for d in range(N_FLEET)]
    for a in f.singles:
        a.setflags(write=False)
    f.total = sum(len(a) for a in f.singles)
    yield f
    f.eng.close()


def test_fleet_holds_the_states_the_batch_must_answer(fleet):
    s = fleet.singles
    assert [len(a) for a in s[:4]] == [0, 1, 64, 65] and len(s[8]) == 0
    k4 = s[4]["kind"]
    assert (k4 == abi.OP_ANNOTATE).sum() > 64 and (k4 == abi.OP_REMOVE).sum() > 64 and len(k4) >= 130
    r = s[REGEN_DOC]
    x = r[r["kind"] == abi.DELTA_REGEN_X]
    assert (x["len"] >= 0).any() and (x["len"] == -1).any()
    assert {abi.DELTA_REGEN, abi.DELTA_REGEN + 1, abi.DELTA_REGEN + 2} <= set(r["kind"].tolist())
    assert any(w.size >= 3 for w in fleet.words[REGEN_DOC])  # a property set with at least one pair
    rows, cols = s[ROWS_DOC], s[COLS_DOC]
    assert (rows["kind"] == DELTA_CELL).sum() >= 2 and (rows["kind"] == DELTA_RECYCLE).any()
    assert (rows["kind"] == abi.DELTA_TLINK).any() and (cols["kind"] == abi.DELTA_TLINK).any()
    assert (rows["kind"] == abi.DELTA_REGEN_X).any()  # (its len is a handle: no words)
    assert all(w.size == 0 for d in (ROWS_DOC, COLS_DOC) for w in fleet.words[d])


def test_null_list_is_every_document(fleet):
    assert compare(fleet, None, n=N_FLEET) == fleet.total
    assert compare(fleet, None, n=4) == 130  # (documents 0 .. n - 1)


def test_scrambled_list_with_repeats(fleet):
    docs = [5, 0, 4, 8, 6, 5, 1, 7, 3, 2, 4]
    assert compare(fleet, docs) == sum(len(fleet.singles[d]) for d in docs)


def test_list_of_empty_documents_writes_nothing(fleet):
    assert compare(fleet, [0, 8, 0]) == 0
    out = np.full(16, PATTERN, dtype="<u4")
    first = np.full(4, PATTERN, dtype="<i8")
    poff = np.full(4, PATTERN, dtype="<i8")
    w = np.full(4, PATTERN, dtype="<u4")
    assert call(fleet.eng, [0, 8, 0], 3, out, 4, first, w, w.size, poff) == 0, err()
    assert first.tolist() == [0, 0, 0, 0] and poff.tolist() == [0] + [PATTERN] * 3
    assert (out == PATTERN).all() and (w == PATTERN).all()


@pytest.mark.parametrize("doc", range(N_FLEET))
def test_one_document(fleet, doc):
    assert compare(fleet, [doc]) == len(fleet.singles[doc])


@pytest.mark.parametrize("props", ["skip", "size", "fetch"])
def test_props_part_fetched_sized_and_skipped(fleet, props):
    docs = [REGEN_DOC, ROWS_DOC, 3, REGEN_DOC]
    assert compare(fleet, docs, props=props) == sum(len(fleet.singles[d]) for d in docs)


def test_python_hosts_shape_the_records_like_the_single_calls(fleet):
    eng, docs = fleet.eng, [4, 0, 5, 8, 6, 1]
    many = eng.deltas_many(docs)
    assert all(a.dtype == abi.DELTA_DTYPE and np.array_equal(a, fleet.singles[d]) for a, d in zip(many, docs))
    first, recs = eng.deltas_batch()  # (every document of the engine)
    assert first.tolist() == np.cumsum([0] + [len(a) for a in fleet.singles]).tolist()
    assert np.array_equal(recs, np.concatenate(fleet.singles))
    first, recs = eng.deltas_batch(n=3)
    assert first.tolist() == [0, 0, 1, 65] and len(recs) == 65
    first, recs, poff, words = eng.deltas_batch([], props=True)
    assert first.tolist() == [0] and poff.tolist() == [0] and recs.size == 0 and words.size == 0
    from fluidframework_amd.live import EngineExecutor
    assert all(np.array_equal(a, fleet.singles[d]) for a, d in zip(EngineExecutor(eng).deltas_many(docs), docs))


def test_regenerated_ops_from_the_batched_records(fleet):
    """regen.batched: the regenerated ops built from the batch's (records, props_off, props) equal those built with an
    Engine.props call per reference."""
    eng, d = fleet.eng, REGEN_DOC
    first, recs, poff, words = eng.deltas_batch([3, d], props=True)
    a, b = int(first[1]), int(first[2])
    rec_map, props_of = regen.batched(recs[a:b], poff[a:b + 1], words, fleet.it)
    want_map = regen.records(fleet.singles[d])
    assert rec_map == want_map
    for op, f0 in zip(REGEN_OPS, fleet.firsts):
        want = regen.regenerated_op(op, want_map, f0, lambda r: regen.props_dict(eng.props(d, r), fleet.it))
        assert regen.regenerated_op(op, rec_map, f0, props_of) == want
    seg = regen.regenerated_op(REGEN_OPS[1], rec_map, fleet.firsts[1], props_of)
    assert seg["type"] == 0 and isinstance(seg["seg"], str)  # (the insert without properties: len == -1)


def test_catch_ups_resolved_from_one_call(fleet):
    """sequence.resolve_all fills the same catch-up contents as SequenceLog.resolve(engine.deltas(d)) per document."""
    import copy

    docs = [4, 1, 0, 3, 2]
    logs = [fleet.logs[d] for d in docs]
    assert sum(1 for log in logs if log.pending) == 4
    want = []
    for log, d in zip(logs, docs):
        c = copy.deepcopy(log)
        c.resolve(fleet.singles[d])
        want.append(c.catchup_blob())
    mine = [copy.deepcopy(log) for log in logs]
    resolve_all(fleet.eng, mine, docs)
    assert [log.catchup_blob() for log in mine] == want and any(w for w in want)


def test_second_batch_without_flagged_ops():
    """After a batch with no MTR_F_DELTA op every count is 0, also for the documents that held records before."""
    it = Interner()
    eng = fleet_engine()
    logs, _ = fleet_logs(it)
    eng.apply(build_batch(logs, it))
    assert call(eng, None, N_FLEET, None, 0, np.zeros(N_FLEET + 1, dtype="<i8")) > 0
    for log in logs[:5]:
        log.pending = []
    logs[0].message(_msg("w", ins(0, "q"), 3, 2), it)  # (caught up: not flagged)
    eng.apply(build_batch(logs, it))
    f = _Fleet()
    f.eng = eng
    f.singles = [eng.deltas(d) for d in range(N_BATCH)] + [np.zeros(0, dtype=abi.DELTA_DTYPE)]
    assert all(len(a) == 0 for a in f.singles)
    f.words = [[] for _ in range(N_FLEET)]
    assert compare(f, None, n=N_FLEET) == 0
    assert compare(f, [5, 4, 6, 2]) == 0
    eng.close()


def test_live_session_fetches_a_step_with_one_call():
    """LiveSession.sync leaves in `deltas` what the per-client Engine.deltas calls return."""
    from fluidframework_amd.engine import Engine
    from fluidframework_amd.live import EngineExecutor, LiveSession

    eng = Engine(3, max_segments=1024, heap_entries=1024, text_units=1 << 12, prop_words=1 << 10, remover_cells=1 << 10)
    s = LiveSession(EngineExecutor(eng), legacy=True)
    cs = [s.client(n) for n in ("a", "b", "c")]
    for c in cs:
        c.log.start_collab(c.name)
    for c in cs[:2]:
        c.log.message(_msg("w", ins(0, "base"), 1, 0), s.it)
        c.log.message(_msg("w", ins(4, "!"), 2, 1), s.it)
        c.log.message(_msg("v", ins(1, "z"), 3, 1), s.it)  # lagging (it saw the base alone): flagged
    s.sync()
    assert sorted(s.deltas) == [0, 1, 2] and len(s.deltas[2]) == 0  # (every client with records in the step)
    for d in (0, 1):
        assert len(s.deltas[d]) == 1 and np.array_equal(s.deltas[d], eng.deltas(d))
    assert not cs[0].log.pending and not cs[1].log.pending
    eng.close()
