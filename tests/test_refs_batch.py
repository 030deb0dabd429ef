"""mtr_get_refs: the local references of many documents in one launch (positions, states or compare keys).

The batched call is defined by the calls that exist, so every check here is word for word against
mtr_get_ref_positions / mtr_get_ref_states / mtr_get_ref_keys on the same engine state (themselves pinned to the oracle
by test_local_refs.py and test_interval_live.py); the batch is never compared against itself.

The fleet (one engine, ref_slots = 256, every document collaborating):
  0  text, no reference record        3  65 references (a second 64-reference block)
  1  one reference                    4  130 references on more than 64 leaves (below)
  2  exactly 64 references            5  never in a batch at all
Document 4: 100 two-unit inserts that end in a newline (zamboni appends none of them), 130 references of every kind
across them (SlideOnRemove, Simple, StayOnRemove, Transient), then an acked remove (sliding references leave its
segments, simple ones are let go), a pending local remove, three MTR_OP_REF_REMOVE records, and the minimum sequence
number raised step by step so that zamboni unlinks the acked-removed segments under the references still naming them
(key -2).  The single calls' own results show that each of these states is present.
"""
import random

import numpy as np
import pytest

from fluidframework_amd import abi
from fluidframework_amd.batch import DocLog, Interner, build_batch
from test_local_refs import SIMPLE, SLIDE, STAY, TRANSIENT, ins, rem

pytestmark = pytest.mark.gpu

MODES = (abi.REFS_POSITIONS, abi.REFS_STATES, abi.REFS_KEYS)
PATTERN = 0x5a5a5a5a
N_FLEET = 6
BIG = 4  # the 130-reference document


# ---------------------------------------------------------------- the raw calls
def _lib():
    from fluidframework_amd.engine import lib
    return lib()


def _err():
    return _lib().mtr_last_error().decode()


def _call(eng, docs, n, mode, out, cap, first):
    d = None if docs is None else np.ascontiguousarray(docs, dtype="<u4")
    return int(_lib().mtr_get_refs(eng.h, None if d is None or d.size == 0 else d.ctypes.data, n, mode,
                                   None if out is None else out.ctypes.data, cap,
                                   None if first is None else first.ctypes.data))


def _batched(eng, docs, mode, n=None):
    """The size query, then the fetch into a buffer of exactly the size -> (doc_first, words)."""
    n = len(docs) if n is None else n
    size = np.full(n + 1, PATTERN, dtype="<i8")
    total = _call(eng, docs, n, mode, None, 0, size)
    assert total >= 0, _err()
    assert size[0] == 0 and size[n] == total and (np.diff(size) >= 0).all()
    out = np.full(total * mode + 4, PATTERN, dtype="<i4")
    first = np.full(n + 1, PATTERN, dtype="<i8")
    assert _call(eng, docs, n, mode, out, total * mode, first) == total, _err()
    assert np.array_equal(first, size)
    assert (out[total * mode:] == PATTERN).all()  # (nothing past the words)
    return first, out[:total * mode]


def _single(eng, doc, mode):
    """The single call of `mode` on one document, as flat words."""
    fn = {abi.REFS_POSITIONS: eng.ref_positions, abi.REFS_STATES: eng.ref_states, abi.REFS_KEYS: eng.ref_keys}[mode]
    return np.array(fn(doc), dtype="<i4").reshape(-1)


def _compare(eng, docs, singles, mode, n=None):
    """mtr_get_refs over `docs` against the single calls' words (singles[mode][doc]); returns the total."""
    first, words = _batched(eng, docs, mode, n)
    listed = list(range(n)) if docs is None else list(docs)
    at = 0
    for i, d in enumerate(listed):
        want = singles[mode][d]
        assert first[i] == at, f"mode {mode}: doc_first[{i}] = {first[i]}, the single calls sum to {at}"
        got = words[mode * at:mode * at + want.size]
        assert np.array_equal(got, want), f"mode {mode}: listed {i} (document {d}): {got.tolist()} != {want.tolist()}"
        at += want.size // mode
    assert first[len(listed)] == at and words.size == mode * at
    return at


# ---------------------------------------------------------------- the documents
def _msg(client, op, seq, ref, msn=0):
    return {"clientId": client, "sequenceNumber": seq, "referenceSequenceNumber": ref, "minimumSequenceNumber": msn,
            "type": "op", "contents": op}


def _text_doc(it, units=70):
    log = DocLog()
    log.start_collab("me")
    log.message(_msg("w", ins(0, "x" * units), 1, 0), it)
    log.message(_msg("w", ins(units // 2, "--"), 2, 1), it)  # (splits the first segment)
    return log


def _with_refs(it, n):
    log = _text_doc(it)
    for r in range(n):
        log.create_ref(r, (SLIDE, SIMPLE, STAY)[r % 3])
    return log


def _big_doc(it):
    log = DocLog()
    log.start_collab("me")
    seq = 0
    for i in range(100):  # 100 leaves of two units; the newline keeps zamboni from appending them
        seq += 1
        log.message(_msg("w", ins(2 * i, "a\n"), seq, seq - 1), it)
    kinds = (SLIDE, SIMPLE, STAY, TRANSIENT, SLIDE)
    for r in range(130):
        log.create_ref((r * 3) % 200, kinds[r % 5])
    seq += 1
    log.message(_msg("w", rem(10, 30), seq, seq - 1), it)  # acked: references slide off or are let go
    log.local_op(rem(50, 60), it)                          # pending: references stay on removed segments
    for r in (5, 77, 129):
        log.remove_ref(r)
    for _ in range(80):  # zamboni is incremental: raise the minimum sequence number step by step
        log.seq_update(seq, seq)
    return log


class _Fleet:
    pass


@pytest.fixture(scope="module")
def fleet():
    from fluidframework_amd.engine import Engine

    it = Interner()
    logs = [_text_doc(it), _with_refs(it, 1), _with_refs(it, 64), _with_refs(it, 65), _big_doc(it)]
    f = _Fleet()
    f.eng = Engine(N_FLEET, max_segments=4096, heap_entries=4096, text_units=1 << 14, prop_words=1 << 12,
                   remover_cells=1 << 12, ops_per_launch=64, ref_slots=256)
    f.eng.apply(build_batch(logs, it))
    for d in range(len(logs)):
        st, op = f.eng.status(d)
        assert st == 0, f"document {d}: status {st:#x} at op {op}"
    f.singles = {m: [_single(f.eng, d, m) for d in range(N_FLEET)] for m in MODES}  # the reference, computed once
    for a in f.singles.values():
        for x in a:
            x.setflags(write=False)
    yield f
    f.eng.close()


def test_fleet_holds_the_states_the_batch_must_answer(fleet):
    """What the single calls report about the fleet: the counts, and in the 130-reference document every state the
    round body distinguishes."""
    assert [x.size for x in fleet.singles[abi.REFS_POSITIONS]] == [0, 1, 64, 65, 130, 0]
    k = fleet.singles[abi.REFS_KEYS][BIG].reshape(-1, 4)
    pos, bits, key = k[:, 0], k[:, 1], k[:, 2]
    assert key.max() >= 64                                     # more than 64 leaves: several leaf rounds
    assert (key == -2).any()                                   # a segment zamboni unlinked
    assert (key == -1).sum() >= 3                              # MTR_OP_REF_REMOVE: no segment
    assert ((bits & abi.REF_ST_REMOVED) != 0).any()            # on a pending-removed segment
    assert (pos == abi.DETACHED_POSITION).any() and (pos >= 0).any()
    transient = np.arange(130) % 5 == 3
    assert ((bits[transient] & abi.REF_ST_HELD) == 0).all() and (pos[transient] >= 0).any()


@pytest.mark.parametrize("mode", MODES)
def test_every_document_in_order(fleet, mode):
    assert _compare(fleet.eng, list(range(N_FLEET)), fleet.singles, mode) == 1 + 64 + 65 + 130


@pytest.mark.parametrize("mode", MODES)
def test_scrambled_list_with_a_repeat(fleet, mode):
    assert _compare(fleet.eng, [4, 0, 3, 5, 4, 1, 2], fleet.singles, mode) == 130 + 65 + 130 + 1 + 64


@pytest.mark.parametrize("mode", MODES)
def test_null_list_is_every_document(fleet, mode):
    assert _compare(fleet.eng, None, fleet.singles, mode, n=N_FLEET) == 260
    assert _compare(fleet.eng, None, fleet.singles, mode, n=3) == 65  # (documents 0 .. n - 1)


def test_reference_free_documents_write_no_words(fleet):
    out = np.full(16, PATTERN, dtype="<i4")
    first = np.full(4, PATTERN, dtype="<i8")
    assert _call(fleet.eng, [0, 5, 0], 3, abi.REFS_KEYS, out, out.size, first) == 0, _err()
    assert first.tolist() == [0, 0, 0, 0] and (out == PATTERN).all()


def test_sizes_and_errors(fleet):
    eng, docs = fleet.eng, [3, 4, 1]
    total = 65 + 130 + 1
    for mode in MODES:
        first = np.full(4, PATTERN, dtype="<i8")
        assert _call(eng, docs, 3, mode, None, 0, first) == total  # the size query
        assert first.tolist() == [0, 65, 195, 196]
        out = np.full(mode * total, PATTERN, dtype="<i4")
        first[:] = PATTERN
        assert _call(eng, docs, 3, mode, out, mode * total - 1, first) == abi.MTR_SUMMARY_TOO_SMALL
        assert first.tolist() == [0, 65, 195, 196] and (out == PATTERN).all()
    out = np.full(8 * total, PATTERN, dtype="<i4")
    first = np.full(4, PATTERN, dtype="<i8")

    def untouched():
        return (out == PATTERN).all() and (first == PATTERN).all()

    for mode in (0, 3, 8, -1):
        assert _call(eng, docs, 3, mode, out, out.size, first) == -1 and "mode" in _err() and untouched()
    assert _call(eng, docs, 3, abi.REFS_STATES, out, out.size, None) == -1 and "doc_first" in _err() and untouched()
    assert _call(eng, [3, 4, N_FLEET], 3, abi.REFS_STATES, out, out.size, first) == -1
    assert "index 2" in _err() and untouched()
    assert _call(eng, None, N_FLEET + 1, abi.REFS_STATES, out, out.size, first) == -1  # (documents 0 .. n - 1)
    assert f"index {N_FLEET}" in _err() and untouched()
    assert _call(eng, None, 0, abi.REFS_STATES, None, 0, first) == 0  # n = 0 is accepted
    assert first[0] == 0 and (first[1:] == PATTERN).all()
    assert _call(eng, None, 0, abi.REFS_STATES, None, 0, None) == 0


def test_python_hosts_shape_the_words_like_the_single_calls(fleet):
    eng, docs = fleet.eng, [4, 0, 3, 1]
    assert eng.ref_positions_many(docs) == [eng.ref_positions(d) for d in docs]
    assert eng.ref_states_many(docs) == [eng.ref_states(d) for d in docs]
    assert eng.ref_keys_many(docs) == [eng.ref_keys(d) for d in docs]
    assert eng.ref_keys_many() == [eng.ref_keys(d) for d in range(N_FLEET)]
    first, words = eng.refs_batch([], abi.REFS_KEYS)
    assert first.tolist() == [0] and words.size == 0


def test_engine_without_a_reference_table():
    """An engine that never saw a reference record has not allocated its table: every count is 0."""
    from fluidframework_amd.engine import Engine

    it = Interner()
    eng = Engine(3, max_segments=1024, heap_entries=1024, text_units=1 << 12, prop_words=1 << 10,
                 remover_cells=1 << 10, ref_slots=256)
    eng.apply(build_batch([_text_doc(it), _text_doc(it)], it))
    singles = {m: [_single(eng, d, m) for d in range(3)] for m in MODES}
    assert all(x.size == 0 for a in singles.values() for x in a)
    for mode in MODES:
        assert _compare(eng, [2, 0, 1, 0], singles, mode) == 0
        assert _compare(eng, None, singles, mode, n=3) == 0
    eng.close()


def test_document_that_was_reset():
    """Documents that held references and were then mtr_reset have none; a resubmit gives one of them references again."""
    from fluidframework_amd.engine import Engine

    it = Interner()
    eng = Engine(2, max_segments=1024, heap_entries=1024, text_units=1 << 12, prop_words=1 << 10,
                 remover_cells=1 << 10, ref_slots=256)
    eng.apply(build_batch([_with_refs(it, 7), _with_refs(it, 66)], it))
    singles = {m: [_single(eng, d, m) for d in range(2)] for m in MODES}
    for mode in MODES:
        assert _compare(eng, [1, 0], singles, mode) == 73
    eng.reset()
    singles = {m: [_single(eng, d, m) for d in range(2)] for m in MODES}
    for mode in MODES:
        assert _compare(eng, [1, 0], singles, mode) == 0
    it = Interner()
    eng.apply(build_batch([_with_refs(it, 9), _text_doc(it)], it))  # document 1: references before the reset, none now
    singles = {m: [_single(eng, d, m) for d in range(2)] for m in MODES}
    assert singles[abi.REFS_POSITIONS][1].size == 0
    for mode in MODES:
        assert _compare(eng, [1, 0, 1], singles, mode) == 9
    eng.close()


def test_hole_layout_document():
    """One document grown past 8,192 leaves by one-unit inserts with the minimum sequence number held at 0 (nothing
    merges): it is HBM-resident with hole slots, so the round body reads the leaf arrays through the holes."""
    from fluidframework_amd.engine import Engine

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
    eng = Engine(1, max_segments=16384, heap_entries=16384, text_units=1 << 15, prop_words=1 << 10,
                 remover_cells=1 << 12, ref_slots=256)
    eng.apply(build_batch([log], it))
    st, op = eng.status(0)
    assert st == 0, f"status {st:#x} at op {op}"
    assert eng.launch_counts()["global_mode"] > 0
    assert eng.stats()["max_leaves"] > len(eng.export(0)[0]) > 8192  # more slots than leaves: holes
    singles = {m: [_single(eng, 0, m)] for m in MODES}
    assert singles[abi.REFS_POSITIONS][0].size == 70
    assert singles[abi.REFS_KEYS][0].reshape(-1, 4)[:, 2].max() > 8192
    for mode in MODES:
        assert _compare(eng, [0], singles, mode) == 70
        assert _compare(eng, [0, 0], singles, mode) == 140
    eng.close()


def test_read_only_and_memory_accounting():
    """The call drops none of the cached summary results, and its work buffers are counted and freed with the engine."""
    from fluidframework_amd.engine import Engine, live_bytes

    start = live_bytes()
    it = Interner()
    eng = Engine(3, max_segments=1024, heap_entries=1024, text_units=1 << 12, prop_words=1 << 10,
                 remover_cells=1 << 10, ref_slots=256)
    eng.apply(build_batch([_with_refs(it, 66), _text_doc(it), _with_refs(it, 3)], it))
    eng.summarize()
    hashes = eng.hashes().copy()
    ids = eng.blob_ids()
    singles = {m: [_single(eng, d, m) for d in range(3)] for m in MODES}
    held = live_bytes()
    for mode in MODES:
        assert _compare(eng, [2, 1, 0], singles, mode) == 69
    assert live_bytes() > held  # (the work buffers are counted)
    assert np.array_equal(eng.hashes(), hashes)
    assert eng.blob_ids() == ids
    assert eng.summary(0) and eng.summary(2)
    eng.close()
    assert live_bytes() == start


def test_interval_headers_from_one_call():
    """sequence.interval_headers over several interval documents of one engine equals the per-document
    log.interval_header(engine.ref_states(d)) bytes, and ref_keys_many equals ref_keys."""
    import interval_farm as F
    from fluidframework_amd.engine import Engine
    from fluidframework_amd.live import EngineExecutor
    from fluidframework_amd.sequence import SequenceLog, interval_headers

    it = Interner()
    logs = []
    for seed in (1, 2, 3):  # test_intervals' farm documents
        initial, msgs, _ = F.farm(seed)
        log = SequenceLog(legacy=False)
        log.local_insert(0, initial, it)
        log.start_collab("observer")
        for m in msgs:
            log.message(dict(m), it)
        logs.append(log)
    recipe = SequenceLog(legacy=False)  # ... and the withIntervals fixture's recipe (90 intervals: 180 references)
    for o in F.snapshot_recipe("withIntervals"):
        recipe.local_insert(o[1], o[2], it)
    for label, s, e, t, i in F.fixture_ids():
        recipe.interval_collection(label).local_add(recipe, s, e, t, {"intervalId": i})
    logs.append(recipe)
    plain = SequenceLog(legacy=False)  # no interval collection: no header
    plain.local_insert(0, "plain", it)
    logs.append(plain)
    eng = Engine(len(logs), ref_slots=4096)
    eng.apply(build_batch(logs, it))
    for d in range(len(logs)):
        st, op = eng.status(d)
        assert st == 0, f"document {d}: status {st:#x} at op {op}"
    want = [log.interval_header(eng.ref_states(d)) for d, log in enumerate(logs)]
    assert want[3].decode() == F.V2_HEADER and want[4] is None and all(w for w in want[:3])
    docs = [3, 0, 4, 2, 1]
    assert interval_headers(eng, [logs[d] for d in docs], docs) == [want[d] for d in docs]
    assert eng.ref_keys_many(docs) == [eng.ref_keys(d) for d in docs]
    assert EngineExecutor(eng).ref_keys_many(docs) == [eng.ref_keys(d) for d in docs]
    eng.close()
