"""mtr_query_intervals at the C ABI: n = 0, every refusal (named by its index, nothing written), the size query,
MTR_SUMMARY_TOO_SMALL, and repeated calls with growing and shrinking n (the work buffers' lifetime)."""
import random

import numpy as np
import pytest

from fluidframework_amd import abi
from fluidframework_amd.batch import Interner, build_batch
from test_interval_queries_batch import CAPS, NEXT, OVERLAP, PATTERN, PREVIOUS, _edge_doc, _err, _lib, raw

pytestmark = pytest.mark.gpu

SETS = [(0, 0, 10), (1, 10, 6), (0, 4, 3)]
REFS = [(2 * k, 2 * k + 1) for k in range(10)] + [(k, k + 6) for k in range(6)]


@pytest.fixture(scope="module")
def eng():
    from fluidframework_amd.engine import Engine

    rnd = random.Random(11)
    it = Interner()
    e = Engine(3, ref_slots=32, **CAPS)
    e.apply(build_batch([_edge_doc(it, 70, rnd, n_refs=20)[0], _edge_doc(it, 20, rnd, n_refs=12)[0]], it))
    assert [e.status(d)[0] for d in (0, 1)] == [0, 0]
    yield e
    e.close()


def _good():
    return [(0, 5, 120, OVERLAP), (1, 3, 30, OVERLAP), (2, 40, 40, PREVIOUS), (0, 9, 9, NEXT), (1, 0, 0, NEXT),
            (2, 0, 200, OVERLAP), (0, 77, 77, PREVIOUS)]


def _refused(eng, sets, refs, qs, needle):
    rc, first, status, _ = raw(eng, sets, refs, qs)
    assert rc == -1 and needle in _err(), _err()
    assert (first == PATTERN).all() and (status == PATTERN).all()


def test_no_queries(eng):
    rc, first, status, rows = raw(eng, SETS, REFS, [])
    assert rc == 0 and first[0] == 0 and (status == PATTERN).all()
    assert int(_lib().mtr_query_intervals(eng.h, None, 0, None, 0, None, 0, None, None, None, 0)) == 0


@pytest.mark.parametrize("what", ["set_first", "set_last", "mode", "mode_negative"])
def test_bad_queries_are_refused_with_their_index(eng, what):
    qs = _good()
    k = {"set_first": 0, "set_last": len(qs) - 1}.get(what, 4)
    s, a, b, mode = qs[k]
    qs[k] = {"set_first": (3, a, b, mode), "set_last": (1 << 30, a, b, mode), "mode": (s, a, b, 3),
             "mode_negative": (s, a, b, -1)}[what]
    _refused(eng, SETS, REFS, qs, f"query {k} ")


@pytest.mark.parametrize("what", ["doc", "past_the_end", "first_past_the_end"])
def test_bad_sets_are_refused_with_their_index(eng, what):
    sets = list(SETS)
    k = {"doc": 1, "past_the_end": 2, "first_past_the_end": 0}[what]
    sets[k] = {"doc": (3, 10, 6), "past_the_end": (0, 14, 3), "first_past_the_end": (0, 0xffffffff, 2)}[what]
    _refused(eng, sets, REFS, _good(), f"set {k} ")


def test_unknown_reference_is_refused_by_set_and_interval(eng):
    """A reference id the document does not have is found on the device: document 1 holds 12 references."""
    refs = list(REFS)
    refs[13] = (3, 12)
    _refused(eng, SETS, refs, _good(), "set 1, interval 3")
    refs = list(REFS)
    refs[5] = (1 << 31, 2)  # (interval 5 of set 0, and interval 1 of set 2: the first set that holds it is named)
    _refused(eng, SETS, refs, _good(), "set 0, interval 5")


def test_missing_arrays_are_refused(eng):
    s = np.array(SETS, dtype=abi.INTERVAL_SET_DTYPE)
    r = np.array(REFS, dtype="<u4")
    q = np.array(_good(), dtype=abi.INTERVAL_QUERY_DTYPE)
    first = np.full(len(q) + 1, PATTERN, dtype="<i8")
    status = np.full(len(q), PATTERN, dtype="<i4")
    args = [s.ctypes.data, len(s), r.ctypes.data, len(r), q.ctypes.data, len(q), first.ctypes.data, status.ctypes.data]
    for missing in (0, 2, 4, 6, 7):
        a = list(args)
        a[missing] = None
        assert int(_lib().mtr_query_intervals(eng.h, *a, None, 0)) == -1 and "required" in _err()
        assert (first == PATTERN).all() and (status == PATTERN).all()


def test_size_query_and_too_small(eng):
    qs = _good()
    total, first, status, _ = raw(eng, SETS, REFS, qs, hits=False)
    assert total > 2 and first[0] == 0 and first[len(qs)] == total and (np.diff(first) >= 0).all()
    assert (status == 0).all()
    rc, first2, status2, rows = raw(eng, SETS, REFS, qs, cap=total - 1)
    assert rc == abi.MTR_SUMMARY_TOO_SMALL and np.array_equal(first, first2) and np.array_equal(status, status2)
    assert (rows == PATTERN).all()  # (no row was written)
    rc, _, _, rows = raw(eng, SETS, REFS, qs)
    assert rc == total and (rows[:, 0] >= 0).all() and (rows[:, 7] & ~abi.IVQ_TIE == 0).all()


def test_growing_and_shrinking_calls(eng):
    """The work buffers grow on demand and are reused: each call's rows equal those of the same queries asked alone."""
    base = _good()
    alone = {}
    for q in base:
        rc, _, _, rows = raw(eng, SETS, REFS, [q])
        assert rc >= 0, _err()
        alone[q] = rows.tolist()
    for reps in (1, 40, 3, 200, 1, 9):
        qs = base * reps
        rc, first, status, rows = raw(eng, SETS, REFS, qs)
        assert rc >= 0, _err()
        for i, q in enumerate(qs):
            assert rows[first[i]:first[i + 1]].tolist() == alone[q], (reps, i)


def test_buffers_are_released_with_the_engine():
    from fluidframework_amd.engine import Engine, live_bytes

    before = live_bytes()
    it = Interner()
    e = Engine(1, ref_slots=32, **CAPS)
    e.apply(build_batch([_edge_doc(it, 40, random.Random(2), n_refs=20)[0]], it))
    idle = live_bytes()
    first, status, hits = e.query_intervals([(0, 0, 10)], REFS[:10], [(0, 0, 100, OVERLAP)])
    assert first[1] == len(hits) > 0 and status[0] == 0
    assert live_bytes() > idle  # (the work buffers are the engine's own, and counted)
    e.close()
    assert live_bytes() == before
