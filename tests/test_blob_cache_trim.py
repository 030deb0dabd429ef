"""The blob-id cache's life cycle: generations, mtr_blob_cache_ages, _trim, _trim_to, _export and _import.

The reference everywhere is gitid.BlobCacheModel, an insertion-ordered dict from hex id to stamp: every GPU test drives
the engine and a model with the same calls and, after every step, compares size, generation, export() (ids, order and
ages), ages(4), ages(1024) and blob_cache_has over ids the cache holds and ids it does not.  Everything is exact.
"""
import gc
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- CPU
def _model():
    from fluidframework_amd.gitid import BlobCacheModel

    return BlobCacheModel()


A, B, C, D, E, F = ("%040x" % k for k in (0xa, 0xb, 0xc, 0xd, 0xe, 0xf))


def _three_generations():
    """a, b at generation 0; c, d and b again at 1; e and a again at 2"""
    m = _model()
    m.add([A, B])
    m.add_summary([C, B, D, C])
    m.add_summary([E, A])
    return m


def test_model_add_and_stamps():
    m = _three_generations()
    assert m.generation == 2 and m.size() == 5
    assert m.export() == ([A, B, C, D, E], [0, 1, 1, 1, 0])
    assert m.has([A, F, E]) == [True, False, True]
    assert m.ages(3) == [2, 3, 0] and m.ages(1) == [5] and m.ages(2) == [2, 3]
    for n in (0, 1025):
        with pytest.raises(ValueError):
            m.ages(n)


def test_model_trim_keeps_order():
    m = _three_generations()
    assert m.trim(0) == 0 and m.export() == ([A, B, C, D, E], [0, 1, 1, 1, 0])
    assert m.trim(2) == 3
    assert m.export() == ([A, E], [0, 0]) and m.generation == 2
    m.add([B])  # a removed id is new again: appended
    assert m.export() == ([A, E, B], [0, 0, 0])
    assert m.trim(3) == 3 and m.size() == 0 and m.generation == 2


def test_model_trim_to_drops_whole_generations():
    m = _three_generations()  # stamps: a 2, b 1, c 1, d 1, e 2
    assert m.trim_to(5) == 0 and m.size() == 5
    assert m.trim_to(4) == 3  # the cap falls inside generation 1: all three of it go
    assert m.export() == ([A, E], [0, 0])
    m = _three_generations()
    assert m.trim_to(1) == 5  # not even the youngest generation fits
    assert m.size() == 0 and m.generation == 2
    m = _three_generations()
    assert m.trim_to(0) == 5 and m.export() == ([], []) and m.generation == 2


def test_model_ages_lump_the_rest():
    m = _model()
    for k in range(6):  # one id a generation, generations 1..6
        m.add_summary(["%040x" % (0x100 + k)])
    assert m.generation == 6
    assert m.ages(1024)[:7] == [1, 1, 1, 1, 1, 1, 0] and sum(m.ages(1024)) == 6
    assert m.ages(4) == [1, 1, 1, 3]


def test_model_import_export_round_trip():
    m = _three_generations()
    ids, ages = m.export()
    r = _model()
    r.import_(ids, ages)
    assert r.export() == (ids, ages) == ([A, B, C, D, E], [0, 1, 1, 1, 0])
    assert r.generation == 1  # (the largest age: no entry of m is older)
    # into a model that is further on: the stamps are relative to its generation
    r = _model()
    r.import_([F], [7])
    r.import_(ids, ages)
    assert r.generation == 7 and r.export() == ([F, A, B, C, D, E], [7, 0, 1, 1, 1, 0])


def test_model_import_youngest_age_wins():
    m = _model()
    m.import_([A, B, A, A], [5, 2, 1, 3])
    assert m.generation == 5 and m.export() == ([A, B], [1, 2])
    m.import_([B], [4])  # an older age moves nothing
    assert m.export() == ([A, B], [1, 2])
    with pytest.raises(ValueError):
        m.import_([A], [])


def test_model_clear_resets_the_generation():
    m = _three_generations()
    m.clear()
    assert m.generation == 0 and m.size() == 0 and m.export() == ([], []) and m.ages(2) == [0, 0]
    m.add([B])
    assert m.export() == ([B], [0])


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mtr.h")).read()
    names = set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", text))
    assert {"mtr_blob_cache_generation", "mtr_blob_cache_ages", "mtr_blob_cache_trim", "mtr_blob_cache_trim_to",
            "mtr_blob_cache_export", "mtr_blob_cache_import"} <= names


def test_stamp_kernel_uses_no_scratch():
    from fluidframework_amd import build

    build.build_engine()
    res = json.load(open(os.path.join(ROOT, "fluidframework_amd", "build", "kernel_resources.json")))
    ks = {k: v for k, v in res.items() if "cache_stamp_kernel" in k}
    assert ks, "no resource entry for the stamp kernel"
    for k, v in ks.items():
        assert build._CACHE_STAMP_KERNEL.match(k), k
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["VGPRs Spill"] == 0, (k, v)
    # the build's own check refuses such a kernel
    name = next(iter(ks))
    with pytest.raises(RuntimeError, match="cache stamp kernel"):
        build.check_cache_stamp_no_scratch({name: {"ScratchSize [bytes/lane]": 16, "VGPRs Spill": 1}})
    assert not build.check_cache_stamp_no_scratch({name: {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0}})


# ---------------------------------------------------------------- GPU
def _engine(n_docs, **kw):
    from test_blob_cache import _engine as make

    return make(n_docs, **kw)


def _random_ids(rng, n):
    ids = rng.integers(0, 256, size=(n, 20), dtype="u1")
    assert len({r.tobytes() for r in ids}) == n
    return ids


def _hex(ids):
    if len(ids) and isinstance(ids[0], str):
        return list(ids)
    return [r.tobytes().hex() for r in np.asarray(ids, dtype="u1").reshape(-1, 20)]


class _Pair:
    """An engine and a model given the same calls; check() compares all there is to see."""

    def __init__(self, eng, probe):
        self.eng, self.model, self.probe = eng, _model(), probe
        self.probe_hex = _hex(probe)

    def add(self, ids):
        self.eng.blob_cache_add(ids)
        self.model.add(_hex(ids))
        self.check()

    def import_(self, ids, ages):
        self.eng.blob_cache_import(ids, ages)
        self.model.import_(_hex(ids), list(ages))
        self.check()

    def bump(self, ids, to):
        """moves both to generation `to`: an import of an entry of stamp 0 at age `to` changes nothing else"""
        assert self.model.stamps[_hex(ids[:1])[0]] == 0
        self.import_(ids[:1], [to])
        assert self.model.generation == to

    def trim(self, g):
        got, want = self.eng.blob_cache_trim(g), self.model.trim(g)
        assert got == want, (g, got, want)
        self.check()
        return got

    def trim_to(self, cap):
        got, want = self.eng.blob_cache_trim_to(cap), self.model.trim_to(cap)
        assert got == want, (cap, got, want)
        self.check()
        return got

    def check(self):
        eng, model = self.eng, self.model
        assert eng.blob_cache_size() == model.size()
        assert eng.blob_cache_generation() == model.generation
        ids, ages = eng.blob_cache_export()
        want_ids, want_ages = model.export()
        assert ids.shape == (len(want_ids), 20) and ages.dtype == np.dtype("<u4")
        assert _hex(ids) == want_ids
        assert ages.tolist() == want_ages
        for n in (4, 1024):
            assert eng.blob_cache_ages(n).tolist() == model.ages(n), n
        has = eng.blob_cache_has(self.probe).astype(bool).tolist()
        assert has == model.has(self.probe_hex), (sum(has), model.size())


@pytest.mark.gpu
def test_stamps_and_histogram():
    from fluidframework_amd.engine import EngineError

    rng = np.random.default_rng(0x57a3b)
    ids = _random_ids(rng, 5302)
    ids, others = ids[:5002], ids[5002:]
    p = _Pair(_engine(1), np.concatenate([ids, others]))
    p.check()  # (no cache yet)
    cuts = [0, 700, 1500, 2200, 3000, 3600, 4300, 5001]  # the 1,024-slot array doubles at 513 and at 1,025 entries ...
    for g in range(7):
        if g:
            p.bump(ids, g)
        lo, hi = cuts[g], cuts[g + 1]
        mid = (lo + hi) // 2
        p.add(ids[lo:mid])  # stamped with the generation
        if g == 1:
            p.add([_hex(ids[mid:mid + 1])[0]])  # (a hex string)
        # given ages, some ids twice, some of them older than anything so far: the generation moves on with them
        chunk = np.concatenate([ids[mid:hi], ids[mid:hi][::3]])
        p.import_(chunk, rng.integers(0, g + 2, size=len(chunk)))
        if g:  # ids of earlier generations again: add moves their stamps up, an import with an old age does not
            # (ids[0] keeps stamp 0: bump() moves the generation with it)
            p.add(ids[1 + rng.choice(lo - 1, 150, replace=False)])
            again = 1 + rng.choice(lo - 1, 150, replace=False)
            p.import_(ids[again], rng.integers(0, p.model.generation + 1, size=150))
    assert p.model.size() == 5001 and len(set(p.model.stamps.values())) >= 7
    # 70 copies of one id, more than a wave of equal lanes, at 70 different ages: the youngest wins
    ages70 = rng.permutation(np.arange(3, 73))
    p.import_(np.repeat(ids[5001:5002], 70, axis=0), ages70)
    assert p.model.export()[1][-1] == 3 and p.model.size() == 5002
    p.import_(np.repeat(ids[40:41], 70, axis=0), rng.permutation(np.arange(1, 71)))
    assert p.model.generation - p.model.stamps[_hex(ids[40:41])[0]] == 1
    assert p.eng.blob_cache_ages(4)[3] == sum(p.model.ages(1024)[3:]) > 0
    for n in (0, 1025, -1):
        with pytest.raises(EngineError, match="outside 1..1024"):
            p.eng.blob_cache_ages(n)
    with pytest.raises(EngineError, match="ages"):
        p.eng.blob_cache_import(ids[:2], [1])
    p.check()


def _colliding_ids():
    """test_blob_cache.test_colliding_ids' 600 ids: 300 equal in the first 16 bytes and 300 equal in the last 16, so
    that whatever the hash reads, one of the groups is a single probe chain."""
    rng = np.random.default_rng(0xc0111de)
    tail = np.repeat(rng.integers(0, 256, size=(1, 20), dtype="u1"), 300, axis=0)
    tail[:, 16:] = np.arange(300, dtype=">u4").view("u1").reshape(300, 4)
    head = np.repeat(rng.integers(0, 256, size=(1, 20), dtype="u1"), 300, axis=0)
    head[:, :4] = np.arange(300, dtype="<u4").view("u1").reshape(300, 4)
    return np.concatenate([tail, head])


@pytest.mark.gpu
def test_trim_rebuilds_the_probe_chains():
    """Every other id of a 300-entry probe chain goes: a removal that empties the slots of the removed entries and
    leaves the rest where it is loses the survivors behind the first hole.  (Confirmed once against a scratch build
    with exactly that trim: the check after the trim found 150 of the 300 survivors.)"""
    ids = _colliding_ids()
    p = _Pair(_engine(1), ids)
    p.add(ids[::2])  # generation 0: every other id of both chains
    p.bump(ids, 1)
    p.add(ids[1::2][::-1])  # generation 1: the ids between them
    assert p.model.size() == 600
    assert p.trim(1) == 300
    has = p.eng.blob_cache_has(ids)
    assert has[1::2].all(), int(has[1::2].sum())  # every survivor is still found
    assert not has[::2].any(), int(has[::2].sum())  # no removed id is
    assert _hex(p.eng.blob_cache_export()[0]) == _hex(ids[1::2][::-1])
    p.add(ids[4:5])  # a removed id is new again, appended at the end
    got = p.eng.blob_cache_export()
    assert got[0][-1].tobytes() == ids[4].tobytes() and got[1][-1] == 0 and len(got[1]) == 301
    p.add(ids[::2][::-1])
    assert p.eng.blob_cache_has(ids).all() and p.model.size() == 600


@pytest.mark.gpu
def test_shrink_and_empty():
    from fluidframework_amd.engine import live_bytes

    rng = np.random.default_rng(0x5121)
    ids = _random_ids(rng, 5202)
    ids, others = ids[:5002], ids[5002:]
    gc.collect()
    eng = _engine(1)
    base = live_bytes()  # an engine without a cache
    p = _Pair(eng, np.concatenate([ids, others]))
    p.add(ids)  # 5,002 entries: 16,384 slots
    p.bump(ids, 1)
    p.add(ids[[7, 2500, 5001]])
    # a trim that removes nothing
    before = p.eng.blob_cache_export()
    full = live_bytes()
    assert p.trim(0) == 0
    after = p.eng.blob_cache_export()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert live_bytes() <= full
    # 3 survivors: the table, the stamps and the slot array (1,024 again) are new and small, the old ones released
    full = live_bytes()
    assert p.trim(1) == 4999
    assert _hex(p.eng.blob_cache_export()[0]) == _hex(ids[[7, 2500, 5001]])
    small = live_bytes()
    # (5,002 entries took at least 24 bytes each, 3 take the smallest table's 512 x 24; the slots went from 16,384 to
    # 1,024 words: a slot array that stayed would leave the drop at the table's share alone)
    assert full - small >= (5002 - 512) * 24 + (16384 - 1024) * 4, (base, small, full)
    # no survivor: as after a clear, but for the generation
    assert p.trim(2) == 3
    assert eng.blob_cache_size() == 0 and not eng.blob_cache_has(p.probe).any()
    assert eng.blob_cache_generation() == 1
    assert live_bytes() == base, (base, live_bytes())
    assert p.trim(5) == 0 and p.trim_to(0) == 0  # (nothing to trim)
    # it starts again, small, and doubles again
    p.add(ids[:400])
    at_1024 = live_bytes()
    p.add(ids[400:1500])
    assert live_bytes() > at_1024 and p.model.size() == 1500
    assert p.model.export()[1] == [0] * 1500  # (stamped with generation 1, which stayed)
    eng.blob_cache_clear()
    p.model.clear()
    p.check()
    assert eng.blob_cache_generation() == 0 and live_bytes() == base
    eng.close()


@pytest.mark.gpu
def test_trim_to():
    rng = np.random.default_rng(0x7710)
    ids = _random_ids(rng, 700)
    p = _Pair(_engine(1), ids)
    # generations 0..4 hold 240, 180, 120, 60 and 30 entries (ages 4..0), in mixed table order
    ages = rng.permutation(np.repeat([4, 3, 2, 1, 0], [240, 180, 120, 60, 30]))
    p.import_(ids[:630], ages)
    assert p.model.generation == 4 and p.model.ages(5) == [30, 60, 120, 180, 240]
    assert p.trim_to(631) == 0 and p.trim_to(630) == 0  # a cap equal to the size
    assert p.trim_to(629) == 240  # one below: the oldest generation goes whole
    assert p.trim_to(250) == 180  # inside generation 1 (390 with it, 210 without): it goes whole
    assert p.model.ages(5) == [30, 60, 120, 0, 0]
    assert p.trim_to(29) == 210  # not even the youngest generation fits
    assert p.model.size() == 0 and p.eng.blob_cache_generation() == 4
    p.import_(ids[:100], rng.integers(0, 5, size=100))
    assert p.trim_to(0) == 100 and p.eng.blob_cache_generation() == 4
    # more generations than the histogram has buckets: the cutoff is searched with the count kernel
    old = [0, 1, 7, 1021, 1022, 1023, 1024, 1025, 1500, 2999, 3000]
    p.import_(ids[100:700], rng.choice(old, size=600))
    assert p.model.generation == 3000 and p.model.ages(1024)[1023] > 250
    size = 600
    for cap in (599, 520, 440, 380, 330, 290, 200, 60, 0):
        size -= p.trim_to(cap)
        assert size == p.model.size() <= cap
    assert size == 0 and p.eng.blob_cache_generation() == 3000


@pytest.mark.gpu
def test_against_summaries():
    from test_blob_cache import FIRST, HELD, _N, _check_novel, _fleet_batch, _id, _record_blobs

    eng = _engine(_N, chunk_size=8)
    model = _model()
    shorter = (17, 63, 101)  # every document of one log: their last blobs are in no other document
    # batch A summarized and acknowledged: generation 1
    eng.apply(_fleet_batch())
    eng.summarize()
    blobs_a = _record_blobs(eng, _N)
    ids_a = [_id(b) for doc in blobs_a for b in doc]
    eng.blob_cache_add_summary()
    model.add_summary(ids_a)
    # some documents one message group shorter: generation 2
    eng.reset()
    eng.apply(_fleet_batch(shorter=shorter))
    eng.summarize()
    ids_b = [_id(b) for doc in _record_blobs(eng, _N) for b in doc]
    eng.blob_cache_add_summary()
    model.add_summary(ids_b)
    assert eng.blob_cache_generation() == model.generation == 2
    ids, ages = eng.blob_cache_export()
    assert (_hex(ids), ages.tolist()) == model.export()
    only_a, shared = set(ids_a) - set(ids_b), set(ids_a) & set(ids_b)
    assert only_a and shared and set(ages.tolist()) == {0, 1}
    # what generation 2 did not refer to goes
    removed = eng.blob_cache_trim(2)
    assert removed == model.trim(2) == len(only_a)
    assert not eng.blob_cache_has(sorted(only_a)).any() and eng.blob_cache_has(sorted(shared)).all()
    # A again: the blobs only A's summary held are to be uploaded again, the shared ones are held
    eng.reset()
    eng.apply(_fleet_batch())
    eng.summarize()
    assert _record_blobs(eng, _N) == blobs_a
    want = _check_novel(eng, blobs_a, model.ids())
    rows = [r for doc in want for r in doc]
    flat = [b for doc in blobs_a for b in doc]
    for i in only_a:
        k = ids_a.index(i)
        assert rows[k] == (i, FIRST, k, flat[k])
    assert all(s == HELD and b is None for i, s, _, b in rows if i in shared)
    assert sum(s == FIRST for _, s, _, _ in rows) == len(only_a)
    eng.close()


@pytest.mark.gpu
def test_invalidation():
    from test_blob_cache import _N, _check_novel, _fleet_batch, _id, _record_blobs

    n = _N
    eng = _engine(n, chunk_size=8)
    model = _model()
    eng.apply(_fleet_batch())
    eng.summarize()
    blobs = _record_blobs(eng, n)
    ids = [[_id(b) for b in doc] for doc in blobs]
    distinct = sorted({i for doc in ids for i in doc})
    eng.set_baseline([[i for i in doc[:2]] for doc in ids[:100]])

    def others():
        return eng.summary_delta(0, n), eng.blob_ids(0, n), eng.tree_ids(0, n)

    before = others()
    assert any(b is None for doc in before[0] for _, b in doc) and any(b is not None for doc in before[0] for _, b in doc)
    half = len(distinct) // 2
    eng.blob_cache_add(distinct[:half])
    model.add(distinct[:half])
    eng.blob_cache_import(distinct[half:], [1] * (len(distinct) - half))  # generation 1; this half has stamp 0
    model.import_(distinct[half:], [1] * (len(distinct) - half))
    eng.blob_cache_add(distinct[:3])  # stamp 1
    model.add(distinct[:3])
    _check_novel(eng, blobs, model.ids())
    built = eng.timing()["novel_ms"]
    assert built > 0
    # reading the cache, stamping held ids and a trim that finds nothing leave the result that was built in place
    assert eng.blob_cache_generation() == 1
    assert eng.blob_cache_ages(3).tolist() == model.ages(3) == [3, len(distinct) - 3, 0]
    assert _hex(eng.blob_cache_export()[0]) == model.ids()
    assert eng.blob_cache_trim(0) == 0 and eng.blob_cache_trim_to(len(distinct)) == 0
    eng.blob_cache_add(distinct[3:5])  # (held: only their stamps move)
    model.add(distinct[3:5])
    _check_novel(eng, blobs, model.ids())
    assert eng.timing()["novel_ms"] == built, "the novel result was built again"
    assert others() == before
    # a trim that removes entries drops it: the next result knows the removed ids as new
    assert eng.blob_cache_trim(1) == model.trim(1) == len(distinct) - 5
    assert model.ids() == distinct[:5]
    want = _check_novel(eng, blobs, model.ids())
    assert {s for doc in want for _, s, _, _ in doc} == {0, 1, 2}
    assert eng.timing()["cache_trim_ms"] > 0
    assert eng.blob_cache_trim_to(0) == model.trim_to(0) == 5
    _check_novel(eng, blobs, None)
    assert others() == before  # the positional baseline and its delta never noticed
    eng.close()


@pytest.mark.gpu
def test_export_import_across_engines_and_resets():
    from fluidframework_amd.engine import lib

    rng = np.random.default_rng(0xe7907)
    ids = _random_ids(rng, 1400)
    ids, others = ids[:1300], ids[1300:]
    a = _Pair(_engine(1), np.concatenate([ids, others]))
    a.add(ids[:500])
    a.import_(ids[300:900], rng.integers(0, 6, size=600))
    assert a.model.generation == 5 and a.trim(3) > 300
    a.import_(ids[:100], [5] * 100)  # (removed, so new again: stamp 0)
    a.add(ids[850:1300])
    assert 0 < a.model.size() < 1300 and 0 in a.model.stamps.values()
    n = a.model.size()
    exp = a.eng.blob_cache_export()
    # a second engine takes the export over
    b = _Pair(_engine(1), a.probe)
    b.import_(*exp)
    got = b.eng.blob_cache_export()
    assert got[0].tobytes() == exp[0].tobytes() and got[1].tobytes() == exp[1].tobytes()
    assert b.eng.blob_cache_generation() == a.eng.blob_cache_generation() == a.model.generation
    assert np.array_equal(b.eng.blob_cache_has(a.probe), a.eng.blob_cache_has(a.probe))
    # mtr_reset changes nothing
    a.eng.reset()
    a.check()
    got = a.eng.blob_cache_export()
    assert got[0].tobytes() == exp[0].tobytes() and got[1].tobytes() == exp[1].tobytes()
    # a buffer one entry too small: -(count), nothing written
    raw, age = np.full((n + 1, 20), 0xa5, dtype="u1"), np.full(n + 1, 0xa5a5a5a5, dtype="<u4")
    assert lib().mtr_blob_cache_export(a.eng.h, raw.ctypes.data, age.ctypes.data, n - 1) == -n
    assert (raw == 0xa5).all() and (age == 0xa5a5a5a5).all()
    assert lib().mtr_blob_cache_export(a.eng.h, raw.ctypes.data, age.ctypes.data, n) == n
    assert raw[:n].tobytes() == exp[0].tobytes() and age[:n].tobytes() == exp[1].tobytes()
    assert (raw[n] == 0xa5).all() and age[n] == 0xa5a5a5a5
    # an import of nothing
    assert lib().mtr_blob_cache_import(a.eng.h, None, None, 0) == 0
    a.import_(ids[:0], [])
    assert a.eng.blob_cache_export()[0].tobytes() == exp[0].tobytes()
    # without an engine
    assert lib().mtr_blob_cache_generation(None) == -1 and lib().mtr_blob_cache_trim(None, 0) == -1
    assert b"no engine" in lib().mtr_last_error()
    a.eng.close()
    b.eng.close()


@pytest.mark.gpu
def test_determinism():
    rng = np.random.default_rng(0xde7e)
    ids = _random_ids(rng, 3000)
    calls = [("add", np.concatenate([ids[:900], ids[:900][::-1]])),
             ("import", ids[600:1800], rng.integers(0, 9, size=1200)),
             ("add", ids[rng.choice(1800, 700)]),
             ("trim", 4),
             ("add", np.concatenate([ids[1500:3000][::-1], ids[:200]])),
             ("import", np.repeat(ids[5:6], 70, axis=0), rng.permutation(70)),
             ("trim_to", 2300),  # (2,458 entries by then; the two oldest generations go)
             ("add", ids[::7])]
    exports = []
    for _ in range(2):
        eng = _engine(1)
        removed = []
        for c in calls:
            if c[0] == "add":
                eng.blob_cache_add(c[1])
            elif c[0] == "import":
                eng.blob_cache_import(c[1], c[2])
            elif c[0] == "trim":
                removed.append(eng.blob_cache_trim(c[1]))
            else:
                removed.append(eng.blob_cache_trim_to(c[1]))
        x, y = eng.blob_cache_export()
        exports.append((x.tobytes(), y.tobytes(), eng.blob_cache_generation(), tuple(removed)))
        eng.close()
    assert exports[0] == exports[1]
    assert len(exports[0][1]) // 4 > 2000 and exports[0][3] == (769, 204)
    # ... and they are the model's
    model = _model()
    for c in calls:
        if c[0] == "add":
            model.add(_hex(c[1]))
        elif c[0] == "import":
            model.import_(_hex(c[1]), list(c[2]))
        else:
            (model.trim if c[0] == "trim" else model.trim_to)(c[1])
    want_ids, want_ages = model.export()
    assert exports[0][0] == bytes.fromhex("".join(want_ids))
    assert exports[0][1] == np.array(want_ages, dtype="<u4").tobytes() and exports[0][2] == model.generation == 69
