"""The device blob-id cache (mtr_blob_cache_*) and the hand-over against it (mtr_summary_novel): a blob is uploaded
once, whatever document and index it sits at -- SummaryTreeUploadManager.writeSummaryBlob's rule against blobsShaCache.

The reference everywhere is gitid.summary_novel: hashlib ids (gitid.git_blob_id) and a dict over the blobs of
eng.summaries().  Everything is exact.
"""
import gc
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_SMALL = -3  # include/mtr.h: MTR_SUMMARY_TOO_SMALL
HELD, FIRST, REPEAT = 0, 1, 2


# ---------------------------------------------------------------- CPU
def _id(b):
    from fluidframework_amd.gitid import git_blob_id

    return git_blob_id(b)


_BLOBS = [[b"header 0", b"body 0"], [b"header 1"], [b"header 2", b"", b"body 2 b"]]


def test_host_definition_no_cache():
    from fluidframework_amd.gitid import summary_novel

    want = [[(_id(b"header 0"), FIRST, 0, b"header 0"), (_id(b"body 0"), FIRST, 1, b"body 0")],
            [(_id(b"header 1"), FIRST, 2, b"header 1")],
            [(_id(b"header 2"), FIRST, 3, b"header 2"), (_id(b""), FIRST, 4, b""), (_id(b"body 2 b"), FIRST, 5, b"body 2 b")]]
    assert summary_novel(None, _BLOBS) == want
    assert summary_novel(set(), _BLOBS) == want


def test_host_definition_full_cache():
    from fluidframework_amd.gitid import summary_novel

    cache = {_id(b) for doc in _BLOBS for b in doc}
    assert summary_novel(cache, _BLOBS) == [[(_id(b), HELD, -1, None) for b in doc] for doc in _BLOBS]


def test_host_definition_one_id_missing():
    from fluidframework_amd.gitid import summary_novel

    cache = {_id(b) for doc in _BLOBS for b in doc} - {_id(b"body 2 b")}
    got = summary_novel(cache, _BLOBS)
    assert got[:2] == [[(_id(b), HELD, -1, None) for b in doc] for doc in _BLOBS[:2]]
    assert got[2] == [(_id(b"header 2"), HELD, -1, None), (_id(b""), HELD, -1, None),
                      (_id(b"body 2 b"), FIRST, 5, b"body 2 b")]


def test_host_definition_repeats_in_and_across_documents():
    from fluidframework_amd.gitid import summary_novel

    blobs = [[b"h", b"same", b"x", b"same"], [b"same", b"h"], [b"y"]]
    got = summary_novel(None, blobs)
    assert got[0] == [(_id(b"h"), FIRST, 0, b"h"), (_id(b"same"), FIRST, 1, b"same"), (_id(b"x"), FIRST, 2, b"x"),
                      (_id(b"same"), REPEAT, 1, None)]
    assert got[1] == [(_id(b"same"), REPEAT, 1, None), (_id(b"h"), REPEAT, 0, None)]
    assert got[2] == [(_id(b"y"), FIRST, 6, b"y")]
    # held ids are held wherever they repeat
    got = summary_novel({_id(b"same")}, blobs)
    assert [s for _, s, _, _ in got[0] + got[1]] == [FIRST, HELD, FIRST, HELD, HELD, REPEAT]


def test_host_definition_empty_blob_and_zero_documents():
    from fluidframework_amd.gitid import summary_novel

    empty = "e69de29bb2d1d6434b8b29ae775ad8c2e48c5391"  # git's empty blob
    assert summary_novel(None, [[b""], [], [b""]]) == [[(empty, FIRST, 0, b"")], [], [(empty, REPEAT, 0, None)]]
    assert summary_novel([empty], [[b""]]) == [[(empty, HELD, -1, None)]]
    assert summary_novel(None, []) == [] and summary_novel({empty}, []) == []


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mtr.h")).read()
    names = set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", text))
    assert {"mtr_blob_cache_add", "mtr_blob_cache_add_summary", "mtr_blob_cache_clear", "mtr_blob_cache_size",
            "mtr_blob_cache_has", "mtr_summary_novel_info", "mtr_summary_novel"} <= names


def test_classify_kernel_uses_no_scratch():
    from fluidframework_amd import build

    build.build_engine()
    res = json.load(open(os.path.join(ROOT, "fluidframework_amd", "build", "kernel_resources.json")))
    ks = {k: v for k, v in res.items() if "novel_classify_kernel" in k}
    assert ks, "no resource entry for the classify kernel"
    for k, v in ks.items():
        assert build._NOVEL_CLASSIFY_KERNEL.match(k), k
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["VGPRs Spill"] == 0, (k, v)
    # the build's own check refuses such a kernel
    name = next(iter(ks))
    with pytest.raises(RuntimeError, match="novel classify kernel"):
        build.check_novel_classify_no_scratch({name: {"ScratchSize [bytes/lane]": 16, "VGPRs Spill": 1}})
    assert not build.check_novel_classify_no_scratch({name: {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0}})


def test_clear_and_size_without_an_engine():
    """Refused before any device call, each under its own name."""
    from fluidframework_amd import build
    from fluidframework_amd.engine import lib

    build.build_engine()
    for name in ("mtr_blob_cache_clear", "mtr_blob_cache_size"):
        assert getattr(lib(), name)(None) == -1
        assert lib().mtr_last_error() == (name + ": no engine").encode()


# ---------------------------------------------------------------- GPU
def _engine(n_docs, **kw):
    from fluidframework_amd.engine import Engine

    caps = dict(max_segments=4096, heap_entries=4096, text_units=1 << 16, prop_words=1 << 14, remover_cells=1 << 12)
    caps.update(kw)
    return Engine(n_docs, **caps)


def _random_ids(rng, n):
    return rng.integers(0, 256, size=(n, 20), dtype="u1")


@pytest.mark.gpu
def test_set_semantics_with_host_ids():
    eng = _engine(1)
    rng = np.random.default_rng(0xcac4e)
    ids = _random_ids(rng, 5002)
    assert len({r.tobytes() for r in ids}) == 5002
    others = _random_ids(rng, 5000)
    assert not {r.tobytes() for r in others} & {r.tobytes() for r in ids}
    assert eng.blob_cache_size() == 0 and not eng.blob_cache_has(ids).any()
    eng.blob_cache_add([])  # (a no-op)
    assert eng.blob_cache_size() == 0

    def check(held):
        assert eng.blob_cache_size() == held
        has = eng.blob_cache_has(ids)
        assert has[:held].all() and not has[held:].any(), (held, int(has.sum()))
        assert not eng.blob_cache_has(others).any()

    eng.blob_cache_add([ids[0].tobytes().hex()])  # (hex strings)
    check(1)
    eng.blob_cache_add(np.repeat(ids[1:2], 70, axis=0))  # 70 copies of one id: more than a wave of equal lanes
    check(2)
    for a, b in ((2, 1700), (1700, 3300), (3300, 5002)):  # a 1,024-slot table doubles at least twice on the way
        # (each call also repeats ids of the call before and holds every id of its own twice)
        eng.blob_cache_add(np.concatenate([ids[max(a - 50, 0):b], ids[a:b][::-1]]))
        check(b)
    eng.blob_cache_add(ids)  # (all held: absorbed)
    check(5002)
    eng.blob_cache_clear()
    assert eng.blob_cache_size() == 0
    assert not eng.blob_cache_has(ids).any() and not eng.blob_cache_has(others).any()
    eng.blob_cache_add(ids[:3])  # (a cleared cache starts again)
    check(3)


@pytest.mark.gpu
def test_colliding_ids():
    """Ids that agree in 16 of their 20 bytes: a compare of a prefix or a suffix alone takes them for one id, and
    whatever the hash reads, one of the two groups falls into a single probe chain."""
    eng = _engine(1)
    rng = np.random.default_rng(0xc0111de)
    tail = np.repeat(_random_ids(rng, 1), 300, axis=0)  # equal in the first 16 bytes, different in the last 4
    tail[:, 16:] = np.arange(300, dtype=">u4").view("u1").reshape(300, 4)
    head = np.repeat(_random_ids(rng, 1), 300, axis=0)  # equal in the last 16 bytes, different in the first 4
    head[:, :4] = np.arange(300, dtype="<u4").view("u1").reshape(300, 4)
    ids = np.concatenate([tail, head])
    eng.blob_cache_add(ids[::2])
    assert eng.blob_cache_size() == 300
    has = eng.blob_cache_has(ids)
    assert has[::2].all() and not has[1::2].any(), (int(has[::2].sum()), int(has[1::2].sum()))
    eng.blob_cache_add(ids[1::2][::-1])
    assert eng.blob_cache_size() == 600 and eng.blob_cache_has(ids).all()


_FLEET = {}
_N = 136
_OTHER = {17: "len_8-clients_4", 40: "len_8-clients_8", 63: "len_8-clients_4", 88: "len_8-clients_8",
          101: "len_8-clients_4", 135: "len_8-clients_8"}
_BATCHES = {}
_GROUPS = 64  # groups of messages replayed of each log (all of them)


def _fleet_batch(shorter=()):
    """136 documents: the golden log len_8-clients_2 in 130 of them, two other logs in six more, interleaved.
    `shorter`: documents that stop one group of messages before the log's end."""
    from fixtures import load_replay, replay_files, replay_log

    from fluidframework_amd.batch import Interner, build_batch

    if shorter not in _BATCHES:
        it = Interner()
        groups = {name: load_replay([p for p in replay_files() if name in p][0])
                  for name in ["len_8-clients_2"] + sorted(set(_OTHER.values()))}
        logs = []
        for d in range(_N):
            g = groups[_OTHER.get(d, "len_8-clients_2")]
            log = replay_log(g, it)
            for grp in g[:_GROUPS - int(d in shorter)]:
                for m in grp["msgs"]:
                    log.message(m, it)
            logs.append(log)
        _BATCHES[shorter] = build_batch(logs, it)
    return _BATCHES[shorter]


def _record_blobs(eng, n):
    from fluidframework_amd.engine import Engine

    buf, off = eng.summaries(0, n)
    return [Engine.split_record(buf, int(off[d]), int(off[d + 1])) for d in range(n)]


def _fleet():
    """The fleet's engine (8-unit chunks: several body_k a document), its blobs from eng.summaries() and their ids,
    made once; a test leaves the summary as it is and sets the cache it wants first."""
    if not _FLEET:
        eng = _engine(_N, chunk_size=8)
        eng.apply(_fleet_batch())
        assert eng.stats()["bad_docs"] == 0
        eng.summarize()
        blobs = _record_blobs(eng, _N)
        ids = [[_id(b) for b in doc] for doc in blobs]
        assert min(len(doc) for doc in blobs) >= 3, "documents without several body_k blobs"
        assert all(blobs[d] == blobs[0] for d in range(_N) if d not in _OTHER)
        assert all(blobs[d] != blobs[0] for d in _OTHER)
        _FLEET.update(eng=eng, blobs=blobs, ids=ids)
        assert eng.blob_ids() == ids
    return _FLEET["eng"], _FLEET["blobs"], _FLEET["ids"]


def _check_novel(eng, blobs, cache, lo=0, hi=None):
    """The raw and the listed result of [lo, hi) against gitid.summary_novel over all documents; returns the
    reference rows of the range."""
    from fluidframework_amd.gitid import summary_novel

    hi = len(blobs) if hi is None else hi
    want = summary_novel(cache, blobs)[lo:hi]
    flat = [x for doc in want for x in doc]
    buf, state, rep, off, first = eng.summary_novel_raw(lo, hi)
    assert first.tolist() == np.concatenate([[0], np.cumsum([len(d) for d in want])]).tolist()
    assert state.tolist() == [s for _, s, _, _ in flat]
    assert rep.tolist() == [r for _, _, r, _ in flat]
    assert off[0] == 0 and np.array_equal(np.diff(off), [len(b) if b is not None else 0 for _, _, _, b in flat])
    assert buf[:off[-1]].tobytes() == b"".join(b for _, _, _, b in flat if b is not None)
    nb, nf, nbytes = eng.summary_novel_info(lo, hi)
    assert (nb, nf, nbytes) == (len(flat), int((state == FIRST).sum()), int(off[-1]))
    assert eng.summary_novel(lo, hi) == want
    return want


@pytest.mark.gpu
def test_identical_documents():
    eng, blobs, ids = _fleet()
    eng.blob_cache_clear()
    flat_ids = [i for doc in ids for i in doc]
    flat_blobs = [b for doc in blobs for b in doc]
    distinct = {}
    for k, i in enumerate(flat_ids):
        distinct.setdefault(i, k)
    assert len(distinct) < len(flat_ids) // 10, "the fleet's blobs are not mostly equal"
    buf, state, rep, off, first = eng.summary_novel_raw()
    # exactly one blob per distinct id has state 1, the one at the smallest index, and its bytes are the blob
    assert np.flatnonzero(state == FIRST).tolist() == sorted(distinct.values())
    for i, k in distinct.items():
        assert buf[off[k]:off[k + 1]].tobytes() == flat_blobs[k] and _id(flat_blobs[k]) == i
    # all others repeat it
    for k, i in enumerate(flat_ids):
        assert rep[k] == distinct[i] and state[k] == (FIRST if distinct[i] == k else REPEAT), k
    assert eng.summary_novel_info() == (len(flat_ids), len(distinct), sum(len(flat_blobs[k]) for k in distinct.values()))
    _check_novel(eng, blobs, None)
    assert eng.timing()["novel_ms"] > 0
    # storage acknowledged
    eng.blob_cache_add_summary()
    assert eng.blob_cache_size() == len(distinct)
    assert eng.blob_cache_has(sorted(distinct)).all()
    buf, state, rep, off, first = eng.summary_novel_raw()
    assert not state.any() and (rep == -1).all() and not off.any()
    assert eng.summary_novel_info() == (len(flat_ids), 0, 0)
    _check_novel(eng, blobs, set(distinct))


def _half(ids, seed):
    distinct = sorted({i for doc in ids for i in doc})
    rng = np.random.default_rng(seed)
    return [distinct[k] for k in sorted(rng.choice(len(distinct), len(distinct) // 2, replace=False))]


@pytest.mark.gpu
def test_partial_cache():
    eng, blobs, ids = _fleet()
    cache = _half(ids, 0x5eed)
    eng.blob_cache_clear()
    eng.blob_cache_add(cache)
    assert eng.blob_cache_size() == len(cache)
    want = _check_novel(eng, blobs, cache)
    states = {s for doc in want for _, s, _, _ in doc}
    assert states == {HELD, FIRST, REPEAT}


@pytest.mark.gpu
def test_ranges():
    eng, blobs, ids = _fleet()
    cache = _half(ids, 0xa11)
    eng.blob_cache_clear()
    eng.blob_cache_add(cache)
    n = _N
    buf, state, rep, off, first = eng.summary_novel_raw(0, n)
    b, s, r, o, fi = eng.summary_novel_raw(0, 0)
    assert len(s) == 0 and len(r) == 0 and o.tolist() == [0] and fi.tolist() == [0]
    assert eng.summary_novel(0, 0) == [] and eng.summary_novel_info(0, 0) == (0, 0, 0)
    for lo, hi in ((0, 1), (40, 90), (0, n)):
        _check_novel(eng, blobs, cache, lo, hi)
    # a range behind the first occurrences: its repeats point before it and bring no bytes
    want = _check_novel(eng, blobs, cache, 2, 17)
    assert not any(s == FIRST for doc in want for _, s, _, _ in doc)
    assert any(s == REPEAT and r < int(first[2]) for doc in want for _, s, r, _ in doc)
    assert eng.summary_novel_info(2, 17)[1:] == (0, 0)
    # the pieces of a partition, put together, are the whole
    cuts = [0, 1, 17, 18, 64, 101, n]
    parts = [eng.summary_novel_raw(a, z) for a, z in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), state)
    assert np.array_equal(np.concatenate([p[2] for p in parts]), rep)
    assert b"".join(p[0][:p[3][-1]].tobytes() for p in parts) == buf[:off[-1]].tobytes()
    assert sum((eng.summary_novel(a, z) for a, z in zip(cuts, cuts[1:])), []) == eng.summary_novel(0, n)


@pytest.mark.gpu
def test_too_small_buffers():
    from fluidframework_amd.engine import lib

    eng, blobs, ids = _fleet()
    eng.blob_cache_clear()
    lo, hi = 0, 20
    nb, nf, nbytes = eng.summary_novel_info(lo, hi)
    assert 0 < nf < nb and nbytes > 0

    def buffers():
        return (np.full(nbytes + 16, 0xa5, dtype="u1"), np.full(nb + 1, 0xa5, dtype="u1"),
                np.full(nb + 1, -7, dtype="<i8"), np.full(nb + 2, -7, dtype="<i8"), np.full(hi - lo + 1, -7, dtype="<i8"))

    for cap_bytes, cap_blobs in ((nbytes - 1, nb), (nbytes, nb - 1)):
        out, st, rp, bo, df = buffers()
        r = lib().mtr_summary_novel(eng.h, lo, hi, out.ctypes.data, cap_bytes, st.ctypes.data, rp.ctypes.data,
                                    bo.ctypes.data, cap_blobs, df.ctypes.data)
        assert r == TOO_SMALL
        assert (out == 0xa5).all() and (st == 0xa5).all() and (rp == -7).all() and (bo == -7).all() and (df == -7).all()
    out, st, rp, bo, df = buffers()
    r = lib().mtr_summary_novel(eng.h, lo, hi, out.ctypes.data, nbytes, st.ctypes.data, rp.ctypes.data, bo.ctypes.data,
                                nb, df.ctypes.data)
    assert r == nbytes and (out[nbytes:] == 0xa5).all() and st[nb] == 0xa5 and rp[nb] == -7 and bo[nb + 1] == -7
    assert lib().mtr_summary_novel(eng.h, 5, 3, None, 0, None, None, bo.ctypes.data, 0, None) == -1
    assert lib().mtr_summary_novel(eng.h, 0, _N + 1, None, 0, None, None, bo.ctypes.data, 0, None) == -1


@pytest.mark.gpu
def test_invalidation_and_independence():
    from fluidframework_amd.engine import EngineError

    n = _N
    eng = _engine(n, chunk_size=8)
    with pytest.raises(EngineError, match="mtr_summarize"):
        eng.summary_novel()
    with pytest.raises(EngineError, match="mtr_summarize"):
        eng.blob_cache_add_summary()
    eng.apply(_fleet_batch())
    eng.summarize()
    blobs = _record_blobs(eng, n)
    ids = [[_id(b) for b in doc] for doc in blobs]
    eng.set_baseline([[i for i in doc[:2]] for doc in ids[:100]])

    def others():
        return eng.summary_delta(0, n), eng.blob_ids(0, n), eng.tree_ids(0, n)

    before = others()
    assert any(b is None for doc in before[0] for _, b in doc) and any(b is not None for doc in before[0] for _, b in doc)
    # the novel result follows every change of the set; the delta, the ids and the tree ids do not notice
    _check_novel(eng, blobs, None)
    cache = _half(ids, 0x1d)
    eng.blob_cache_add(cache)
    _check_novel(eng, blobs, cache)
    eng.blob_cache_add(cache)  # (nothing new)
    _check_novel(eng, blobs, cache)
    assert others() == before
    rest = sorted({i for doc in ids for i in doc} - set(cache))
    eng.blob_cache_add(rest[:1])
    _check_novel(eng, blobs, cache + rest[:1])
    eng.blob_cache_clear()
    _check_novel(eng, blobs, None)
    eng.blob_cache_add_summary()
    _check_novel(eng, blobs, {i for doc in ids for i in doc})
    assert others() == before
    # the cache survives reset + resubmit + summarize: the same documents come back all held
    eng.reset()
    with pytest.raises(EngineError):
        eng.summary_novel()
    held = eng.blob_cache_size()
    assert held == len({i for doc in ids for i in doc})
    eng.apply(_fleet_batch())
    eng.summarize()
    assert _record_blobs(eng, n) == blobs
    assert eng.summary_novel_info() == (sum(len(d) for d in ids), 0, 0)
    # changed documents: their new blobs reappear, once each
    changed = (3, 17, 90)
    eng.reset()
    eng.apply(_fleet_batch(shorter=changed))
    eng.summarize()
    blobs2 = _record_blobs(eng, n)
    assert [d for d in range(n) if blobs2[d] != blobs[d]] == list(changed)
    want = _check_novel(eng, blobs2, {i for doc in ids for i in doc})
    assert eng.blob_cache_size() == held
    for d in range(n):
        assert any(s != HELD for _, s, _, _ in want[d]) == (d in changed), d
    assert want[3][0][1] == FIRST and want[90][0][1] == REPEAT and want[90][0][2] == sum(len(doc) for doc in blobs2[:3])
    assert eng.summary_delta(0, n) != before[0]  # (the baseline is still there and sees the change its own way)
    eng.close()


@pytest.mark.gpu
def test_lifetime():
    from fluidframework_amd.engine import live_bytes

    gc.collect()
    start = live_bytes()
    eng = _engine(_N, chunk_size=8)
    eng.apply(_fleet_batch())
    eng.summarize()
    eng.blob_cache_add(_random_ids(np.random.default_rng(7), 3000))
    mid = live_bytes()
    assert mid > start
    assert eng.summary_novel_info()[1] > 0
    eng.blob_cache_add_summary()
    assert eng.summary_novel_info()[1] == 0
    assert live_bytes() > mid
    eng.close()
    assert live_bytes() == start
