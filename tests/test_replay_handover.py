"""mtr_replay_handover: the pipelined hand-over that downloads only the blobs storage lacks.

The call is defined by calls that exist: it writes what mtr_submit + mtr_run + mtr_summarize, mtr_summary_novel over
all documents and mtr_summary_blob_ids write.  So every case compares it, exactly, with those serial calls on the same
engine, and the duplicate-heavy cases also with gitid.summary_novel (hashlib ids and a dict) over the serial records.
Ranges of any size: MTR_PIPE_MIN_PART_DOCS=0 -- by default ranges under 3,000 documents take the serial calls inside.
"""
import gc
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELD, FIRST, REPEAT = 0, 1, 2
TOO_SMALL = "mtr_replay_handover: the output buffers hold"


# ---------------------------------------------------------------- CPU
def test_header_declares_the_call():
    src = open(os.path.join(ROOT, "include", "mtr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int64_t\s+mtr_replay_handover\s*\(([^)]*)\)", src)
    assert m, "include/mtr.h does not declare mtr_replay_handover"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["e", "b", "parts", "out", "cap_bytes", "ids", "state", "rep",
                                                        "blob_off", "cap_blobs", "doc_first"]


def test_range_kernels_use_no_scratch():
    """The range gather keeps a lane's 16 bytes in registers like the whole-summary gather, the range classify its five
    id words; the ranges are hashed by the blob id kernel itself, which stays without scratch.  The build refuses a
    range kernel with scratch by the same checks."""
    from fluidframework_amd import build

    build.build_engine()
    res = json.load(open(os.path.join(ROOT, "fluidframework_amd", "build", "kernel_resources.json")))
    for name, pattern, check, what in [
            ("delta_gather_range_kernel", build._DELTA_GATHER_KERNEL, build.check_delta_gather_no_scratch, "delta gather"),
            ("novel_classify_range_kernel", build._NOVEL_CLASSIFY_KERNEL, build.check_novel_classify_no_scratch,
             "novel classify"),
            ("git_blob_id_kernel", build._BLOB_ID_KERNEL, build.check_blob_id_no_scratch, "blob id")]:
        ks = {k: v for k, v in res.items() if name in k}
        assert ks, f"no resource entry for {name}"
        for k, v in ks.items():
            assert pattern.match(k), k
            assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
            assert v["VGPRs Spill"] == 0, (k, v)
        with pytest.raises(RuntimeError, match=what + " kernel"):
            check({next(iter(ks)): {"ScratchSize [bytes/lane]": 16, "VGPRs Spill": 1}})


def test_python_binding_has_the_call_and_the_timing_slots():
    from fluidframework_amd.engine import Engine

    assert callable(Engine.replay_handover)
    src = open(os.path.join(ROOT, "fluidframework_amd", "engine.py")).read()
    for key in ("handover_copied_bytes", "handover_ids_ms", "handover_novel_ms", "handover_ranges"):
        assert key in src


# ---------------------------------------------------------------- GPU
def _engine(n_docs, **kw):
    from fluidframework_amd.engine import Engine

    caps = dict(max_segments=4096, heap_entries=4096, text_units=1 << 16, prop_words=1 << 14, remover_cells=1 << 12)
    caps.update(kw)
    return Engine(n_docs, **caps)


def _id(b):
    from fluidframework_amd.gitid import git_blob_id

    return git_blob_id(b)


def _records(eng, n):
    from fluidframework_amd.engine import Engine

    buf, off = eng.summaries(0, n)
    return [Engine.split_record(buf, int(off[d]), int(off[d + 1])) for d in range(n)]


def _serial(eng, batch, n):
    """The serial calls on a reset engine: (bytes, state, rep, blob_off, doc_first, ids), the layout of a hand-over."""
    eng.reset()
    eng.submit(batch)
    eng.run()
    eng.summarize()
    assert eng.stats()["bad_docs"] == 0
    buf, state, rep, off, first = eng.summary_novel_raw()
    ids, first2 = eng.blob_ids_raw()
    assert np.array_equal(first, first2)
    return buf[:int(off[-1])].copy(), state, rep, off, first, ids


def _handover(eng, batch, n, parts, out=None, cap_blobs=None):
    from fluidframework_amd.engine import pinned

    eng.reset()
    if out is None:
        out = pinned(8 << 20, "u1")
    out[:] = 0xEE
    buf, state, rep, off, first, ids = eng.replay_handover(batch, out, parts, cap_blobs=cap_blobs)
    assert eng.stats()["bad_docs"] == 0
    # only novel bytes crossed: the bytes-copied slot is the returned first_bytes, exactly
    assert eng.timing()["handover_copied_bytes"] == float(off[-1])
    return buf[:int(off[-1])].copy(), state, rep, off, first, ids


def _same(got, want):
    for name, g, w in zip(("bytes", "state", "rep", "blob_off", "doc_first", "ids"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), name


def _rows(res):
    """A hand-over result as gitid.summary_novel's rows: per document [(id_hex, state, rep, bytes | None)]."""
    buf, state, rep, off, first, ids = res
    hexes = [row.tobytes().hex() for row in ids]
    return [[(hexes[k], int(state[k]), int(rep[k]), buf[off[k]:off[k + 1]].tobytes() if state[k] == FIRST else None)
             for k in range(int(first[d]), int(first[d + 1]))] for d in range(len(first) - 1)]


def _range_of_blob(first, n, parts, k):
    """The pipelined range (documents [n p / parts, n (p + 1) / parts)) that holds blob k."""
    doc = int(np.searchsorted(first, k, side="right")) - 1
    lo = [n * p // parts for p in range(parts + 1)]
    return int(np.searchsorted(lo, doc, side="right")) - 1


# ---- 1. duplicates across ranges: the replay-log fleet of tests/test_blob_cache.py, rebuilt here.  Its records pass
# the pipelined path's op scan (remote inserts, removes and annotates, a local insert before the collaboration starts),
# so the fleet itself is used, not a tiled synthetic batch.
_N = 136
_OTHER = {17: "len_8-clients_4", 40: "len_8-clients_8", 63: "len_8-clients_4", 88: "len_8-clients_8",
          101: "len_8-clients_4", 135: "len_8-clients_8"}
_FLEET = {}


def _fleet():
    """136 documents: the golden log len_8-clients_2 in 130 of them, two other logs in six more, interleaved; 8-unit
    chunks, so several body_k a document.  The engine, the batch, the serial records and their hashlib ids, made once."""
    if not _FLEET:
        from fixtures import load_replay, replay_files, replay_log

        from fluidframework_amd.batch import Interner, build_batch

        it = Interner()
        groups = {name: load_replay([p for p in replay_files() if name in p][0])
                  for name in ["len_8-clients_2"] + sorted(set(_OTHER.values()))}
        logs = []
        for d in range(_N):
            g = groups[_OTHER.get(d, "len_8-clients_2")]
            log = replay_log(g, it)
            for grp in g:
                for m in grp["msgs"]:
                    log.message(m, it)
            logs.append(log)
        batch = build_batch(logs, it)
        eng = _engine(_N, chunk_size=8)
        eng.blob_cache_clear()
        _serial(eng, batch, _N)
        blobs = _records(eng, _N)
        assert min(len(doc) for doc in blobs) >= 3, "documents without several body_k blobs"
        _FLEET.update(eng=eng, batch=batch, blobs=blobs, ids=[[_id(b) for b in doc] for doc in blobs])
    return _FLEET


@pytest.mark.gpu
@pytest.mark.parametrize("parts", [4, 7])
@pytest.mark.parametrize("cache", ["none", "half", "all"])
def test_duplicates_across_ranges(parts, cache, monkeypatch):
    from fluidframework_amd.gitid import summary_novel

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    f = _fleet()
    eng, batch = f["eng"], f["batch"]
    distinct = sorted({x for doc in f["ids"] for x in doc})
    rng = np.random.default_rng(0x5eed)
    held = {"none": [], "half": [distinct[i] for i in rng.permutation(len(distinct))[:len(distinct) // 2]],
            "all": distinct}[cache]
    eng.blob_cache_clear()
    eng.blob_cache_add(held)
    want = _serial(eng, batch, _N)
    got = _handover(eng, batch, _N, parts, cap_blobs=len(want[1]))
    # the ranges ran, so the bytes-copied equality in _handover counts the copies they issued
    assert eng.timing()["handover_ranges"] == 1 and eng.timing()["handover_ids_ms"] > 0
    _same(got, want)
    assert _rows(got) == summary_novel(set(held), f["blobs"])
    buf, state, rep, off, first, ids = got
    if cache == "all":
        assert not state.any() and off[-1] == 0
    else:
        # the case the carry and the kept id set exist for: a repeat whose first occurrence an earlier range produced
        across = [k for k in np.flatnonzero(state == REPEAT)
                  if _range_of_blob(first, _N, parts, int(rep[k])) < _range_of_blob(first, _N, parts, int(k))]
        assert across, "no repeat refers to an earlier range"
    # the cache is read, not changed
    assert eng.blob_cache_size() == len(held)


# ---- 2. mostly distinct blobs, uneven ranges and the serial fallback inside
_SYNTH = {}
_CAPS = {}  # per n: the capacities of _synthetic's engine, for a second engine that takes the same batch


def _synthetic(n, ops=200):
    """(engine, page-locked batch) of n recorded documents, made once per n."""
    if n not in _SYNTH:
        from fluidframework_amd.synth import make_cfg, tables

        cfg = make_cfg(n, ops, writers=4, max_lag=16, seed=0x4a0d + n)
        _CAPS[n] = dict(max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=2 * int(cfg.text_cap) + 1024,
                        prop_words=16384, remover_cells=4096, ops_per_launch=48)
        eng = _engine(n, **_CAPS[n])
        eng.generate(cfg, tables(writers=4))
        _SYNTH[n] = (eng, eng.download(0, n, pinned_memory=True))
    return _SYNTH[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n, parts, force", [(400, 4, True), (400, 16, True), (5, 16, True), (40, 1, True),
                                             (4000, 16, False)])
def test_equals_serial_calls(n, parts, force, monkeypatch):
    """Ranges that divide the documents evenly and not, fewer ranges than asked (5 documents, 16 parts), and the serial
    calls inside: parts = 1, and by default ranges under 3,000 documents."""
    from fluidframework_amd.engine import pinned

    if force:
        monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    else:
        monkeypatch.delenv("MTR_PIPE_MIN_PART_DOCS", raising=False)
    eng, hb = _synthetic(n)
    eng.blob_cache_clear()
    want = _serial(eng, hb, n)
    got = _handover(eng, hb, n, parts, out=pinned(want[0].size + 64, "u1"), cap_blobs=len(want[1]))
    _same(got, want)
    t = eng.timing()
    if force and parts > 1:  # the ranges ran: their passes were timed
        assert t["handover_ranges"] == 1 and t["handover_ids_ms"] > 0 and t["handover_novel_ms"] > 0
    else:  # the serial calls inside
        assert t["handover_ranges"] == 0 and t["handover_ids_ms"] == 0 and t["handover_novel_ms"] == 0


# ---- 3. a range that starts at an unaligned byte of the compact buffer, and a range without any new blob
@pytest.mark.gpu
def test_unaligned_range_starts_and_an_empty_range(monkeypatch):
    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    n, parts = 400, 4
    eng, hb = _synthetic(n)
    lo = [n * p // parts for p in range(parts + 1)]
    eng.blob_cache_clear()
    want = _serial(eng, hb, n)
    _, state, _, off, first, ids = want
    starts = [int(off[first[lo[p]]]) for p in range(1, parts)]  # the ranges' first chosen byte offsets
    assert any(s % 16 for s in starts), starts
    _same(_handover(eng, hb, n, parts, cap_blobs=len(want[1])), want)
    # the cache holds everything range 1 produces: no state-1 blob there, the ranges after it start where range 0 ended
    b0, b1 = int(first[lo[1]]), int(first[lo[2]])
    eng.blob_cache_add(ids[b0:b1])
    want = _serial(eng, hb, n)
    _, state, _, off, first, _ = want
    assert not (state[b0:b1] == FIRST).any() and off[b0] == off[b1]
    assert (state[:b0] == FIRST).any() and (state[b1:] == FIRST).any()
    _same(_handover(eng, hb, n, parts, cap_blobs=len(want[1])), want)


# ---- 4. the engine after the call is the engine after a summary whose ids and novel result are built
@pytest.mark.gpu
def test_engine_state_afterwards(monkeypatch):
    from fluidframework_amd.gitid import summary_tree_id

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    n, parts = 400, 4
    eng, hb = _synthetic(n)
    eng.blob_cache_clear()
    want = _serial(eng, hb, n)
    want_h = eng.hashes(n).copy()
    rec, rec_off = eng.summaries(0, n)
    rec = rec[:int(rec_off[-1])].copy()
    want_ids = eng.blob_ids()
    ids_ms = eng.timing()["blob_ids_ms"]
    assert ids_ms > 0
    blobs = _records(eng, n)
    _same(_handover(eng, hb, n, parts, cap_blobs=len(want[1])), want)
    for d in (0, n // 2, n - 1):
        again, again_off = eng.summaries(d, d + 1)
        assert np.array_equal(again[:int(again_off[-1])], rec[int(rec_off[d]):int(rec_off[d + 1])])
    assert np.array_equal(eng.hashes(n), want_h)
    assert eng.blob_ids() == want_ids
    assert eng.timing()["blob_ids_ms"] == ids_ms, "the ids were hashed again"
    assert eng.tree_ids() == [summary_tree_id(doc, True) for doc in blobs]
    # a range of the novel result only downloads
    lo, hi = 100, 300
    buf, state, rep, off, first = eng.summary_novel_raw(lo, hi)
    b0, b1 = int(want[4][lo]), int(want[4][hi])
    assert np.array_equal(state, want[1][b0:b1]) and np.array_equal(rep, want[2][b0:b1])
    assert np.array_equal(buf[:int(off[-1])], want[0][int(want[3][b0]):int(want[3][b1])])
    # storage has acknowledged: the same batch again has nothing to send
    eng.blob_cache_add_summary()
    buf, state, rep, off, first, ids = _handover(eng, hb, n, parts, cap_blobs=len(want[1]))
    assert len(state) == len(want[1]) and not state.any() and (rep == -1).all()
    assert buf.size == 0 and not off.any()
    assert eng.timing()["handover_copied_bytes"] == 0
    assert np.array_equal(ids, want[5]) and np.array_equal(first, want[4])


@pytest.mark.gpu
def test_records_outgrow_the_device_buffer(monkeypatch):
    """The cache holds every blob and the caller sized `out` for what is left: nothing.  The records then outgrow the
    device buffer sized from the caller's bounds on an engine that has none yet, and the call finishes with the serial
    calls itself; the next call finds the buffer grown and runs the ranges.  The same result both times."""
    from fluidframework_amd.engine import pinned

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    n, parts = 400, 4
    ref, hb = _synthetic(n)
    ref.blob_cache_clear()
    ids = _serial(ref, hb, n)[5]
    ref.blob_cache_add(ids)
    want = _serial(ref, hb, n)
    ref.blob_cache_clear()
    assert not want[1].any() and want[0].size == 0
    eng = _engine(n, **_CAPS[n])
    try:
        eng.blob_cache_add(ids)
        for ranges_ran in (False, True):
            _same(_handover(eng, hb, n, parts, out=pinned(64, "u1"), cap_blobs=len(ids)), want)
            assert (eng.timing()["handover_ids_ms"] > 0) == ranges_ran
            assert eng.timing()["handover_ranges"] == int(ranges_ran)
    finally:
        eng.close()


@pytest.mark.gpu
def test_refused_range_is_not_continued_by_the_serial_calls(monkeypatch):
    """A refused range in a run whose records also outgrow the device buffer (a fresh engine, the cache holding
    everything, a 64-byte `out`): the refused range was never applied, so the call must fail with the refusal and not
    finish with the serial calls."""
    from fluidframework_amd import abi
    from fluidframework_amd.engine import EngineError, pinned
    from fluidframework_amd.synth import tables, with_docs

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    n, parts = 400, 4
    ref, hb = _synthetic(n)
    ref.blob_cache_clear()
    want = _serial(ref, hb, n)
    ops_arr = hb.ops.copy()
    ops_arr["flags"][int(hb.docs["op_begin"][123]) + 7] |= abi.F_DELTA
    flagged = with_docs(tables(writers=4), hb.docs.copy(), ops_arr, hb.text)
    eng = _engine(n, **_CAPS[n])
    try:
        eng.blob_cache_add(want[5])
        with pytest.raises(EngineError, match="beyond remote ops"):
            eng.replay_handover(flagged, pinned(64, "u1"), parts, cap_blobs=len(want[1]))
        eng.blob_cache_clear()
        _same(_serial(eng, flagged, n), want)
    finally:
        eng.close()


# ---- 6. buffers too small
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["bytes", "blobs"])
@pytest.mark.parametrize("warm", [False, True])
def test_buffers_too_small(which, warm, monkeypatch):
    """warm: the engine's record buffer stands from an earlier summary, so the ranges run and the stage itself meets
    the bound; cold, the record buffer is sized from the same bounds."""
    from fluidframework_amd.engine import EngineError, pinned

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    n, parts = 400, 4
    ref, hb = _synthetic(n)
    ref.blob_cache_clear()
    want = _serial(ref, hb, n)
    eng = ref if warm else _engine(n, **_CAPS[n])
    nbytes, nblobs = want[0].size, len(want[1])
    eng.reset()
    with pytest.raises(EngineError, match=TOO_SMALL):
        if which == "bytes":
            eng.replay_handover(hb, pinned(nbytes * 2 // 3, "u1"), parts, cap_blobs=nblobs)
        else:
            eng.replay_handover(hb, pinned(nbytes + 64, "u1"), parts, cap_blobs=nblobs * 2 // 3)
    assert eng.stats()["bad_docs"] == 0
    eng.summarize()
    buf, state, rep, off, first = eng.summary_novel_raw()
    _same((buf[:int(off[-1])], state, rep, off, first), want[:5])
    if not warm:
        eng.close()


# ---- 7. a refused range
@pytest.mark.gpu
def test_refuses_records_beyond_remote_ops(monkeypatch):
    from fluidframework_amd import abi
    from fluidframework_amd.engine import EngineError, pinned
    from fluidframework_amd.synth import tables, with_docs

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    n = 400
    eng, hb = _synthetic(n)
    eng.blob_cache_clear()
    want = _serial(eng, hb, n)
    ops_arr = hb.ops.copy()
    ops_arr["flags"][int(hb.docs["op_begin"][123]) + 7] |= abi.F_DELTA
    flagged = with_docs(tables(writers=4), hb.docs.copy(), ops_arr, hb.text)
    eng.reset()
    with pytest.raises(EngineError, match="beyond remote ops"):
        eng.replay_handover(flagged, pinned(want[0].size + 64, "u1"), 4)
    _same(_serial(eng, flagged, n), want)


# ---- 8. lifetime
@pytest.mark.gpu
def test_engine_memory_is_returned(monkeypatch):
    from fluidframework_amd.engine import EngineError, live_bytes, pinned
    from fluidframework_amd.synth import make_cfg, tables

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    n, ops = 64, 32
    caps = dict(max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=1 << 12, prop_words=1 << 12,
                remover_cells=1 << 10, ops_per_launch=16)
    gc.collect()  # (engines an earlier test left to the collector go now, not in the middle of this one)
    out = pinned(4 << 20, "u1")
    tiny = pinned(64, "u1")
    before = live_bytes()
    eng = _engine(n, **caps)
    try:
        eng.generate(make_cfg(n, ops, writers=8, max_lag=16), tables(writers=8))
        hb = eng.download(0, n)
        eng.blob_cache_add([_id(b"held")])
        eng.reset()
        _, state, _, off, _, _ = eng.replay_handover(hb, out, 4)
        assert (state == FIRST).any() and off[-1] > 0 and live_bytes() > before
    finally:
        eng.close()
    assert live_bytes() == before
    eng = _engine(n, **caps)
    try:
        with pytest.raises(EngineError, match=TOO_SMALL):
            eng.replay_handover(hb, tiny, 4)
        eng.reset()
        with pytest.raises(EngineError, match=TOO_SMALL):  # (the ranges ran this time: the record buffer stands)
            eng.replay_handover(hb, out, 4, cap_blobs=8)
    finally:
        eng.close()
    assert live_bytes() == before
