"""The incremental summary hand-over (mtr_summary_delta): only the blobs whose git id is new or differs from a baseline
come back, gathered on the device into one compact buffer.

The reference everywhere is hashlib (gitid.git_blob_id) over the blobs of eng.summary(d) / eng.summaries(): a blob is
changed exactly when its id is absent at that (document, index) of the baseline, and a changed blob's bytes in the
delta equal the blob.  Everything is exact.
"""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_SMALL = -3  # include/mtr.h: MTR_SUMMARY_TOO_SMALL


# ---------------------------------------------------------------- CPU
def _ids(blobs):
    from fluidframework_amd.gitid import git_blob_id

    return [[git_blob_id(b) for b in doc] for doc in blobs]


_BLOBS = [[b"header 0", b"body 0"], [b"header 1"], [b"header 2", b"", b"body 2 b"]]


def test_host_definition_no_baseline():
    from fluidframework_amd.gitid import summary_delta

    ids = _ids(_BLOBS)
    got = summary_delta(None, _BLOBS)
    assert got == [[(i, b) for i, b in zip(di, db)] for di, db in zip(ids, _BLOBS)]
    assert summary_delta(None, []) == []


def test_host_definition_identical_baseline():
    from fluidframework_amd.gitid import summary_delta

    ids = _ids(_BLOBS)
    assert summary_delta(ids, _BLOBS) == [[(i, None) for i in di] for di in ids]


def test_host_definition_one_id_altered():
    from fluidframework_amd.gitid import summary_delta

    ids = _ids(_BLOBS)
    base = [list(d) for d in ids]
    base[2][1] = "0" * 40
    got = summary_delta(base, _BLOBS)
    assert got[0] == [(i, None) for i in ids[0]] and got[1] == [(ids[1][0], None)]
    assert got[2] == [(ids[2][0], None), (ids[2][1], b""), (ids[2][2], None)]


def test_host_definition_baseline_blob_counts():
    from fluidframework_amd.gitid import summary_delta

    ids = _ids(_BLOBS)
    fewer = [ids[0][:1], ids[1], ids[2]]
    got = summary_delta(fewer, _BLOBS)
    assert got[0] == [(ids[0][0], None), (ids[0][1], b"body 0")] and got[2] == [(i, None) for i in ids[2]]
    more = [ids[0], ids[1] + ["ab" * 20], ids[2]]
    assert summary_delta(more, _BLOBS) == [[(i, None) for i in di] for di in ids]
    # the same id at another index is not the same blob of the tree
    swapped = [ids[0][::-1], ids[1], ids[2]]
    assert [b for _, b in summary_delta(swapped, _BLOBS)[0]] == _BLOBS[0]


def test_host_definition_baseline_document_counts():
    from fluidframework_amd.gitid import summary_delta

    ids = _ids(_BLOBS)
    got = summary_delta(ids[:2], _BLOBS)
    assert got[:2] == [[(i, None) for i in di] for di in ids[:2]]
    assert got[2] == list(zip(ids[2], _BLOBS[2]))
    assert summary_delta(ids + [["cd" * 20]], _BLOBS) == [[(i, None) for i in di] for di in ids]


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mtr.h")).read()
    names = set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", text))
    assert {"mtr_summary_set_baseline", "mtr_summary_set_baseline_ids", "mtr_summary_clear_baseline",
            "mtr_summary_delta_info", "mtr_summary_delta"} <= names


def test_gather_kernel_uses_no_scratch():
    from fluidframework_amd import build

    build.build_engine()
    res = json.load(open(os.path.join(ROOT, "fluidframework_amd", "build", "kernel_resources.json")))
    ks = {k: v for k, v in res.items() if "delta_gather_kernel" in k}
    assert ks, "no resource entry for the gather kernel"
    for k, v in ks.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["VGPRs Spill"] == 0, (k, v)
    # the build's own check refuses such a kernel
    bad = {"_ZN3mtr19delta_gather_kernelEPKhPKmS3_jmjPh": {"ScratchSize [bytes/lane]": 16, "VGPRs Spill": 1}}
    with pytest.raises(RuntimeError, match="delta gather kernel"):
        build.check_delta_gather_no_scratch(bad)
    assert not build.check_delta_gather_no_scratch(
        {"_ZN3mtr19delta_gather_kernelEPKhPKmS3_jmjPh": {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0}})


# ---------------------------------------------------------------- GPU
def _engine(n_docs, **kw):
    from fluidframework_amd.engine import Engine
    caps = dict(max_segments=8192, heap_entries=8192, text_units=1 << 18, prop_words=1 << 18, remover_cells=1 << 14)
    caps.update(kw)
    return Engine(n_docs, **caps)


def _synthetic(n, ops, seed, **kw):
    from fluidframework_amd.synth import make_cfg, tables

    cfg = make_cfg(n, ops, writers=8, max_lag=32, seed=seed)
    caps = dict(max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=2 * int(cfg.text_cap) + 1024,
                prop_words=16384, remover_cells=4096, ops_per_launch=48)
    caps.update(kw)
    eng = _engine(n, **caps)
    eng.generate(cfg, tables(writers=8))
    return eng


def msg(seq, ref, client, contents, msn=0):
    return {"sequenceNumber": seq, "referenceSequenceNumber": ref, "clientId": client, "contents": contents,
            "minimumSequenceNumber": msn, "type": "op"}


def _alter(hex_id, byte=0):
    raw = bytearray(bytes.fromhex(hex_id))
    raw[byte % 20] ^= 0x5a
    return raw.hex()


def _check_delta(eng, blobs, baseline, lo=0, hi=None):
    """The raw and the listed delta of [lo, hi) against gitid.summary_delta over the same inputs; returns the
    reference."""
    from fluidframework_amd.gitid import summary_delta

    hi = len(blobs) if hi is None else hi
    want = summary_delta(baseline, blobs)[lo:hi]
    flat = [x for doc in want for x in doc]
    buf, flags, off, first = eng.summary_delta_raw(lo, hi)
    assert first.tolist() == np.concatenate([[0], np.cumsum([len(d) for d in want])]).tolist()
    assert flags.tolist() == [int(b is not None) for _, b in flat]
    assert off[0] == 0 and np.array_equal(np.diff(off), [len(b) if b is not None else 0 for _, b in flat])
    assert buf[:off[-1]].tobytes() == b"".join(b for _, b in flat if b is not None)
    nb, nc, nbytes = eng.summary_delta_info(lo, hi)
    assert (nb, nc, nbytes) == (len(flat), int(flags.sum()), int(off[-1]))
    assert eng.summary_delta(lo, hi) == want
    return want


_MANY = {}


def _many():
    """64 documents x 200 ops with 64-unit chunks (many blobs a document): the engine, its blobs and their ids, made
    once and left unchanged (tests set their own baseline first)."""
    if not _MANY:
        n = 64
        eng = _synthetic(n, 200, 0xb10b, chunk_size=64)
        eng.summarize()
        blobs = [eng.summary(d) for d in range(n)]
        _MANY.update(eng=eng, n=n, blobs=blobs, ids=_ids(blobs))
        assert eng.blob_ids() == _MANY["ids"]
    return _MANY["eng"], _MANY["n"], _MANY["blobs"], _MANY["ids"]


@pytest.mark.gpu
def test_no_baseline_everything_changed():
    eng, n, blobs, ids = _many()
    eng.clear_baseline()
    buf, flags, off, first = eng.summary_delta_raw()
    raw_ids, raw_first = eng.blob_ids_raw(0, n)
    assert np.array_equal(first, raw_first) and len(flags) == len(raw_ids) == len(off) - 1
    assert flags.all()
    flat = [b for doc in blobs for b in doc]
    assert np.array_equal(np.diff(off), [len(b) for b in flat])
    assert buf[:off[-1]].tobytes() == b"".join(flat)
    _check_delta(eng, blobs, None)


@pytest.mark.gpu
def test_identical_baseline_nothing_changed():
    eng, n, blobs, ids = _many()
    eng.set_baseline()
    buf, flags, off, first = eng.summary_delta_raw()
    total = sum(len(d) for d in ids)
    assert len(flags) == total and not flags.any() and not off.any()
    assert eng.summary_delta_info() == (total, 0, 0)
    assert eng.summary_delta() == [[(i, None) for i in d] for d in ids]
    assert eng.blob_ids() == ids  # (the current ids stay valid)


def _mixed_baseline(ids, seed):
    rng = np.random.default_rng(seed)
    base = [[_alter(x, int(rng.integers(20))) if rng.random() < 0.5 else x for x in d] for d in ids]
    for d in (3, 17, 40):
        base[d] = base[d][:len(base[d]) // 2]
    for d in (5, 29):
        base[d] = base[d] + ["ab" * 20]
    return base[:-5]


@pytest.mark.gpu
def test_host_baseline_with_a_controlled_mix():
    from fluidframework_amd.gitid import summary_delta

    eng, n, blobs, ids = _many()
    base = _mixed_baseline(ids, 0x5eed)
    # input conditions, on the host reference
    want = summary_delta(base, blobs)
    flat = [b for doc in want for _, b in doc]
    assert any(b is None for b in flat) and any(b is not None for b in flat)
    assert any(any(doc[k][1] is None and doc[k + 1][1] is not None for k in range(len(doc) - 1)) and
               any(doc[k][1] is not None and doc[k + 1][1] is None for k in range(len(doc) - 1)) for doc in want), \
        "no document with changed and unchanged blobs interleaved"
    recs, doc_off = eng.summaries(0, n)
    src, dst, pos = set(), set(), 0
    for d, doc in enumerate(want):
        s = int(doc_off[d]) + 4 + 4 * len(doc)  # the record: u32 nb, nb u32 lengths, the blobs
        for k, (_, b) in enumerate(doc):
            if b is not None:
                src.add(s % 4)
                dst.add(pos % 16)
                pos += len(b)
            s += len(blobs[d][k])
    assert src == {0, 1, 2, 3}, f"changed blobs start at source alignments {sorted(src)} only"
    assert len(dst) >= 8, f"changed blobs start at {len(dst)} destination alignments mod 16 only"
    eng.set_baseline(base)
    assert _check_delta(eng, blobs, base) == want
    # the same baseline in blob_ids_raw's layout
    first = np.concatenate([[0], np.cumsum([len(d) for d in base])]).astype("<i8")
    raw = np.frombuffer(bytes.fromhex("".join(x for d in base for x in d)), dtype="u1").reshape(-1, 20)
    eng.clear_baseline()
    eng.set_baseline((raw, first))
    _check_delta(eng, blobs, base)


@pytest.mark.gpu
def test_bad_host_baselines_are_refused():
    from fluidframework_amd.engine import EngineError, lib

    eng = _engine(1)
    ids = np.zeros((2, 20), dtype="u1")
    for first in ([1, 2], [0, 2, 1]):
        f = np.array(first, dtype="<i8")
        assert lib().mtr_summary_set_baseline_ids(eng.h, ids.ctypes.data, f.ctypes.data, len(first) - 1) == -1
    with pytest.raises(EngineError):
        eng.set_baseline()  # (no summary)
    with pytest.raises(EngineError, match="mtr_summarize"):
        eng.summary_delta()


@pytest.mark.gpu
def test_tile_boundaries_and_a_long_blob():
    from fluidframework_amd.batch import DocLog, Interner, build_batch
    from fluidframework_amd.engine import lib

    n, long_doc = 6, 2
    it = Interner()
    logs = [DocLog() for _ in range(n)]
    for d, log in enumerate(logs):
        log.start_collab("observer")
        if d == long_doc:
            for k in range(20):
                log.message(msg(k + 1, k, "A", {"type": 0, "pos1": 0, "seg": chr(97 + k) * 10000}), it)
        else:
            for k in range(1 + d % 3):
                log.message(msg(k + 1, k, "A", {"type": 0, "pos1": 0, "seg": "short insert %d.%d " % (d, k)}), it)
    eng = _engine(n, chunk_size=1 << 20, text_units=1 << 19)
    eng.apply(build_batch(logs, it))
    assert eng.stats()["bad_docs"] == 0
    eng.summarize()
    blobs = [eng.summary(d) for d in range(n)]
    ids = _ids(blobs)
    assert max(len(b) for b in blobs[long_doc]) > 200000
    # the long document's blobs and the blobs of alternate small documents are changed
    base = [[_alter(x) for x in doc] if d == long_doc or d % 2 == 1 else list(doc) for d, doc in enumerate(ids)]
    eng.set_baseline(base)
    want = _check_delta(eng, blobs, base)
    total = sum(len(b) for doc in want for _, b in doc if b is not None)
    nb = sum(len(d) for d in ids)
    out = np.full(total + 4096, 0xa5, dtype="u1")
    flags, off, first = np.zeros(nb, dtype="u1"), np.zeros(nb + 1, dtype="<i8"), np.zeros(n + 1, dtype="<i8")
    r = lib().mtr_summary_delta(eng.h, 0, n, out.ctypes.data, out.size, flags.ctypes.data, off.ctypes.data, nb,
                                first.ctypes.data)
    assert r == total
    assert out[:total].tobytes() == b"".join(b for doc in want for _, b in doc if b is not None)
    assert (out[total:] == 0xa5).all(), "the output buffer was written past the returned total"


@pytest.mark.gpu
def test_an_incremental_round():
    from fluidframework_amd.batch import DocLog, Interner, build_batch
    from fluidframework_amd.engine import EngineError

    n = 8
    changed = (1, 4, 6)

    def start():
        it = Interner()
        logs = [DocLog() for _ in range(n)]
        for d, log in enumerate(logs):
            log.start_collab("observer")
            log.message(msg(1, 0, "A", {"type": 0, "pos1": 0, "seg": "document %d " % d * 9}), it)
        return it, logs

    def append(it, logs):
        for d in changed:
            logs[d].message(msg(2, 1, "B", {"type": 0, "pos1": 3, "seg": "more text"}), it)

    it, logs = start()
    eng = _engine(n)
    eng.apply(build_batch(logs, it))
    eng.summarize()
    first = [eng.summary(d) for d in range(n)]
    eng.set_baseline()
    append(it, logs)
    eng.apply(build_batch(logs, it))
    with pytest.raises(EngineError, match="mtr_summarize"):
        eng.summary_delta()  # (the batch cleared the summary)
    eng.summarize()
    second = [eng.summary(d) for d in range(n)]
    want = _check_delta(eng, second, _ids(first))
    for d in range(n):
        assert any(b is not None for _, b in want[d]) == (d in changed), d
    # the baseline survives reset: both rounds replayed from the start answer against it as before
    eng.reset()
    with pytest.raises(EngineError):
        eng.summary_delta()
    it, logs = start()
    append(it, logs)
    eng.apply(build_batch(logs, it))
    eng.summarize()
    assert [eng.summary(d) for d in range(n)] == second
    assert _check_delta(eng, second, _ids(first)) == want
    eng.clear_baseline()
    got = _check_delta(eng, second, None)
    assert all(b is not None for doc in got for _, b in doc)


@pytest.mark.gpu
def test_ranges_and_capacities():
    from fluidframework_amd.engine import lib

    eng, n, blobs, ids = _many()
    base = _mixed_baseline(ids, 0x5eed)
    eng.set_baseline(base)
    buf, flags, off, first = eng.summary_delta_raw()
    for lo, hi in ((0, 1), (3, 11), (17, 18), (40, 64), (58, 61)):
        b, f, o, fi = eng.summary_delta_raw(lo, hi)
        b0, b1 = int(first[lo]), int(first[hi])
        assert np.array_equal(fi, first[lo:hi + 1] - b0)
        assert np.array_equal(f, flags[b0:b1])
        assert np.array_equal(o, off[b0:b1 + 1] - off[b0])
        assert b[:o[-1]].tobytes() == buf[off[b0]:off[b1]].tobytes()
        _check_delta(eng, blobs, base, lo, hi)
    b, f, o, fi = eng.summary_delta_raw(2, 2)
    assert len(f) == 0 and o.tolist() == [0] and fi.tolist() == [0]
    assert eng.summary_delta(2, 2) == [] and eng.summary_delta_info(2, 2) == (0, 0, 0)
    # one short in bytes, one short in blobs: refused with nothing written
    lo, hi = 3, 11
    nb, nc, nbytes = eng.summary_delta_info(lo, hi)
    assert 0 < nc < nb and nbytes > 0
    for cap_bytes, cap_blobs in ((nbytes - 1, nb), (nbytes, nb - 1)):
        out = np.full(nbytes + 16, 0xa5, dtype="u1")
        fl = np.full(nb + 1, 0xa5, dtype="u1")
        bo = np.full(nb + 2, -1, dtype="<i8")
        df = np.full(hi - lo + 1, -1, dtype="<i8")
        r = lib().mtr_summary_delta(eng.h, lo, hi, out.ctypes.data, cap_bytes, fl.ctypes.data, bo.ctypes.data,
                                    cap_blobs, df.ctypes.data)
        assert r == TOO_SMALL
        assert (out == 0xa5).all() and (fl == 0xa5).all() and (bo == -1).all() and (df == -1).all()
    r = lib().mtr_summary_delta(eng.h, lo, hi, out.ctypes.data, nbytes, fl.ctypes.data, bo.ctypes.data, nb,
                                df.ctypes.data)
    assert r == nbytes and (out[nbytes:] == 0xa5).all() and fl[nb] == 0xa5 and bo[nb + 1] == -1
    assert lib().mtr_summary_delta(eng.h, 5, 3, None, 0, None, bo.ctypes.data, 0, None) == -1
    assert lib().mtr_summary_delta(eng.h, 0, n + 1, None, 0, None, bo.ctypes.data, 0, None) == -1


@pytest.mark.gpu
def test_delta_after_replay_pipelined(monkeypatch):
    from fluidframework_amd.engine import Engine, pinned

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    n = 600
    eng = _synthetic(n, 120, 0x9e1)
    hb = eng.download(0, n, pinned_memory=True)
    eng.reset()
    buf, off = eng.replay_pipelined(hb, pinned(64 << 20, "u1"), 4)
    assert eng.stats()["bad_docs"] == 0
    blobs = [Engine.split_record(buf, int(off[d]), int(off[d + 1])) for d in range(n)]
    ids = eng.blob_ids()
    assert ids == _ids(blobs)
    base = [[_alter(x) for x in doc] if d % 3 == 0 else doc for d, doc in enumerate(ids)]
    eng.set_baseline(base)
    want = _check_delta(eng, blobs, base)
    for d in range(n):
        assert all((b is not None) == (d % 3 == 0) for _, b in want[d])
    assert eng.timing()["delta_ms"] > 0


@pytest.mark.gpu
def test_matrix_pair_handle_tables_only():
    from fluidframework_amd.engine import Engine
    from fluidframework_amd.synth import make_cfg, tables

    ops = 300
    cfg = make_cfg(1, ops, writers=8, max_lag=16, weights=(12, 8, 80), max_text=4, max_range=3)  # (config C4's mix)
    eng = Engine(2, max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=1 << 15, prop_words=1024,
                 remover_cells=4096, ops_per_launch=64)
    eng.generate_matrix(cfg, tables(writers=8))  # matrix 0 = documents (0 rows, 1 cols)
    for d in (0, 1):
        assert eng.status(d)[0] == 0
    eng.summarize()
    blobs = [eng.summary(d) for d in (0, 1)]
    ids = eng.blob_ids()
    assert ids == _ids(blobs)
    base = [doc[:-1] + [_alter(doc[-1])] for doc in ids]
    eng.set_baseline(base)
    want = _check_delta(eng, blobs, base)
    for d in (0, 1):
        assert len(blobs[d]) >= 2 and blobs[d][-1].startswith(b"[") and blobs[d][-1].endswith(b"]")  # handleTable
        assert [b for _, b in want[d]] == [None] * (len(blobs[d]) - 1) + [blobs[d][-1]]
    assert eng.summary_delta_info() == (sum(len(b) for b in blobs), 2, sum(len(b[-1]) for b in blobs))
