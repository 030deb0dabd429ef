"""Git blob ids of the summary blobs, hashed on the device (mtr_summary_blob_ids / mtr_git_blob_ids).

The reference for every id is hashlib.sha1(b"blob %d\\0" % len(b) + b): ids are equal or they are wrong.
"""
import hashlib
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EMPTY_ID = "e69de29bb2d1d6434b8b29ae775ad8c2e48c5391"
HELLO_ID = "3b18e512dba79e4c8300dd08aeb37f8e728b8dad"


def _ref(b):
    return hashlib.sha1(b"blob %d\0" % len(b) + b).hexdigest()


# ---------------------------------------------------------------- CPU
def test_host_definition_known_answers():
    from fluidframework_amd.gitid import git_blob_id

    assert git_blob_id(b"") == EMPTY_ID
    assert git_blob_id(b"hello world\n") == HELLO_ID
    assert git_blob_id(bytearray(b"hello world\n")) == HELLO_ID


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mtr.h")).read()
    names = set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", text))
    assert {"mtr_summary_blob_ids", "mtr_git_blob_ids"} <= names
    assert re.search(r"#define\s+MTR_BLOB_ID_BYTES\s+20\b", text)


def test_id_kernel_uses_no_scratch():
    from fluidframework_amd import build

    build.build_engine()
    res = json.load(open(os.path.join(ROOT, "fluidframework_amd", "build", "kernel_resources.json")))
    ks = {k: v for k, v in res.items() if "git_blob_id_kernel" in k}
    assert ks, "no resource entry for the id kernel"
    for k, v in ks.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["VGPRs Spill"] == 0, (k, v)
    # the build's own check refuses such a kernel
    bad = {"_ZN3mtr18git_blob_id_kernelEPKhPKmPKjjPj": {"ScratchSize [bytes/lane]": 8, "VGPRs Spill": 2}}
    with pytest.raises(RuntimeError, match="blob id kernel"):
        build.check_blob_id_no_scratch(bad)


# ---------------------------------------------------------------- GPU
def _engine(n_docs, **kw):
    from fluidframework_amd.engine import Engine
    caps = dict(max_segments=8192, heap_entries=8192, text_units=1 << 18, prop_words=1 << 18, remover_cells=1 << 14)
    caps.update(kw)
    return Engine(n_docs, **caps)


_EDGE = {}


def _edge_set():
    """One buffer of seeded random bytes; blobs packed back to back from byte offset 1: lengths 0..200 (every start
    alignment, every residue of (prefix + len) % 64, prefix lengths 7, 8, 9), then lengths across more digit-count
    boundaries, three 64-byte constant blobs and the two known answers.  The reference ids are computed once."""
    if not _EDGE:
        lens = list(range(201)) + [999, 1000, 9999, 10000, 65535, 65536, 99999, 100000, 1000000] + [64, 64, 64, 0, 12]
        off = np.zeros(len(lens) + 1, dtype="<i8")
        off[0] = 1
        off[1:] = 1 + np.cumsum(lens)
        data = np.random.default_rng(0x91d).integers(0, 256, int(off[-1]), dtype=np.uint8)
        for k, fill in zip((-5, -4, -3), (0x00, 0xff, 0x80)):
            data[off[k - 1]:off[k]] = fill
        data[off[-2]:off[-1]] = np.frombuffer(b"hello world\n", dtype="u1")
        ref = [_ref(data[off[i]:off[i + 1]].tobytes()) for i in range(len(lens))]
        assert ref[-2] == EMPTY_ID and ref[-1] == HELLO_ID and ref[0] == EMPTY_ID
        data.setflags(write=False)
        _EDGE.update(data=data, off=off, ref=ref)
    return _EDGE["data"], _EDGE["off"], _EDGE["ref"]


@pytest.mark.gpu
def test_raw_ids_edge_lengths():
    data, off, ref = _edge_set()
    eng = _engine(1)
    got = eng.git_blob_ids_packed(data, off)
    bad = [(i, int(off[i + 1] - off[i])) for i in range(len(ref)) if got[i] != ref[i]]
    assert not bad, f"{len(bad)} ids differ, first (index, length): {bad[:8]}"
    assert eng.git_blob_ids([b"", b"hello world\n"]) == [EMPTY_ID, HELLO_ID]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_raw_ids_wave_tails(n):
    data, off, ref = _edge_set()
    eng = _engine(1)
    assert eng.git_blob_ids_packed(data, off[:n + 1]) == ref[:n]


def _check_engine_ids(eng, n, blobs_of=None):
    """blob_ids of every document against hashlib over its summary blobs; doc_first consistent."""
    blobs = [eng.summary(d) if blobs_of is None else blobs_of(d) for d in range(n)]
    want = [[_ref(b) for b in bl] for bl in blobs]
    ids, first = eng.blob_ids_raw(0, n)
    assert first[0] == 0 and first[-1] == len(ids) == sum(len(w) for w in want)
    assert np.array_equal(np.diff(first), [len(w) for w in want])
    assert eng.blob_ids() == want
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("v1", [True, False], ids=["v1", "legacy"])
def test_summary_ids_on_snapshot_fixtures(v1):
    from fixtures import SNAPSHOT_VERSIONS, load_snapshots, snapshot_log
    from fluidframework_amd.batch import Interner, build_batch

    snaps = load_snapshots()
    keys = sorted(k for k in snaps if SNAPSHOT_VERSIONS[k.split("/")[0]] == v1)
    it = Interner()
    logs = [snapshot_log(k.split("/")[1], it) for k in keys]
    b = build_batch(logs, it)
    n = len(keys)
    eng = _engine(n, snapshot_v1=v1, max_segments=16384, heap_entries=256)
    eng.apply(b)
    eng.summarize()
    want = _check_engine_ids(eng, n)
    # (withAnnotations / withMarkers are the multi-blob documents: header + body, or header + body_0..2)
    assert max(len(w) for w in want) == (4 if v1 else 2), "no multi-blob document among the fixtures"
    lo, hi = min(3, n), min(7, n)
    assert eng.blob_ids(lo, hi) == want[lo:hi]
    ids, first = eng.blob_ids_raw(lo, hi)
    assert first[0] == 0 and first[-1] == len(ids)
    assert eng.blob_ids(2, 2) == []
    ids, first = eng.blob_ids_raw(2, 2)
    assert len(ids) == 0 and first.tolist() == [0]


def _synthetic(n, ops, seed, **kw):
    from fluidframework_amd.synth import make_cfg, tables

    cfg = make_cfg(n, ops, writers=8, max_lag=32, seed=seed)
    caps = dict(max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=2 * int(cfg.text_cap) + 1024,
                prop_words=16384, remover_cells=4096, ops_per_launch=48)
    caps.update(kw)
    eng = _engine(n, **caps)
    eng.generate(cfg, tables(writers=8))
    return eng


@pytest.mark.gpu
def test_many_blobs_per_document_and_small_cap():
    import ctypes as C
    from fluidframework_amd.engine import lib

    n = 64
    eng = _synthetic(n, 200, 0xb10b, chunk_size=64)
    eng.summarize()
    want = _check_engine_ids(eng, n)
    total = sum(len(w) for w in want)
    assert sum(len(w) > 2 for w in want) > n // 2, "most documents should have several body blobs"
    out = np.full((total, 20), 0xa5, dtype="u1")
    first = np.zeros(n + 1, dtype="<i8")
    r = lib().mtr_summary_blob_ids(eng.h, 0, n, out.ctypes.data, total - 1, first.ctypes.data)
    assert r == -total
    assert (out == 0xa5).all(), "out written although cap_blobs was too small"
    r = lib().mtr_summary_blob_ids(eng.h, 0, n, out.ctypes.data, total, first.ctypes.data)
    assert r == total
    assert [row.tobytes().hex() for row in out] == [x for w in want for x in w]


@pytest.mark.gpu
def test_matrix_pair_ids_cover_the_handle_table():
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
    want = _check_engine_ids(eng, 2)
    for d in (0, 1):
        blobs = eng.summary(d)
        assert len(blobs) >= 2 and blobs[-1].startswith(b"[") and blobs[-1].endswith(b"]")  # handleTable
        assert want[d][-1] == _ref(blobs[-1])


@pytest.mark.gpu
def test_ids_after_replay_pipelined(monkeypatch):
    from fluidframework_amd.engine import Engine, pinned

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    n = 600
    eng = _synthetic(n, 120, 0x9e1)
    hb = eng.download(0, n, pinned_memory=True)
    eng.reset()
    buf, off = eng.replay_pipelined(hb, pinned(64 << 20, "u1"), 4)
    assert eng.stats()["bad_docs"] == 0
    _check_engine_ids(eng, n, lambda d: Engine.split_record(buf, int(off[d]), int(off[d + 1])))


@pytest.mark.gpu
def test_cache_validity():
    from fluidframework_amd.engine import EngineError
    from fluidframework_amd.batch import DocLog, Interner, build_batch

    def msg(seq, ref, client, contents, msn=0):
        return {"sequenceNumber": seq, "referenceSequenceNumber": ref, "clientId": client, "contents": contents,
                "minimumSequenceNumber": msn, "type": "op"}

    n = 8
    it = Interner()
    logs = [DocLog() for _ in range(n)]
    for d, log in enumerate(logs):
        log.start_collab("observer")
        log.message(msg(1, 0, "A", {"type": 0, "pos1": 0, "seg": "document %d " % d * 9}), it)
    eng = _engine(n)
    with pytest.raises(EngineError):
        eng.blob_ids()
    eng.apply(build_batch(logs, it))
    eng.summarize()
    first = _check_engine_ids(eng, n)
    assert eng.blob_ids() == first  # (answered from the device cache)
    changed = (1, 4, 6)
    for d in changed:
        logs[d].message(msg(2, 1, "B", {"type": 0, "pos1": 3, "seg": "more text"}), it)
    eng.apply(build_batch(logs, it))
    with pytest.raises(EngineError):
        eng.blob_ids()  # (the batch cleared the summary)
    eng.summarize()
    second = _check_engine_ids(eng, n)
    assert any(second[d] != first[d] for d in changed)
    eng.reset()
    with pytest.raises(EngineError):
        eng.blob_ids()
