"""Git tree ids of the summary trees, hashed on the device (mtr_summary_tree_ids / mtr_git_tree_ids).

The reference for every id is hashlib through fluidframework_amd.gitid (git_tree_id / summary_tree_id), itself checked
against known answers and, where git is installed, against `git mktree`: ids are equal or they are wrong.
"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EMPTY_TREE = "4b825dc642cb6eb9a060e54bf8d69288fbee4904"
FOURTEEN = "34a1300420dea44447816c075c1c52f67cd12f86"
VECTOR = "74b28af8fdfab570d63148c74cbea4bc0a433334"
BLOB, TREE = 0o100644, 0o40000


def _fourteen():
    from fluidframework_amd.gitid import git_blob_id

    names = ["header"] + [f"body_{k}" for k in range(12)] + ["catchupOps"]
    return [(BLOB, n, git_blob_id(n.encode())) for n in names]


def _vector():
    from fluidframework_amd.gitid import git_blob_id

    return [(TREE, "segments", FOURTEEN), (BLOB, "handleTable", git_blob_id(b"header"))]


def _abc():
    from fluidframework_amd.gitid import git_blob_id

    return [(BLOB, "a0", git_blob_id(b"a0")), (TREE, "a", EMPTY_TREE), (BLOB, "a.b", git_blob_id(b"a.b"))]


# ---------------------------------------------------------------- CPU
def test_host_definition_known_answers():
    from fluidframework_amd.gitid import git_blob_id, git_tree_id, summary_tree_id

    assert git_tree_id([]) == EMPTY_TREE
    assert git_tree_id(_fourteen()) == FOURTEEN
    assert git_tree_id(list(reversed(_fourteen()))) == FOURTEEN
    assert git_tree_id(_vector()) == VECTOR
    # the same trees through summary_tree_id: thirteen engine blobs and a host-made catchupOps; the vector's two levels
    blobs = [b"header"] + [b"body_%d" % k for k in range(12)]
    assert summary_tree_id(blobs, True, extras=[(BLOB, "catchupOps", git_blob_id(b"catchupOps"))]) == FOURTEEN
    assert summary_tree_id([b"x", b"y"], False) == git_tree_id([(BLOB, "header", git_blob_id(b"x")),
                                                                (BLOB, "body", git_blob_id(b"y"))])
    # (the vector's handleTable blob is b"header" in the known answer; its segments need the catch-up entry too)
    inner = git_tree_id([(BLOB, n, i) for _, n, i in _fourteen() if n != "catchupOps"])
    assert summary_tree_id(blobs + [b"header"], True, matrix=True) == git_tree_id(
        [(TREE, "segments", inner), (BLOB, "handleTable", git_blob_id(b"header"))])


def test_subtree_sorts_as_its_name_and_a_slash():
    from fluidframework_amd.gitid import git_tree_id
    import hashlib

    ents = {n: (m, i) for m, n, i in _abc()}
    body = b"".join(b"%o %s\0" % (ents[n][0], n.encode()) + bytes.fromhex(ents[n][1]) for n in ("a.b", "a", "a0"))
    assert b"40000 a\0" in body and b"040000" not in body
    assert git_tree_id(_abc()) == hashlib.sha1(b"tree %d\0" % len(body) + body).hexdigest()


@pytest.mark.parametrize("bad", [[(BLOB, "", EMPTY_TREE)], [(BLOB, "a/b", EMPTY_TREE)], [(BLOB, "a\0b", EMPTY_TREE)],
                                 [(BLOB, "a", EMPTY_TREE), (TREE, "a", EMPTY_TREE)]],
                         ids=["empty", "slash", "nul", "duplicate"])
def test_host_definition_rejects_bad_names(bad):
    from fluidframework_amd.gitid import git_tree_id, summary_tree_id

    with pytest.raises(ValueError):
        git_tree_id(bad)
    with pytest.raises(ValueError):
        summary_tree_id([b"x"], True, extras=bad)


def test_an_extra_may_not_repeat_an_engine_name():
    from fluidframework_amd.gitid import summary_tree_id

    with pytest.raises(ValueError):
        summary_tree_id([b"x", b"y"], True, extras=[(BLOB, "header", EMPTY_TREE)])
    with pytest.raises(ValueError):
        summary_tree_id([b"x", b"y"], True, extras=[(BLOB, "body_0", EMPTY_TREE)])
    summary_tree_id([b"x", b"y"], True, extras=[(BLOB, "body_1", EMPTY_TREE)])  # (no such chunk: the name is free)


def test_forty_byte_name_is_rejected_at_the_python_and_c_boundary():
    from fluidframework_amd import build
    from fluidframework_amd.engine import TREE_ENTRY, pack_tree_entries

    x, first = pack_tree_entries([[(BLOB, "n" * 39, EMPTY_TREE)]])
    assert x[0]["name_len"] == 39 and first.tolist() == [0, 1]
    with pytest.raises(ValueError, match="40 bytes"):
        pack_tree_entries([[(BLOB, "n" * 40, EMPTY_TREE)]])
    with pytest.raises(ValueError):
        pack_tree_entries([[(BLOB, "", EMPTY_TREE)]])
    # the C entry point validates before it touches the engine, so a null engine serves on a machine without a GPU
    lib = C.CDLL(build.build_engine())
    lib.mtr_git_tree_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.mtr_git_tree_ids.restype = C.c_int
    lib.mtr_last_error.restype = C.c_char_p
    out = np.full(20, 0xa5, dtype="u1")
    for name_len, name, what in ((40, b"n" * 39, b"name length 40"), (0, b"", b"name length 0"),
                                 (3, b"a/b", b"'/'"), (3, b"a\0b", b"NUL")):
        x = np.zeros(2, dtype=TREE_ENTRY)
        x[0] = (np.zeros(20, "u1"), BLOB, 1, b"ok")
        x[1] = (np.zeros(20, "u1"), BLOB, name_len, name)
        assert lib.mtr_git_tree_ids(None, x.ctypes.data, first_of(2).ctypes.data, 1, out.ctypes.data) == -1
        msg = lib.mtr_last_error()
        assert what in msg and b"tree 0, entry 1" in msg, msg
    x = np.zeros(2, dtype=TREE_ENTRY)
    x[0] = (np.zeros(20, "u1"), BLOB, 1, b"a")
    x[1] = (np.zeros(20, "u1"), TREE, 1, b"a")
    assert lib.mtr_git_tree_ids(None, x.ctypes.data, first_of(2).ctypes.data, 1, out.ctypes.data) == -1
    assert b"appears twice" in lib.mtr_last_error()
    assert (out == 0xa5).all()


def first_of(*counts):
    first = np.zeros(len(counts) + 1, dtype="<i8")
    np.cumsum(counts, out=first[1:])
    return first


@pytest.mark.skipif(shutil.which("git") is None, reason="git is not installed")
def test_host_definition_against_git_mktree(tmp_path):
    from fluidframework_amd.gitid import git_blob_id, git_tree_id

    env = dict(os.environ, GIT_CONFIG_NOSYSTEM="1", HOME=str(tmp_path), GIT_DIR=str(tmp_path / "repo.git"))

    def git(*args, data=b""):
        r = subprocess.run(["git"] + list(args), input=data, capture_output=True, env=env, cwd=tmp_path)
        assert r.returncode == 0, r.stderr.decode()
        return r.stdout.decode().strip()

    git("init", "--bare", "-q", str(tmp_path / "repo.git"))

    def mktree(entries):
        lines = []
        for mode, name, oid in entries:
            lines.append("%06o %s %s\t%s" % (mode, "tree" if mode == TREE else "blob", oid, name))
        return git("mktree", "--missing", data=("\n".join(lines) + "\n").encode() if lines else b"")

    for content in [b"header", b"catchupOps", b"a0", b"a.b"] + [b"body_%d" % k for k in range(12)]:
        assert git("hash-object", "-w", "--stdin", data=content) == git_blob_id(content)
    assert mktree([]) == EMPTY_TREE == git_tree_id([])
    assert mktree(_fourteen()) == FOURTEEN
    assert mktree(_vector()) == VECTOR
    assert mktree(_abc()) == git_tree_id(_abc())


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mtr.h")).read()
    names = set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", text))
    assert {"mtr_summary_tree_ids", "mtr_git_tree_ids"} <= names
    assert re.search(r"#define\s+MTR_TREE_NAME_MAX\s+39\b", text)
    from fluidframework_amd.engine import TREE_ENTRY

    assert TREE_ENTRY.itemsize == 64 and re.search(r"typedef struct mtr_tree_entry\s*\{\s*/\* 64 bytes \*/", text)


def test_tree_id_kernel_uses_no_scratch():
    from fluidframework_amd import build

    build.build_engine()
    res = json.load(open(os.path.join(ROOT, "fluidframework_amd", "build", "kernel_resources.json")))
    ks = {k: v for k, v in res.items() if "git_tree_id_kernel" in k}
    assert ks, "no resource entry for the tree id kernel"
    for k, v in ks.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["VGPRs Spill"] == 0, (k, v)
        assert build.check_tree_id_no_scratch({k: v}) == {}
    # the build's own check refuses a kernel with scratch, and looks at the kernel the build made
    for k in ks:
        with pytest.raises(RuntimeError, match="tree id kernel"):
            build.check_tree_id_no_scratch({k: {"ScratchSize [bytes/lane]": 8, "VGPRs Spill": 2}})
        assert build.check_tree_id_no_scratch({k: {"ScratchSize [bytes/lane]": 8, "VGPRs Spill": 0}}, strict=False)


# ---------------------------------------------------------------- GPU
def _engine(n_docs, **kw):
    from fluidframework_amd.engine import Engine
    caps = dict(max_segments=8192, heap_entries=8192, text_units=1 << 18, prop_words=1 << 18, remover_cells=1 << 14)
    caps.update(kw)
    return Engine(n_docs, **caps)


_EDGE = {}
_ALPHABET = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789._-~ +"


def _prefix_len(body_len):
    return len(b"tree %d\0" % body_len)


def _edge_set():
    """Host trees with seeded random ids and names, entries in shuffled order.  The first 65 trees (the wave-tail
    cases take prefixes of the set) hold the empty tree, the a.b / a / a0 case, every name length 1..39 in both modes
    and trees of 2, 3, 40 and 130 entries.  Then one-entry and two-entry blob trees whose name lengths are chosen so
    that (prefix + body) % 64 takes every value, and trees around the 9/10, 99/100 and 999/1000 body lengths.
    A blob entry of name length L takes 28 + L bytes, a subtree entry 27 + L.  The references are computed once."""
    if _EDGE:
        return _EDGE["trees"], _EDGE["ref"]
    from fluidframework_amd.gitid import git_tree_id

    rng = np.random.default_rng(0x7ee)

    def rid():
        return rng.integers(0, 256, 20, dtype=np.uint8).tobytes().hex()

    def name(length, taken):
        while True:
            s = "".join(_ALPHABET[i] for i in rng.integers(0, len(_ALPHABET), length))
            if s not in taken:
                taken.add(s)
                return s

    def tree(lengths, modes=None):
        taken = set()
        t = [((BLOB, TREE)[int(rng.integers(0, 2))] if modes is None else modes[k], name(L, taken), rid())
             for k, L in enumerate(lengths)]
        return [t[i] for i in rng.permutation(len(t))]

    trees = [[], [(BLOB, "a0", rid()), (TREE, "a", rid()), (BLOB, "a.b", rid())]]
    trees += [tree([L], [(BLOB, TREE)[L % 2]]) for L in range(1, 40)]              # 39 one-entry trees
    trees += [tree([L, 40 - L], [(TREE, BLOB)[L % 2], BLOB]) for L in range(1, 20)]  # 19 two-entry trees
    trees += [tree(rng.integers(1, 40, 3)), tree(rng.integers(1, 40, 40)), tree(rng.integers(1, 40, 130)),
              tree(rng.integers(1, 40, 130)), tree(rng.integers(1, 40, 40))]
    assert len(trees) == 65
    # body lengths 29..67 (one blob entry) and 58..134 (two): with the prefix, every residue mod 64
    trees += [tree([L], [BLOB]) for L in range(1, 40)]
    trees += [tree([a, b], [BLOB, BLOB]) for a in (1, 39) for b in range(1, 40)]
    # digit boundaries of the prefix: bodies of 99 / 100 (two and three entries), 999 / 1000 and one past them
    trees += [tree([39, 4], [BLOB, BLOB]), tree([39, 5], [BLOB, BLOB]), tree([39, 6], [BLOB, BLOB])]  # 99, 100, 101
    for want in (998, 999, 1000, 1001):  # 24 blob entries of names 13..14 bytes: 24 * 28 + sum(L) = want
        base = [(want - 24 * 28) // 24] * 24
        for k in range(want - 24 * 28 - sum(base)):
            base[k] += 1
        trees.append(tree(base, [BLOB] * 24))
    ref = [git_tree_id(t) for t in trees]
    _EDGE.update(trees=trees, ref=ref)
    return trees, ref


def _body_len(t):
    return sum((28 if m == BLOB else 27) + len(n.encode()) for m, n, _ in t)


@pytest.mark.gpu
def test_host_trees_edge_lengths():
    trees, ref = _edge_set()
    # the set covers what it claims before anything is compared
    sizes = [_body_len(t) for t in trees]
    assert {len(t) for t in trees} >= {0, 1, 2, 3, 40, 130}
    assert {len(n) for t in trees for _, n, _ in t} == set(range(1, 40))
    assert {(_prefix_len(s) + s) % 64 for s in sizes} == set(range(64))
    # both sides of the prefix's digit boundaries: 9 | 10 (an entry has at least 28 bytes, so the one-digit side is the
    # empty tree alone), 99 | 100, 999 | 1000
    assert {0, 29, 99, 100, 999, 1000} <= set(sizes)
    assert {m for t in trees for m, _, _ in t} == {BLOB, TREE}
    assert ref[0] == EMPTY_TREE
    eng = _engine(1)
    got = eng.git_tree_ids(trees)
    bad = [(i, len(trees[i]), sizes[i]) for i in range(len(ref)) if got[i] != ref[i]]
    assert not bad, f"{len(bad)} ids differ, first (index, entries, body length): {bad[:8]}"
    assert eng.git_tree_ids([_fourteen(), _vector(), []]) == [FOURTEEN, VECTOR, EMPTY_TREE]
    assert eng.timing()["tree_ids_ms"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_host_trees_wave_tails(n):
    trees, ref = _edge_set()
    assert _engine(1).git_tree_ids(trees[:n]) == ref[:n]


def _check_tree_ids(eng, n, v1, blobs_of=None, extras=None, matrix=False):
    from fluidframework_amd.gitid import summary_tree_id

    blobs = [eng.summary(d) if blobs_of is None else blobs_of(d) for d in range(n)]
    want = [summary_tree_id(blobs[d], v1, extras=extras[d] if extras else (), matrix=matrix) for d in range(n)]
    got = eng.tree_ids(0, n, extras)
    bad = [(d, len(blobs[d])) for d in range(n) if got[d] != want[d]]
    assert not bad, f"{len(bad)} of {n} tree ids differ, first (document, blobs): {bad[:8]}"
    return want, blobs


@pytest.mark.gpu
@pytest.mark.parametrize("v1", [True, False], ids=["v1", "legacy"])
def test_tree_ids_on_snapshot_fixtures(v1):
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
    want, blobs = _check_tree_ids(eng, n, v1)
    assert max(len(x) for x in blobs) == (4 if v1 else 2), "no multi-blob document among the fixtures"
    lo, hi = min(3, n), min(7, n)
    assert eng.tree_ids(lo, hi) == want[lo:hi]
    assert eng.tree_ids(2, 2) == []
    assert eng.tree_ids_raw(2, 2).shape == (0, 20)
    assert eng.tree_ids_raw(lo, hi).shape == (hi - lo, 20)


def _synthetic(n, ops, seed, **kw):
    from fluidframework_amd.synth import make_cfg, tables

    cfg = make_cfg(n, ops, writers=8, max_lag=32, seed=seed)
    caps = dict(max_segments=2 * ops + 128, heap_entries=2 * ops + 128, text_units=2 * int(cfg.text_cap) + 1024,
                prop_words=16384, remover_cells=4096, ops_per_launch=48)
    caps.update(kw)
    eng = _engine(n, **caps)
    eng.generate(cfg, tables(writers=8))
    return eng


_TWO_DIGIT = {}


def _two_digit_engine():
    """64 documents x 200 ops at chunk_size 16: 16..35 blobs each, so every tree holds body_10 ahead of body_2.
    Shared by the tests that only read it."""
    if not _TWO_DIGIT:
        eng = _synthetic(64, 200, 0xb10b, chunk_size=16)
        eng.summarize()
        _TWO_DIGIT.update(eng=eng, blobs=[eng.summary(d) for d in range(64)])
    return _TWO_DIGIT["eng"], _TWO_DIGIT["blobs"]


@pytest.mark.gpu
def test_two_digit_chunk_names():
    eng, blobs = _two_digit_engine()
    assert min(len(b) for b in blobs) >= 12, "every document should reach body_10"
    _check_tree_ids(eng, 64, True, blobs_of=lambda d: blobs[d])


@pytest.mark.gpu
def test_three_digit_chunk_names():
    n = 16
    eng = _synthetic(n, 400, 0xb10b, chunk_size=2)
    eng.summarize()
    ok = [d for d in range(n) if eng.status(d)[0] == 0]
    blobs = {d: eng.summary(d) for d in ok}
    assert any(len(b) >= 102 for b in blobs.values()), "no document reaches body_100"
    from fluidframework_amd.gitid import summary_tree_id

    got = eng.tree_ids(0, n)
    bad = [(d, len(blobs[d])) for d in ok if got[d] != summary_tree_id(blobs[d], True)]
    assert not bad, f"tree ids differ, (document, blobs): {bad[:8]}"
    assert ok == list(range(n)), f"documents with a non-OK status at chunk_size 2: {sorted(set(range(n)) - set(ok))}"


def _extras_for(blobs):
    from fluidframework_amd.gitid import git_blob_id

    return [[(BLOB, "catchupOps", git_blob_id(b"catch up %d" % d)), (BLOB, "attribution", git_blob_id(b"attr %d" % d)),
             (BLOB, "intervals", git_blob_id(b"intervals %d" % d)), (TREE, "body_1x", git_blob_id(bl[2]))]
            for d, bl in enumerate(blobs)]


@pytest.mark.gpu
def test_extras_are_merged_by_the_sort_rule():
    from fluidframework_amd.engine import EngineError, lib, pack_tree_entries

    eng, blobs = _two_digit_engine()
    extras = _extras_for(blobs)
    want, _ = _check_tree_ids(eng, 64, True, blobs_of=lambda d: blobs[d], extras=extras)
    assert want != _check_tree_ids(eng, 64, True, blobs_of=lambda d: blobs[d])[0]
    assert eng.tree_ids(5, 9, extras[5:9]) == want[5:9]
    for name in ("header", "body_3"):
        bad = [list(x) for x in extras]
        bad[37] = bad[37] + [(BLOB, name, EMPTY_TREE)]
        x, first = pack_tree_entries(bad)
        out = np.full((64, 20), 0xa5, dtype="u1")
        r = lib().mtr_summary_tree_ids(eng.h, 0, 64, x.ctypes.data, first.ctypes.data, out.ctypes.data)
        assert r == -1
        msg = lib().mtr_last_error().decode()
        assert "document 37" in msg and name in msg, msg
        assert (out == 0xa5).all(), "out written although the call failed"
        with pytest.raises(EngineError, match="document 37"):
            eng.tree_ids(0, 64, bad)
        assert eng.tree_ids(0, 64, extras) == want


@pytest.mark.gpu
def test_matrix_pair_tree_ids_take_two_levels():
    from fluidframework_amd.engine import Engine
    from fluidframework_amd.gitid import git_blob_id, summary_tree_id
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
    assert all(len(b) >= 2 and b[-1].startswith(b"[") for b in blobs)  # (the handleTable blob)
    assert eng.tree_ids() == [summary_tree_id(b, True, matrix=True) for b in blobs]
    assert eng.tree_ids(1, 2) == [summary_tree_id(blobs[1], True, matrix=True)]
    # host entries join the outer tree (one sorts between handleTable and segments, one is a subtree after it)
    extras = [[(BLOB, "rowMeta", git_blob_id(b"%d" % d)), (TREE, "segments0", EMPTY_TREE), (BLOB, "header", EMPTY_TREE)]
              for d in (0, 1)]
    assert eng.tree_ids(0, 2, extras) == [summary_tree_id(b, True, extras=x, matrix=True) for b, x in zip(blobs, extras)]


@pytest.mark.gpu
def test_tree_ids_after_replay_pipelined(monkeypatch):
    from fluidframework_amd.engine import Engine, pinned

    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")
    n = 600
    eng = _synthetic(n, 120, 0x9e1)
    hb = eng.download(0, n, pinned_memory=True)
    eng.reset()
    buf, off = eng.replay_pipelined(hb, pinned(64 << 20, "u1"), 4)
    assert eng.stats()["bad_docs"] == 0
    _check_tree_ids(eng, n, True, blobs_of=lambda d: Engine.split_record(buf, int(off[d]), int(off[d + 1])))


@pytest.mark.gpu
def test_validity_and_the_other_caches():
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
        eng.tree_ids()
    eng.apply(build_batch(logs, it))
    eng.summarize()
    first, _ = _check_tree_ids(eng, n, True)  # (computes the blob ids itself: no blob_ids() call came before)
    ids_before = eng.blob_ids()
    assert eng.tree_ids() == first
    assert eng.blob_ids() == ids_before
    eng.set_baseline()
    changed = (1, 4, 6)
    for d in changed:
        logs[d].message(msg(2, 1, "B", {"type": 0, "pos1": 3, "seg": "more text"}), it)
    eng.apply(build_batch(logs, it))
    with pytest.raises(EngineError):
        eng.tree_ids()  # (the batch cleared the summary)
    eng.summarize()
    delta_before = eng.summary_delta()
    second, _ = _check_tree_ids(eng, n, True)
    assert eng.summary_delta() == delta_before
    assert [d for d in range(n) if second[d] != first[d]] == list(changed)
    eng.set_baseline()
    eng.tree_ids()
    assert all(b is None for row in eng.summary_delta() for _, b in row)
    eng.reset()
    with pytest.raises(EngineError):
        eng.tree_ids()
