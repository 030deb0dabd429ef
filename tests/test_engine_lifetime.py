"""What an engine allocates, mtr_engine_destroy gives back -- every buffer, whichever call made it.

Free device memory is machine-wide, so a test cannot watch it; the engine counts the device and page-locked bytes its
own buffers hold (mtr_debug_live_bytes, engine.live_bytes()).  Each case reads the count, opens an engine with small
capacities, uses one group of calls -- each group allocates buffers the others never touch --, sees the count above
where it started while the engine is open, and exactly back there once it is closed.
"""
import gc

import pytest

pytestmark = pytest.mark.gpu

OPS = 32  # ops per document
SMALL = dict(max_segments=2 * OPS + 128, heap_entries=2 * OPS + 128, text_units=1 << 12, prop_words=1 << 12,
             remover_cells=1 << 10, ops_per_launch=16)
BLOB, TREE = 0o100644, 0o40000


def _lifetime(n_docs, use, **caps):
    from fluidframework_amd.engine import Engine, live_bytes

    gc.collect()  # (engines an earlier test left to the collector go now, not in the middle of this one)
    before = live_bytes()
    eng = Engine(n_docs, **{**SMALL, **caps})
    try:
        use(eng)
        assert live_bytes() > before
    finally:
        eng.close()
    assert live_bytes() == before


def _generate(eng, n):
    from fluidframework_amd.synth import make_cfg, tables

    eng.generate(make_cfg(n, OPS, writers=8, max_lag=16), tables(writers=8))
    assert eng.stats()["bad_docs"] == 0


def test_create_and_close():
    _lifetime(64, lambda eng: None)


def test_record_mode():
    """mtr_generate's generator state (280 bytes per document) was never freed."""
    def use(eng):
        _generate(eng, 64)
        eng.reset()
        eng.run()
        eng.summarize()
        assert eng.stats()["bad_docs"] == 0
        assert eng.summary_bytes() > 0

    _lifetime(64, use)


def test_generate_matrix():
    def use(eng):
        from fluidframework_amd.synth import make_cfg, tables

        cfg = make_cfg(2, OPS, writers=8, max_lag=16, weights=(12, 8, 80), max_text=4, max_range=3)
        eng.generate_matrix(cfg, tables(writers=8))  # matrix m = documents (2m rows, 2m + 1 cols)
        assert [eng.status(d)[0] for d in range(4)] == [0] * 4
        eng.summarize()

    _lifetime(4, use)


def test_hand_over():
    """Blob ids, tree ids with a host-made entry, ids of host blobs and trees, both ways to set a baseline, a delta."""
    def use(eng):
        from fluidframework_amd.gitid import git_blob_id, git_tree_id, summary_tree_id

        n = 16
        _generate(eng, n)
        eng.summarize()
        blobs = [eng.summary(d) for d in range(n)]
        ids = eng.blob_ids()
        assert ids == [[git_blob_id(b) for b in doc] for doc in blobs]
        extras = [[(BLOB, "catchupOps", git_blob_id(b"%d" % d))] for d in range(n)]
        assert eng.tree_ids(0, n, extras) == [summary_tree_id(b, True, extras=x) for b, x in zip(blobs, extras)]
        assert eng.git_blob_ids([b"a", b"bc"]) == [git_blob_id(b"a"), git_blob_id(b"bc")]
        trees = [[(BLOB, "a", git_blob_id(b"a"))], [(TREE, "t", git_tree_id([])), (BLOB, "bc", git_blob_id(b"bc"))]]
        assert eng.git_tree_ids(trees) == [git_tree_id(t) for t in trees]
        eng.set_baseline()  # (the current summary, copied on the device)
        assert eng.summary_delta_info() == (sum(len(doc) for doc in ids), 0, 0)
        eng.set_baseline(ids[:n // 2])  # (uploaded ids: the documents past the baseline's end are new)
        delta = eng.summary_delta()
        assert delta == [[(i, None if d < n // 2 else b) for i, b in zip(ids[d], blobs[d])] for d in range(n)]

    _lifetime(16, use)


def test_pipelined_replay(monkeypatch):
    """mtr_replay_pipelined over 4 ranges: the per-range flags, counters, sizes and events."""
    monkeypatch.setenv("MTR_PIPE_MIN_PART_DOCS", "0")  # (ranges this small would take the serial calls otherwise)

    def use(eng):
        import numpy as np

        from fluidframework_amd.engine import pinned

        n = 64
        _generate(eng, n)
        eng.summarize()
        want, want_off = eng.summaries(0, n)
        hb = eng.download(0, n, pinned_memory=True)  # (mtr_host_alloc: the caller's memory, not counted)
        eng.reset()
        buf, off = eng.replay_pipelined(hb, pinned(int(want_off[-1]) + 4096, "u1"), 4)
        assert eng.stats()["bad_docs"] == 0
        assert np.array_equal(off, want_off)
        assert np.array_equal(buf[:int(off[-1])], want[:int(want_off[-1])])

    _lifetime(64, use)


@pytest.mark.parametrize("run_first", [False, True])
def test_submit_after_pipelined_submit(run_first):
    """A pipelined hand-over belongs to the run that follows it and to no other: mtr_submit_pipelined of 8 documents,
    left without its run (or run, and the engine reset), then mtr_submit of 24 documents and mtr_run apply all 24.
    (The pending ranges once stayed with the engine, and the next run took them for its own batch: the documents past
    the first 8 were never applied, and nothing reported it.)"""
    ops = 100

    def use(eng):
        import numpy as np

        from fluidframework_amd.synth import make_cfg, tables

        n, first = 24, 8
        eng.generate(make_cfg(n, ops, writers=8, max_lag=16), tables(writers=8))
        assert eng.stats()["bad_docs"] == 0
        eng.summarize()
        want = eng.hashes(n)
        assert len(set(want.tolist())) > 1  # (the recipe's documents differ: a hash names its document's content)
        head = eng.download(0, first, pinned_memory=True)
        full = eng.download(0, n)
        eng.reset()
        eng.submit_pipelined(head, 2)
        if run_first:
            eng.run()
            eng.summarize()
            assert eng.stats()["bad_docs"] == 0
            assert np.array_equal(eng.hashes(first), want[:first])
            eng.reset()
        eng.submit(full)
        eng.run()
        eng.summarize()
        assert eng.stats()["bad_docs"] == 0
        assert np.array_equal(eng.hashes(n), want)

    _lifetime(24, use, max_segments=2 * ops + 128, heap_entries=2 * ops + 128)


def test_hbm_resident_launch():
    """Documents larger than LDS (test_gpu_parity.test_c5_shaped_hbm_resident's smallest shape): the scan scratch,
    chunk records and uid hints the first HBM-resident launch allocates."""
    from fluidframework_amd.synth import make_cfg, tables
    from oracle.oracle import generate

    n, grow, ops = 8, 20000, 2000
    cfg = make_cfg(n, ops, writers=64, max_lag=4096, text_cap=2 * grow + ops * 18 + 16)
    b, _, status = generate(cfg, tables(writers=64), 0, n, threads=8, grow=grow)
    assert (status == 0).all()

    def use(eng):
        eng.apply(b)
        assert eng.stats()["bad_docs"] == 0
        assert eng.stats()["max_leaves"] > grow

    _lifetime(n, use, max_segments=grow + grow // 14 + 2 * ops + 128, heap_entries=grow + 2 * ops + 128,
              text_units=2 * (int(cfg.text_cap) + 8192), prop_words=1 << 18, remover_cells=1 << 14, ops_per_launch=256)


def test_refused_create():
    """A capacity whose HBM-mode rows exceed the device's LDS is refused by mtr_engine_create; nothing stays."""
    from fluidframework_amd.engine import Engine, EngineError, live_bytes

    gc.collect()
    before = live_bytes()
    with pytest.raises(EngineError, match="bytes of LDS in HBM-resident mode"):
        Engine(4, **{**SMALL, "max_segments": 1 << 24})
    assert live_bytes() == before
