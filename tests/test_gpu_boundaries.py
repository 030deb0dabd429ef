"""The apply kernel at the edges of its per-op searches, against the CPU oracle.

An op's leaves are located by the view scan's rounds of 64 leaves (the first leaf whose inclusive visible prefix
reaches a position), a split takes its leaf block from one 64-leaf window around the located leaf, and zamboni stamps
and packs a block from the scour's own survivor mask.  These tests sit on the edges of those three: leaf counts at and
around the 64-lane round boundaries (synthetic logs small enough to end there, launches of 8 ops so launch ends fall
mid-document), and hand-built logs for the positions and blocks a search can get wrong -- position 0, the view's
length, a position past it, both ends of a range on leaf boundaries / inside one leaf / equal, a split in the first
and in the last leaf of a full block, and blocks that scour down to one leaf or to none.  Everything is bit-exact:
summaries, and on the hand-built logs every leaf's fields and tree level too.
"""
import numpy as np
import pytest

from fluidframework_amd import abi
from fluidframework_amd.batch import DocLog, Interner, build_batch
from oracle.oracle import OracleDoc, options

pytestmark = pytest.mark.gpu

ROUND_EDGES = (63, 64, 65, 127, 128, 129)  # leaf counts at and around the 64-lane rounds


def _engine(n_docs, **kw):
    from fluidframework_amd.engine import Engine
    caps = dict(max_segments=1024, heap_entries=1024, text_units=1 << 14, prop_words=1 << 14, remover_cells=1 << 12)
    caps.update(kw)
    return Engine(n_docs, **caps)


def _compare_export(eng, d, orc):
    ge, gh = eng.export(d)
    oe, oh = orc.export()
    assert gh == oh, f"doc {d}: height {gh} vs oracle {oh}"
    assert ge.shape == oe.shape, f"doc {d}: {len(ge)} leaves vs oracle {len(oe)}"
    bad = np.nonzero((ge != oe).any(axis=1))[0]
    assert bad.size == 0, f"doc {d}: first differing leaf {bad[0]}: {ge[bad[0]].tolist()} vs {oe[bad[0]].tolist()}"


# ---------------------------------------------------------------- synthetic logs around the round boundaries
N_DOCS = 64
SYNTH = [(60, 0), (60, 32), (130, 0), (130, 32), (260, 0), (260, 32)]  # (ops per document, max_lag)


def synth_case(ops, max_lag):
    """-> (cfg, tables, batch, oracle digests, oracle statuses) of one configuration (oracle only: no GPU)."""
    from fluidframework_amd.synth import make_cfg, tables
    from oracle.oracle import generate

    tabs = tables(writers=8)
    cfg = make_cfg(N_DOCS, ops, writers=8, max_lag=max_lag, seed=0xb0d1e5 + ops + max_lag)
    b, ohash, ost = generate(cfg, tabs, 0, N_DOCS, threads=8)
    return cfg, tabs, b, ohash, ost


def final_leaves(b, n):
    """Leaves of each of the batch's first n documents at the end of its log, from the oracle's export."""
    out = []
    for d in range(n):
        orc = OracleDoc(options())
        assert orc.apply(b, d) == 0
        out.append(len(orc.export()[0]))
    return out


@pytest.mark.parametrize("ops,max_lag", SYNTH, ids=[f"ops{o}-lag{l}" for o, l in SYNTH])
def test_round_boundaries_synthetic(ops, max_lag):
    """64 documents of about 60 / 130 / 260 ops: their leaf counts pass 63, 64, 65 (and 127, 128, 129) on the
    way, so the view scan's last round is full, one short, and one leaf long; launches of 8 ops."""
    cfg, tabs, b, ohash, ost = synth_case(ops, max_lag)
    assert (ost == 0).all()
    eng = _engine(N_DOCS, max_segments=2 * ops + 128, heap_entries=2 * ops + 128,
                  text_units=2 * int(cfg.text_cap) + 8192, ops_per_launch=8)
    eng.apply(b)
    eng.summarize()
    for d in range(N_DOCS):
        st, op = eng.status(d)
        assert st == 0, f"doc {d}: status {st:#x} at op {op}"
    ghash = eng.hashes(N_DOCS)
    bad = np.nonzero(ghash != ohash)[0]
    if bad.size:
        d = int(bad[0])
        orc = OracleDoc(options())
        assert orc.apply(b, d) == 0
        _compare_export(eng, d, orc)
        assert eng.summary(d) == orc.summarize(b, d)
    assert bad.size == 0


# ---------------------------------------------------------------- hand-built logs
class Script:
    """One document's sequenced messages: every op from a remote client, sequence numbers 1, 2, ..."""

    def __init__(self, it):
        self.it = it
        self.log = DocLog()
        self.log.start_collab("A")
        self.seq = 0
        self.msn = 0  # the minimumSequenceNumber the following messages carry

    def _msg(self, client, contents, ref, msn, kind="op"):
        self.seq += 1
        msn = self.msn if msn is None else msn
        self.log.message({"clientId": client, "sequenceNumber": self.seq, "type": kind,
                          "referenceSequenceNumber": self.seq - 1 if ref is None else ref,
                          "minimumSequenceNumber": msn, "contents": contents}, self.it)

    def ins(self, pos, text, client="B", ref=None, msn=None):
        self._msg(client, {"type": 0, "pos1": pos, "seg": text}, ref, msn)

    def rem(self, a, b, client="B", ref=None, msn=None):
        self._msg(client, {"type": 1, "pos1": a, "pos2": b}, ref, msn)

    def ann(self, a, b, props, client="B", ref=None, msn=None):
        self._msg(client, {"type": 2, "pos1": a, "pos2": b, "props": props}, ref, msn)

    def noop(self, client="B"):
        """A sequenced non-op message that moves minSeq up to the last message: updateSeqNumbers only (zamboni runs
        and pops up to two LRU entries)."""
        self.msn = self.seq
        self._msg(client, None, None, None, kind="noop")

    def drain(self, n=8):
        for _ in range(n):
            self.noop()

    def leaves(self, n, width=2):
        """n leaves of `width` units appended one by one (leaf blocks of 4 once a block of 8 splits)."""
        for k in range(n):
            self.ins(k * width, chr(ord("a") + k % 26) * width)


def _s_insert_ends(s):
    s.ins(0, "abc")
    s.ins(3, "de")      # at the end
    s.ins(0, "x")       # at 0 of a document with leaves
    s.ins(6, "yz")      # at the end again
    s.ins(5, "!", client="C", ref=2)  # the end of client C's view at seq 2 ("abcde"): inside for everyone else


def _s_remove_on_boundaries(s):
    s.leaves(5, 3)
    s.rem(3, 9)         # [3, 9) = leaves 1 and 2 exactly: neither end splits


def _s_remove_in_one_leaf(s):
    s.ins(0, "abcdefgh")
    s.rem(2, 5)         # both ends inside the one leaf: two splits of the same leaf
    s.ann(6, 7, {"bold": True})


def _s_remove_empty(s):
    s.leaves(3, 3)
    s.rem(4, 4)         # pos1 == pos2: the leaf is split once at 4, nothing is removed
    s.rem(0, 0)
    s.rem(9, 9)         # at the view's length


def _s_insert_past_end(s):
    s.leaves(3, 2)
    s.ins(9, "zz")      # the view is 6 long
    s.ins(0, "never")   # never applied
    return 4            # the failing op's index (START_COLLAB is op 0 of the log, the three leaves ops 1 .. 3)


def _full_block(s):
    """13 leaves of 2 in blocks of 4, 4, 5; three inserts on the boundary ahead of leaf 5 fill the second block to 7."""
    s.leaves(13)
    for k in range(3):
        s.ins(10, "QRS"[k] * 2)


def _s_split_first_of_full_block(s):
    _full_block(s)
    s.rem(9, 10)        # splits leaf 4, the block's first leaf ("ee" at [8, 10)): the 8th leaf, the block splits


def _s_split_last_of_full_block(s):
    _full_block(s)
    s.ann(21, 22, {"color": "red"})  # splits the block's last leaf ("hh" at [20, 22) after 6 inserted units)


def _s_split_first_leaf_of_full_root(s):
    s.leaves(7)
    s.rem(0, 1)         # the root block holds 7 leaves: leaf 0 splits, the root splits


def _s_split_last_leaf_of_full_root(s):
    s.leaves(7)
    s.ann(13, 14, {"bold": False})  # the document's last leaf splits: the window ends at the array's end


def _s_scour_to_one(s):
    s.leaves(12)
    s.rem(8, 14)        # three of the four leaves of the block of leaves 4 .. 7
    s.drain()           # minSeq passes the remove: the block scours down to one leaf
    s.ins(3, "t")


def _s_scour_to_none(s):
    s.leaves(12)
    s.rem(8, 16)        # the whole block of leaves 4 .. 7
    s.drain()           # it scours down to no leaf: packParent over an empty block
    s.ins(8, "u")


HAND = [_s_insert_ends, _s_remove_on_boundaries, _s_remove_in_one_leaf, _s_remove_empty, _s_insert_past_end,
        _s_split_first_of_full_block, _s_split_last_of_full_block, _s_split_first_leaf_of_full_root,
        _s_split_last_leaf_of_full_root, _s_scour_to_one,
        _s_scour_to_none]


def hand_batch():
    """-> (batch, [index of the op expected to fail, or None] per document)."""
    it = Interner()
    logs, fails = [], []
    for f in HAND:
        s = Script(it)
        fails.append(f(s))
        logs.append(s.log)
    return build_batch(logs, it), fails


def test_hand_built_edges():
    """Every hand-built document: status, every leaf (lengths, seqs, removal info, tree levels) and the summary
    bytes equal the oracle's; the insert past the end fails with MTR_ERR_INSERT_FAILED at that op, as the oracle
    does."""
    b, fails = hand_batch()
    n = len(HAND)
    eng = _engine(n, ops_per_launch=8)
    eng.apply(b)
    eng.summarize()
    for d in range(n):
        orc = OracleDoc(options())
        ost = orc.apply(b, d)
        st, op = eng.status(d)
        name = HAND[d].__name__
        if fails[d] is None:
            assert ost == 0, name
            assert st == 0, f"{name}: status {st:#x} at op {op}"
            _compare_export(eng, d, orc)
            assert eng.summary(d) == orc.summarize(b, d), name
        else:
            assert ost == abi.MTR_ERR_INSERT_FAILED, f"{name}: oracle status {ost:#x}"
            assert (st, op) == (abi.MTR_ERR_INSERT_FAILED, fails[d]), f"{name}: status {st:#x} at op {op}"
