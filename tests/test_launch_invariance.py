"""The apply path at launch splits, slack policies and size-class crossings (mtr_run's round loop: plan_launch and
ApplyRun in csrc/apply_run.hip), against the CPU oracle.

What a document's result may not depend on: how many ops a launch applies (a document is staged into LDS, runs
`ops_per_launch` ops and is stored back: leaves, LRU heap, needsScour bits, cursors), whether the launch had room for
every op or the document yielded and was classed again, which kernel the host chose for its size (fixed capacity,
AV_LDS_LEAN, the HBM-resident team kernel, hole slots from kGapMin leaves), what else the batch holds (a delta flag or
a rare record moves every launch to another instantiation), and how the log was cut into batches.  Every check is
exact: leaves and tree levels (test_gpu_parity._compare_export), the text and the summary bytes, against
oracle.OracleDoc.

Which kernel ran is read from the engine's launch census (Engine.launch_counts, mtr_debug_launch_counts): the
constants below only aim a recipe at a boundary, the census assertions prove that the run reached the kernel.  The
recipes' shapes are checked on the oracle alone (no GPU) by test_recipes_reach_their_shapes_on_the_oracle.
"""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from fixtures import load_replay, replay_files, replay_log
from fluidframework_amd import abi
from fluidframework_amd.batch import Interner, build_batch
from fluidframework_amd.synth import make_cfg, tables, with_docs
from oracle import oracle
from oracle.oracle import OracleDoc, generate, options
from test_gpu_parity import _compare_export

# ---------------------------------------------------------------- the boundaries the recipes aim at
# (leaf counts; csrc/apply_run.hip: plan_launch, the policy of one size class's launch, its knob RunKnobs::lds_limit,
# and ApplyRun::choose_groups for `class_leaves`; csrc/apply.hip.h: MTR_FIXED_CAPS near line 5897, lds_bytes near
# line 448, kGapMin at line 95)
CLASS_LEAVES = 64       # class width of a batch under 4,096 documents (ApplyRun::choose_groups: `class_leaves`)
SLACK = 8               # room of a yielding launch (plan_launch: `slack`, more documents than CUs)
CAP_ROUND = 32          # a launch's capacity is a multiple of it (round32; round64 above 1,024)
FIXED_CAP_MAX = 1536    # the largest capacity with a compile-time layout (MTR_FIXED_CAPS); above it AV_LDS_LEAN
LDS_LIMIT = 160 * 1024  # bytes (RunKnobs::lds_limit); lds_bytes(cap, lhcap) = 32 cap + 8 lhcap + a constant
LDS_LEAVES_LO = 4400    # a capacity of this many leaves fits LDS while the LRU heap holds at most half as many entries
LDS_LEAVES_HI = 5120    # ... and this many leaves never do: apply_kernel<true>, HBM-resident
assert 32 * LDS_LEAVES_HI == LDS_LIMIT and 32 * LDS_LEAVES_LO + 8 * (LDS_LEAVES_LO // 2) < LDS_LIMIT - 4096
#                         (between the two the heap decides; with a small heap the limit is near 4,900 leaves)
GAP_MIN = 8192          # apply.hip.h: kGapMin, the hole-slot layout (Eng::spread, holeify)
DEFAULT_K = 256         # mtr_engine_create's ops_per_launch when the caller passes 0
CUS_NOMINAL = 256       # an MI355X's compute units: the CPU shape check's stand-in for the device's count

WRITERS = 8
STOPS = (0, 1, 2, 63, 64, 65, 127, 128, 129, None)  # test 3: records a document stops after (None: all of them)


def _tabs():
    return tables(writers=WRITERS)


# ---------------------------------------------------------------- oracle side
class _Exported:
    """A kept export, standing where _compare_export reads an engine's or an oracle's."""

    def __init__(self, leaves, height):
        self.leaves, self.height = leaves, height

    def export(self, d=None):
        return self.leaves, self.height


class _Want(_Exported):
    def __init__(self, orc, b, d):
        super().__init__(*orc.export())
        self.text = orc.text()
        self.summary = orc.summarize(b, d)


def _leaves(orc) -> int:
    """len(orc.export()[0]) without the copy."""
    h = C.c_int32(0)
    n = oracle.lib().oracle_doc_export(orc.h, None, 0, C.byref(h))
    return int(-n if n < 0 else n)


def _opts(newlen):
    return options(new_length_calc=newlen)


def _wants(b, newlen, batches=None):
    """Per document the oracle's result of applying `batches` (default: b alone) in order."""
    res = []
    for d in range(len(b.docs)):
        orc = OracleDoc(_opts(newlen))
        for x in batches or [b]:
            st = orc.apply(x, d)
            assert st == 0, f"oracle: doc {d}: status {st:#x}"
        res.append(_Want(orc, b, d))
    return res


def _track(b, d, newlen, start=0):
    """Oracle leaf counts of document d after each of its records from `start` on (prefix stepping)."""
    orc = OracleDoc(_opts(newlen))
    assert orc.apply(b, d, 0, start) == 0
    out = [_leaves(orc)]
    for k in range(start, int(b.docs["op_count"][d])):
        st = orc.apply(b, d, k, k + 1)
        assert st == 0, f"oracle: doc {d}: status {st:#x} at record {k}"
        out.append(_leaves(orc))
    return out


# ---------------------------------------------------------------- recipes
def _prefix(b, counts):
    """b with document d stopped after counts[d] records (None: all)."""
    docs = b.docs.copy()
    for d, k in enumerate(counts):
        if k is not None:
            docs["op_count"][d] = min(int(k), int(docs["op_count"][d]))
    return with_docs(_tabs(), docs, b.ops, b.text)


def _concat(parts):
    """Documents of several recorded batches (sharing the recipe tables) as one batch."""
    docs = np.concatenate([p.docs for p in parts])
    o = t = k = 0
    for p in parts:
        docs["op_begin"][k:k + len(p.docs)] += o
        docs["text_base"][k:k + len(p.docs)] += t
        o, t, k = o + len(p.ops), t + len(p.text), k + len(p.docs)
    return with_docs(_tabs(), docs, np.concatenate([p.ops for p in parts]), np.concatenate([p.text for p in parts]))


@functools.lru_cache(maxsize=None)
def split_recipe(n, long_ranges, newlen):
    """Tests 1-3 and 7: n documents of 200 messages (C3's writers and lag).  Insert-heavy with C3's ranges (about a
    leaf an op: 64 ops outgrow a yielding launch's 8 leaves of room), or long_ranges: removes and annotates of up to
    60 units, remove-heavy -- a range op spans several leaf blocks and zamboni has work."""
    kw = dict(max_range=60, weights=(35, 50, 15)) if long_ranges else dict(weights=(60, 30, 10))
    cfg = make_cfg(n, 200, writers=WRITERS, max_lag=32, seed=0x1a7c + long_ranges, **kw)
    b, _, st = generate(cfg, _tabs(), 0, n, threads=8, opts=_opts(newlen))
    assert (st == 0).all()
    return b


def _grown(n, grow, ops, seed):
    """Insert-heavy documents on `grow` loaded leaves whose writers never catch up (every reference sequence number
    stays 0, and so does the MSN): nothing is scoured, and the leaves grow by more than one an op."""
    cfg = make_cfg(n, ops, writers=WRITERS, max_lag=1 << 20, weights=(90, 5, 5), seed=seed,
                   text_cap=2 * grow + ops * 18 + 16)
    b, _, st = generate(cfg, _tabs(), 0, n, threads=8, grow=grow)
    assert (st == 0).all()
    return b


# test 5's ladder: (loaded leaves, messages of the recipe, messages each document stops after)
LADDER = [
    (0, 80, (4, 10, 16, 22, 30, 38, 46, 54, 62, 70, 80)),  # ends around 32, 64, 96 and 128 leaves
    (960, 80, (8, 30, 55, 80)),                            # around 1,024
    (1470, 80, (8, 30, 55, 80)),                           # around FIXED_CAP_MAX
    (3000, 80, (8, 80)),                                   # AV_LDS_LEAN's own range
    (4500, 80, (8, 80)),                                   # around the LDS limit
    (LDS_LEAVES_HI - 60, 80, (8, 80)),                     # across the first size that can never be LDS-resident
    (6400, 60, (60,)),                                     # well above it
]
LADDER_BIG = sum(len(x[2]) for x in LADDER) - 1  # the largest document's index


@functools.lru_cache(maxsize=None)
def ladder_recipe():
    parts = []
    for i, (grow, ops, stops) in enumerate(LADDER):
        g = _grown(len(stops), grow, ops, 0x1add + i)
        parts.append(_prefix(g, [grow + 1 + k for k in stops]))
    return _concat(parts)


def _continue(b, extra, seed, max_lag, weights, max_range):
    """Every document's log of b continued by `extra` messages drawn as include/mtr_synth.h draws them (a uniformly
    chosen writer at a reference sequence number at most max_lag behind, the MSN the writers' minimum, positions
    valid in the writer's view), with the oracle as the exact simulator; inserted text is taken from the recorded
    text.  Returns (batch, per-document record count of b)."""
    n = len(b.docs)
    per = int(b.docs["op_count"][0])
    assert (b.docs["op_count"] == per).all()
    ops = np.zeros(n * (per + extra), dtype=abi.OP_DTYPE)
    docs = b.docs.copy()
    for d in range(n):
        o = int(b.docs["op_begin"][d])
        ops[d * (per + extra):d * (per + extra) + per] = b.ops[o:o + per]
    docs["op_begin"] = np.arange(n, dtype=np.uint64) * (per + extra)
    docs["op_count"] = per + extra
    nb = with_docs(_tabs(), docs, ops, b.text)
    assert nb.ops.ctypes.data == ops.ctypes.data  # (written in place below, read by the oracle through nb.c)
    rng = random.Random(seed)
    tot = sum(weights)
    for d in range(n):
        base = d * (per + extra)
        orc = OracleDoc(options())
        assert orc.apply(nb, d, 0, per) == 0
        rec = ops[base:base + per]
        msgs = rec[rec["seq"] > 0]
        seq, msn = int(msgs["seq"].max()), int(msgs["min_seq"].max())
        refs = {w: int(msgs["ref_seq"][msgs["client"] == w].max(initial=0)) for w in range(1, WRITERS + 1)}
        tcount = int(docs["text_count"][d])
        for k in range(extra):
            seq += 1
            w = 1 + rng.randrange(WRITERS)
            refs[w] = max(refs[w], seq - 1 - rng.randrange(max_lag + 1))
            msn = max(msn, min(refs.values()))
            L = max(0, int(orc.length(refs[w], w)))
            pick = rng.randrange(tot)
            kind = 0 if pick < weights[0] or L <= 0 else (1 if pick < weights[0] + weights[1] else 2)
            op = ops[base + per + k:base + per + k + 1]
            op["flags"], op["client"], op["seq"], op["ref_seq"], op["min_seq"] = abi.F_LAST, w, seq, refs[w], msn
            if kind == 0:
                units = 1 + rng.randrange(16)
                op["type"], op["pos1"], op["pos2"] = abi.OP_INSERT, rng.randrange(L + 1), -1
                op["payload"], op["payload2"] = rng.randrange(tcount - units), units
            else:
                start = rng.randrange(L)
                op["type"] = abi.OP_REMOVE if kind == 1 else abi.OP_ANNOTATE
                op["pos1"], op["pos2"] = start, start + 1 + rng.randrange(min(L - start, max_range))
                op["payload"] = rng.randrange(64) if kind == 2 else 0
            st = orc.apply(nb, d, per + k, per + k + 1)
            assert st == 0, f"continuing doc {d}: oracle status {st:#x} at message {k}"
    return nb, per


# test 6: name -> (documents, loaded leaves, phase 1 messages, phase 2 messages, phase 2's longest range, K)
CROSSINGS = {
    "fixed-cap": (3, 1400, 150, 250, 60, 32),
    "lds-limit": (2, LDS_LEAVES_LO - 150, 750, 330, 120, 32),
    "gap-min": (2, GAP_MIN - 100, 130, 220, 200, 0),
}


@functools.lru_cache(maxsize=None)
def crossing_recipe(name):
    """Phase 1 (insert-heavy, deep lag) grows the documents through the boundary; phase 2 (remove-heavy, lag <= 2:
    the MSN follows the head) has zamboni take them back down through it.  -> (batch, records of phase 1)"""
    n, grow, up, down, max_range, _ = CROSSINGS[name]
    g = _grown(n, grow, up, 0xc055 + grow)
    return _continue(g, down, 0xd0a + grow, 2, (8, 80, 12), max_range)


def _phases(b, per):
    """(phase 1, phase 2) of a crossing_recipe as two batches, the second holding the records after `per`."""
    docs = b.docs.copy()
    docs["op_begin"] += per
    docs["op_count"] -= per
    return _prefix(b, [per] * len(b.docs)), with_docs(_tabs(), docs, b.ops, b.text)


def _flag_delta(b, d):
    """b with document d's first insert message flagged MTR_F_DELTA (its delta is reported; nothing else changes)."""
    ops = b.ops.copy()
    o, c = int(b.docs["op_begin"][d]), int(b.docs["op_count"][d])
    k = o + int(np.nonzero((ops["type"][o:o + c] == abi.OP_INSERT) & (ops["seq"][o:o + c] > 0))[0][0])
    ops["flags"][k] |= abi.F_DELTA
    return with_docs(_tabs(), b.docs.copy(), ops, b.text)


def _with_rare_record(b, src):
    """b plus one more document: a copy of document src whose first annotate is a combining one ("rewrite",
    MTR_COMB_REWRITE: a record op_scan_kernel counts as `ext`), so the whole batch runs the X instantiations."""
    o, c = int(b.docs["op_begin"][src]), int(b.docs["op_count"][src])
    extra = b.ops[o:o + c].copy()
    k = int(np.nonzero(extra["type"] == abi.OP_ANNOTATE)[0][0])
    extra["payload2"][k] = abi.COMB_REWRITE
    docs = np.concatenate([b.docs, b.docs[src:src + 1]])
    docs["op_begin"][-1] = len(b.ops)
    return with_docs(_tabs(), docs, np.concatenate([b.ops, extra]), b.text)


def _big_alone():
    """Test 5's largest document as a batch of its own."""
    b = ladder_recipe()
    return with_docs(_tabs(), b.docs[LADDER_BIG:LADDER_BIG + 1].copy(), b.ops, b.text)


def _golden_messages():
    path = [p for p in replay_files() if "len_64-clients_8" in p][0]
    groups = load_replay(path)
    return groups, [m for g in groups for m in g["msgs"]]


def _golden_batches(cut):
    """The golden log delivered in batches of `cut` messages (None: one batch), cut as
    test_gpu_parity.test_replay_logs_group_by_group cuts: the log grows, each batch holds what is new."""
    groups, msgs = _golden_messages()
    it = Interner()
    log = replay_log(groups, it)
    cut = cut or len(msgs)
    out = []
    for k in range(0, len(msgs), cut):
        for m in msgs[k:k + cut]:
            log.message(m, it)
        out.append(build_batch([log], it))
    return out


# ---------------------------------------------------------------- C. the recipes' shapes, on the oracle alone
def _span(b, newlen=False, start=None):
    """(fewest, most) oracle leaves of every document of b over its records from `start` (default: after its load)."""
    res = []
    for d in range(len(b.docs)):
        o, c = int(b.docs["op_begin"][d]), int(b.docs["op_count"][d])
        s = start if start is not None else int((b.ops["type"][o:o + c] == abi.OP_LOAD).sum())
        t = _track(b, d, newlen, min(s, c))
        res.append((min(t), max(t)))
    return res


def test_recipes_reach_their_shapes_on_the_oracle():
    """Every recipe of this file replayed on the oracle alone: every status is 0 (asserted inside _track / _wants /
    _continue), and prefix stepping shows each recipe's fewest and most leaves on the intended sides of its
    boundary."""
    # tests 1-3, 7: small documents that pass several 64-leaf classes, in both length modes
    for long_ranges in (False, True):
        for newlen in (False, True):
            for n in (48, CUS_NOMINAL + 64):
                sp = _span(split_recipe(n, long_ranges, newlen), newlen)
                assert min(a for a, _ in sp) == 0
                assert max(z for _, z in sp) >= 2 * CLASS_LEAVES, "no document reaches the third class"
                assert max(z for _, z in sp) + DEFAULT_K + 16 < FIXED_CAP_MAX  # (roomy launches stay fixed-capacity)
    # test 3: the stops are below every document's record count
    assert int(split_recipe(48, False, False).docs["op_count"].min()) > max(k for k in STOPS if k is not None)
    # test 4: the golden log is longer than two cuts
    assert len(_golden_messages()[1]) > 2 * 65
    for cut in (None, 64):
        _wants(_golden_batches(cut)[-1], False, _golden_batches(cut))
    # test 5: the end sizes straddle every boundary
    lad = ladder_recipe()
    ends = [len(w.leaves) for w in _wants(lad, False)]
    for edge in (32, 64, 96, 128, 1024, FIXED_CAP_MAX):
        assert any(edge - 24 <= x < edge for x in ends) and any(edge < x <= edge + 110 for x in ends), (edge, ends)
    assert any(FIXED_CAP_MAX + 300 < x < LDS_LEAVES_LO - DEFAULT_K - 16 - 2 * CAP_ROUND for x in ends), ends
    assert any(LDS_LEAVES_LO < x < LDS_LEAVES_HI - 150 for x in ends), ends
    assert any(LDS_LEAVES_HI - 150 < x < LDS_LEAVES_HI for x in ends) and any(LDS_LEAVES_HI <= x for x in ends), ends
    assert ends[LADDER_BIG] == max(ends) and ends[LADDER_BIG] > LDS_LEAVES_HI + 1000, ends
    # test 6: below the boundary at the start, above at the turn, below again at the end
    for name, (lo_edge, hi_edge) in {"fixed-cap": (FIXED_CAP_MAX, FIXED_CAP_MAX),
                                     "lds-limit": (LDS_LEAVES_LO, LDS_LEAVES_HI),
                                     "gap-min": (GAP_MIN, GAP_MIN)}.items():
        n, grow, up, down, _, K = CROSSINGS[name]
        room = (K or DEFAULT_K) + 16 + 2 * CAP_ROUND if name != "gap-min" else 0  # (capacity = leaves + K + 16, rounded)
        b, per = crossing_recipe(name)
        assert per == grow + 1 + up and len(b.docs) == n
        for d in range(n):
            t = _track(b, d, False, grow + 1)
            assert t[0] == grow and grow + room < lo_edge, (name, d, t[0])
            assert max(t[:up + 1]) > hi_edge, (name, d, max(t[:up + 1]))
            assert min(t[up:]) + room < lo_edge, (name, d, min(t[up:]))
            if name == "gap-min":  # (not so far down that holes outnumber the leaves threefold: that respreads)
                assert min(t[up:]) > GAP_MIN // 3, (name, d, min(t[up:]))
    # test 7: the changed batches still replay, and to the plain run's result
    plain = split_recipe(48, True, False)
    w0 = _wants(plain, False)
    for changed in (_flag_delta(plain, 5), _with_rare_record(plain, 0)):
        w = _wants(changed, False)
        for d in range(len(plain.docs)):
            assert np.array_equal(w[d].leaves, w0[d].leaves) and w[d].summary == w0[d].summary
    big = _big_alone()
    for changed in (_flag_delta(big, 0), _with_rare_record(big, 0)):
        assert np.array_equal(_wants(changed, False)[0].leaves, _wants(big, False)[0].leaves)


# ---------------------------------------------------------------- engine side
def _engine(n_docs, **kw):
    from fluidframework_amd.engine import Engine
    caps = dict(max_segments=1024, heap_entries=1024, text_units=1 << 14, prop_words=1 << 16, remover_cells=1 << 12)
    caps.update(kw)
    return Engine(n_docs, **caps)


def _caps_for_leaves(leaves, text):
    """Engine capacities for documents of up to `leaves` leaves (hole slots: one per 14 and room to respread)."""
    seg = leaves + leaves // 14 + 512
    return dict(max_segments=seg, heap_entries=seg, text_units=2 * text + 8192, prop_words=1 << 16,
                remover_cells=1 << 13)


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _check(eng, wants, what, docs=None):
    """Every document of the engine against the oracle's result: status, leaves and tree levels, text, summary."""
    eng.summarize()
    for d in (range(len(wants)) if docs is None else docs):
        st, op = eng.status(d)
        assert st == 0, f"{what}: doc {d}: status {st:#x} at op {op}"
        try:
            _compare_export(eng, d, wants[d])
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None
        assert eng.text(d) == wants[d].text, f"{what}: doc {d}: text differs"
        assert eng.summary(d) == wants[d].summary, f"{what}: doc {d}: summary bytes differ"


def _kept(eng, n):
    return [_Exported(*eng.export(d)) for d in range(n)]


def _same(eng, kept, what):
    for d, k in enumerate(kept):
        try:
            _compare_export(eng, d, k)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None


def _split_name(K):
    return f"ops_per_launch {K or 'default'}"


@pytest.mark.gpu
@pytest.mark.parametrize("newlen", [False, True], ids=["oldlen", "newlen"])
@pytest.mark.parametrize("long_ranges", [False, True], ids=["short-ranges", "long-ranges"])
def test_split_invariance_roomy(long_ranges, newlen):
    """Test 1.  Fewer documents than CUs: a launch has room for every op and no document yields.  One log under eight
    splits -- K = 1 stores and reloads the document after every op, 63/64/65 straddle a wave's width -- gives the
    oracle's result every time, and the eight exports are identical."""
    n = min(48, _cus())
    b = split_recipe(n, long_ranges, newlen)
    wants = _wants(b, newlen)
    first = None
    for K in (1, 2, 3, 63, 64, 65, 200, 0):
        eng = _engine(n, ops_per_launch=K, new_length_calc=newlen)
        eng.apply(b)
        _check(eng, wants, _split_name(K))
        if first is None:
            first = _kept(eng, n)
        _same(eng, first, f"{_split_name(K)} against ops_per_launch 1")
        c = eng.launch_counts()
        assert c["launches"] == eng.stats()["launches"] > 0 and c["global_mode"] == 0, c
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("newlen", [False, True], ids=["oldlen", "newlen"])
@pytest.mark.parametrize("long_ranges", [False, True], ids=["short-ranges", "long-ranges"])
def test_split_invariance_yielding(long_ranges, newlen):
    """Test 2.  More documents than CUs: a launch has 8 leaves of room, a document that could overflow it stops
    before the op and is classed again.  The census proves the yields.  Without one, round r starts with every
    document r * K records on and launches once per 64-leaf class those documents occupy -- the oracle's prefix
    stepping gives that count exactly -- and a yield adds rounds, so more launches than that means documents yielded
    and were classed again.  Where a run has one round (the default K), the count is at most the classes the
    documents ever visit, the figure asked for first; at K = 64 / 65 that product (rounds x classes ever visited: 4 x
    4 = 16) is out of reach of any such recipe: the documents that yield bunch up under the class's capacity, so a
    round launches one or two classes (measured on an MI355X, long-ranges: 10 launches at K = 64, 8 at the default).
    K = 1 cannot yield on leaves -- an op adds at most two -- so there the exact count is the floor."""
    n = _cus() + 64
    b = split_recipe(n, long_ranges, newlen)
    wants = _wants(b, newlen)
    tracks = [_track(b, d, newlen) for d in range(n)]
    sizes = {x for t in tracks for x in t}
    classes, most = len({x // CLASS_LEAVES for x in sizes}), max(sizes)
    first = None
    for K in (1, 64, 65, 0):
        eng = _engine(n, ops_per_launch=K, new_length_calc=newlen)
        eng.apply(b)
        _check(eng, wants, _split_name(K))
        if first is None:
            first = _kept(eng, n)
        _same(eng, first, f"{_split_name(K)} against ops_per_launch 1")
        c = eng.launch_counts()
        k = K or DEFAULT_K
        rounds = -(-max(len(t) - 1 for t in tracks) // k)
        unyielding = sum(len({t[r * k] // CLASS_LEAVES for t in tracks if r * k < len(t) - 1}) for r in range(rounds))
        print(f"{_split_name(K)}: {c['launches']} launches; without a yield {unyielding} in {rounds} rounds; "
              f"{classes} classes visited; census {c}")
        if K == 1:
            assert c["launches"] >= unyielding > 0, c
        else:
            assert c["launches"] > unyielding, f"{_split_name(K)}: no document yielded: {c}"
        if rounds == 1:
            assert c["launches"] > rounds * classes, f"{_split_name(K)}: {c}"
        assert c["max_cap"] < most + SLACK + 8 + CAP_ROUND, c  # (8 leaves of room, not K: the yielding policy)
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [64, 1])
def test_ragged_op_counts(K):
    """Test 3.  Documents of one batch that stop after 0, 1, 2, 63, 64, 65, 127, 128, 129 and all of their records
    (several of each) leave the rounds at different times; each equals the oracle's prefix."""
    n = min(48, _cus())
    b = _prefix(split_recipe(n, True, False), [STOPS[d % len(STOPS)] for d in range(n)])
    wants = _wants(b, False)
    eng = _engine(n, ops_per_launch=K)
    eng.apply(b)
    _check(eng, wants, _split_name(K))
    assert eng.stats()["ops"] == int(b.docs["op_count"].sum())


@pytest.mark.gpu
def test_batch_split_invariance():
    """Test 4.  One golden log as one batch, as a batch per message, and cut every 63, 64 and 65 messages (around the
    engine's 64 ops a launch): the same leaves, text and summary, the oracle's."""
    whole = _golden_batches(None)
    want = _wants(whole[-1], False, whole)
    groups, _ = _golden_messages()
    assert want[0].text == groups[-1]["resultText"]
    first = None
    for cut in (None, 1, 63, 64, 65):
        eng = _engine(1, ops_per_launch=64, max_segments=8192, heap_entries=8192, text_units=1 << 18,
                      prop_words=1 << 18, remover_cells=1 << 14)  # (test_gpu_parity's capacities for these logs)
        for x in _golden_batches(cut):
            eng.apply(x)
        what = f"batches of {cut or 'all'} messages"
        _check(eng, want, what)
        if first is None:
            first = _kept(eng, 1)
        _same(eng, first, f"{what} against one batch")
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [16, 0], ids=["k16", "default"])
def test_mixed_classes_in_one_batch(K):
    """Test 5.  Documents from 5 to 6,500 leaves in one batch: a round launches many classes and both residencies.
    The census shows fixed-capacity, AV_LDS_LEAN (above the fixed capacities) and AV_HBM_LEAN launches in the one
    run."""
    b = ladder_recipe()
    n = len(b.docs)
    assert n <= _cus()
    wants = _wants(b, False)
    eng = _engine(n, ops_per_launch=K, **_caps_for_leaves(7000, int(b.docs["text_count"].max())))
    eng.apply(b)
    _check(eng, wants, _split_name(K))
    c = eng.launch_counts()
    print(f"{_split_name(K)}: census {c}")
    assert c["fixed_cap"] > 0 and c["LDS_LEAN"] > 0 and c["HBM_LEAN"] > 0, c
    assert c["global_mode"] == c["HBM_LEAN"] and c["launches"] == c["fixed_cap"] + c["LDS_LEAN"] + c["HBM_LEAN"], c
    assert FIXED_CAP_MAX < c["max_lds_cap"], c  # AV_LDS_LEAN as the replay kernel of a large LDS-resident document
    assert c["min_cap"] < FIXED_CAP_MAX < c["max_lds_cap"] < c["max_cap"], c


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CROSSINGS))
def test_crossings_during_a_run(name):
    """Test 6.  Documents that start just under a boundary, grow through it (phase 1: insert-heavy, deep lag) and are
    scoured back down through it (phase 2: remove-heavy, the MSN at the head), the phases as two batches so the
    census tells them apart: across 1,536 leaves fixed-capacity <-> AV_LDS_LEAN, across the LDS limit AV_LDS_LEAN <->
    AV_HBM_LEAN, across 8,192 the first spread and then fewer leaves than kGapMin with the holes still in place."""
    n, grow, up, down, _, K = CROSSINGS[name]
    b, per = crossing_recipe(name)
    p1, p2 = _phases(b, per)
    eng = _engine(n, ops_per_launch=K, **_caps_for_leaves(grow + 2 * up + 64, int(b.docs["text_count"].max())))
    eng.apply(p1)
    _check(eng, _wants(p1, False), f"{name}, phase 1")
    c1 = eng.launch_counts()
    slots1 = eng.stats()["max_leaves"]
    eng.apply(p2)
    wants = _wants(b, False)
    _check(eng, wants, f"{name}, phase 2")
    c2 = eng.launch_counts()
    slots2 = eng.stats()["max_leaves"]
    ph2 = {k: c2[k] - c1[k] for k in c2 if k not in ("min_cap", "max_cap", "max_lds_cap")}
    print(f"{name}: phase 1 census {c1}; phase 2 launches {ph2}; slots {slots1}, {slots2}")
    if name == "fixed-cap":
        assert c1["LDS_LEAN"] > 0 and c1["fixed_cap"] > 0 and c1["global_mode"] == 0, c1
        assert ph2["LDS_LEAN"] > 0 and ph2["fixed_cap"] > 0 and c2["global_mode"] == 0, ph2
        assert c2["max_lds_cap"] > FIXED_CAP_MAX, c2
    elif name == "lds-limit":
        assert c1["LDS_LEAN"] > 0 and c1["HBM_LEAN"] > 0, c1
        assert ph2["LDS_LEAN"] > 0 and ph2["HBM_LEAN"] > 0, ph2
    else:
        assert c2["HBM_LEAN"] == c2["global_mode"] == c2["launches"] - c2["fixed_cap"] - c2["LDS_LEAN"] > 0, c2
        assert ph2["HBM_LEAN"] == ph2["launches"] > 0, ph2
        # hole slots: the engine's slot count passes the leaves it holds once a document has been spread, and stays
        # above them when the leaves are fewer than kGapMin again
        most1 = max(len(w.leaves) for w in _wants(p1, False))
        most2 = max(len(w.leaves) for w in wants)
        assert most1 > GAP_MIN > most2
        assert slots1 > most1 + most1 // 32, (slots1, most1)
        assert slots2 > most2 + most2 // 32, (slots2, most2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["LDS_DL", "LDS_X", "HBM_DL", "HBM_X"])
def test_variants_by_batch_content(case):
    """Test 7.  The same logs reach the other instantiations by what the batch holds: one op flagged MTR_F_DELTA
    moves every launch to the delta-reporting kernels, one document with a combining annotate to the X kernels.  The
    census names the variant; the results equal the oracle's and the plain run's."""
    small = case.startswith("LDS")
    plain = split_recipe(min(48, _cus()), True, False) if small else _big_alone()
    n = len(plain.docs)
    changed = _flag_delta(plain, n // 2) if case.endswith("DL") else _with_rare_record(plain, 0)
    caps = {} if small else _caps_for_leaves(7000, int(plain.docs["text_count"].max()))
    e0 = _engine(n, **caps)
    e0.apply(plain)
    wants = _wants(plain, False)
    _check(e0, wants, "plain batch")
    c0 = e0.launch_counts()
    assert c0[case] == 0 and (c0["fixed_cap"] > 0 if small else c0["HBM_LEAN"] > 0), c0
    eng = _engine(len(changed.docs), **caps)
    eng.apply(changed)
    _check(eng, _wants(changed, False), case)
    _check(eng, wants, f"{case} against the plain batch's oracle", docs=range(n))
    _same(eng, _kept(e0, n), f"{case} against the plain run")
    c = eng.launch_counts()
    print(f"{case}: census {c}")
    family = ("LDS_DL", "HBM_DL") if case.endswith("DL") else ("LDS_X", "HBM_X")
    assert c[case] > 0 and c["launches"] == sum(c[k] for k in family), c
    assert c["global_mode"] == c[family[1]] and (c["global_mode"] == 0) == small, c
    if case.endswith("DL"):
        assert len(eng.deltas(n // 2)) == 1
