// apply_run.hip -- the apply run, the host side of the hot path: every mtr_run, mtr_generate* and mtr_replay_pipelined
// goes through mtr::apply_run.  Four pieces, each readable alone:
//   RunKnobs       the once-per-process tuning knobs of the environment
//   plan_launch    the launch policy of one size class: pure arithmetic on its counters and the batch's traits
//   ApplyRun       the round scheduler: document groups, launch lanes, classify -> one launch per class -> classify ...
//   PipeSummaries  the summaries stage of mtr_replay_pipelined and mtr_replay_handover: a part is sized and written once
//                  it is done, then downloaded -- or hashed, classified and gathered, and its new blobs alone downloaded
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mtr.h"
#include "apply.hip.h"
#include "engine.hip.h"

using namespace mtr;

// ------------------------------------------------------------------ small kernels
// dst[i] = src ? src[i] : 0 for i < n (one block): zeroing and reading back small counters without a DMA copy
__global__ void words_kernel(int32_t* dst, const int32_t* src, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src ? src[i] : 0;
    __threadfence_system();
}

// dst[i] = src[i] for i < n, 64-bit words (summary sizes to mapped host memory, offsets back)
__global__ void words64_kernel(int64_t* dst, const int64_t* src, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[i];
    __threadfence_system();
}

// Size classes for one apply round: documents with ops left are bucketed by leaf count (64-leaf
// classes) so that each class launch sizes its LDS by its own largest document.
// cls layout: [0] max remaining ops, then per class c: cnt[c] at 1+3c, max nseg at 2+3c, max heapn at 3+3c.
// Classes [kClasses, 2 kClasses) hold matrix pairs (rows vector documents), classed by the larger
// of the two vectors; they launch apply_pair_kernel with two LDS regions.
constexpr int kClasses = 64;
constexpr int kAllClasses = 2 * kClasses;
__global__ void __launch_bounds__(256) classify_kernel(const DocHdr* h, const mtr_doc_desc* docs, uint32_t lo,
                                                      uint32_t hi, const uint32_t* dkind, const uint32_t* dpart,
                                                      int32_t* cls, uint32_t* list, int class_leaves,
                                                      int32_t* pleft = nullptr, const uint32_t* plo = nullptr,
                                                      uint32_t pparts = 0) {
    // block-local histogram in LDS, then one global atomic per (block, class): the per-document
    // atomics on a handful of addresses would serialise at the memory side
    __shared__ int lcnt[kAllClasses], lmax[kAllClasses], lheap[kAllClasses], lbase[kAllClasses];
    __shared__ int lrem;
    const int t = threadIdx.x;
    if (t < kAllClasses) lcnt[t] = lmax[t] = lheap[t] = 0;
    if (t == 0) lrem = 0;
    __syncthreads();
    // (documents [lo, hi): one group of the round loop; its class lists are [class][hi - lo])
    const uint32_t n = hi - lo;
    const uint32_t d = lo + blockIdx.x * blockDim.x + t;
    int c = -1, rank = 0;
    if (d < hi) {
        const DocHdr x = h[d];
        const int rem = x.status == MTR_OK ? int(docs[d].op_count) - x.op_cursor : 0;
        if (rem > 0) {
            int nseg = x.nseg, heapn = max(x.heapn, x.heap_need), base = 0;
            if (dkind[d] == 1) {
                const DocHdr y = h[dpart[d]];
                nseg = max(nseg, y.nseg);
                heapn = max(heapn, max(y.heapn, y.heap_need));
                base = kClasses;
            }
            c = base + min(kClasses - 1, nseg / class_leaves);
            rank = atomicAdd(&lcnt[c], 1);
            atomicMax(&lmax[c], nseg);
            atomicMax(&lheap[c], heapn);
            atomicMax(&lrem, rem);
            if (pleft) {  // (a pipelined run: this document's part still has ops left)
                uint32_t pp = 0;  // the last part whose first document is <= d
                for (uint32_t step = 1u << (31 - __clz(int(pparts))); step > 0; step >>= 1)
                    if (pp + step < pparts && plo[pp + step] <= d) pp += step;
                if (!pleft[pp]) atomicOr(&pleft[pp], 1);
            }
        }
    }
    __syncthreads();
    if (t < kAllClasses && lcnt[t]) {
        lbase[t] = atomicAdd(&cls[1 + 3 * t], lcnt[t]);
        atomicMax(&cls[2 + 3 * t], lmax[t]);
        atomicMax(&cls[3 + 3 * t], lheap[t]);
    }
    if (t == 0 && lrem) atomicMax(&cls[0], lrem);
    __syncthreads();
    if (c >= 0) list[size_t(c) * n + lbase[c] + rank] = d;
}

namespace {

int round64(int x) { return std::max(64, (x + 63) & ~63); }
int round32(int x) { return std::max(64, (x + 31) & ~31); }

// ------------------------------------------------------------------ the tuning knobs
// knob `name` clamped to [lo, hi], `absent` when the environment does not set it
int env_int(const char* name, int lo, int hi, int absent) {
    const char* v = std::getenv(name);
    return v ? std::max(lo, std::min(hi, std::atoi(v))) : absent;
}

// The environment's tuning knobs, read once per process (run_knobs).  MTR_PIPE_MIN_PART_DOCS and MTR_PIPE_GROUPS are
// not among them: mtr_replay_pipelined reads those on every call.
struct RunKnobs {
    // documents whose class needs more LDS than this stay HBM-resident (MTR_LDS_LIMIT, bytes; tuning knob)
    size_t lds_limit = [] {
        const char* v = std::getenv("MTR_LDS_LIMIT");
        return v ? std::min<size_t>(size_t(std::atoll(v)), 160 * 1024) : size_t(160 * 1024);
    }();
    // Size classes of `class_leaves` leaves (SharedString classes: LDS sized to the class's largest
    // document plus `slack` leaves; a document that runs out of room yields before the op and is
    // classed again next round).  Tuning knobs: MTR_CLASS_LEAVES, MTR_SLACK.
    int class_env = env_int("MTR_CLASS_LEAVES", 16, INT_MAX, 0);
    int slack_env = env_int("MTR_SLACK", 0, INT_MAX, -1);
    // concurrent launch lanes (1..kLanes) and whether the fixed-capacity kernels are used (tuning knobs:
    // MTR_LANES, MTR_NO_FIXED_CAP)
    int nlanes = env_int("MTR_LANES", 1, mtr_engine::kLanes, mtr_engine::kLanes);
    bool no_fixed_cap = std::getenv("MTR_NO_FIXED_CAP") != nullptr;
    // matrix pairs on one wave even when two could run them (tuning knob MTR_PAIR1)
    bool pair1 = std::getenv("MTR_PAIR1") != nullptr;
    bool ptrace = std::getenv("MTR_PIPE_TRACE") != nullptr;  // (host timeline of a pipelined run)
    // the LRU heap's floor in a yielding (tight) launch: cap / heap_div entries (tuning knob MTR_HEAP_DIV)
    int heap_div = env_int("MTR_HEAP_DIV", 1, INT_MAX, 8);
    // Independent document groups (tuning knob MTR_GROUPS, 1..kLanes): each group runs its own round loop
    // (classify -> one launch per size class -> classify ...) on its own streams, so one group's launches fill
    // the device while another's last documents of a round finish (a round is quantised by how many of its
    // documents the device holds at once).  SharedMatrix pairs keep one group.
    // Default: two groups for batches of 4,096 to 60,000 documents -- the 2- to 8-GPU shares of
    // C3 gain 5-10 % (profiles/r04_groups.json); above that one group (a round already fills the device), and
    // more than two leave each group too few lanes.
    int groups_env = env_int("MTR_GROUPS", 1, mtr_engine::kLanes, 0);
    // ops per launch of a pipelined run: twice the engine's -- while parts are landing a round holds few documents,
    // so its fixed costs (the launches' ramp and tail, the class read-back) weigh more per op; C3 end-to-end
    // 270.1 -> 264.3 ms at 96 against 48, the device-resident rate unchanged (profiles/r06_e2e_sweep.json)
    int pipe_k_env = env_int("MTR_PIPE_K", INT_MIN, INT_MAX, 0);
};

const RunKnobs& run_knobs() {
    static const RunKnobs k;
    return k;
}

// ------------------------------------------------------------------ the launch policy
struct ClassLoad {  // one size class's counters of this round (classify_kernel)
    int cnt, maxseg, maxheap;
};

struct BatchTraits {  // what the policy reads of the run, the batch and the device
    int gen;          // record mode
    int segcap, hcap;
    bool few_docs;    // no more documents than CUs
    bool has_ext, pend_seen, deltas;
    int dev_lds;
};

struct LaunchPlan {
    int cap, lhcap;  // leaf and LRU-heap capacity of the launch
    size_t lds;
    int global_mode;  // 1: HBM-resident
    int ops_this_launch;
    int variant;  // an ApplyVariant; -1: try the fixed-capacity kernels first, else AV_LDS_LEAN
    uint32_t region;  // a pair's LDS region
    bool stuck;       // no room and no larger LDS class
};

// The launch of one size class (`pair`: a matrix-pair class) with at most k ops per document.
LaunchPlan plan_launch(const ClassLoad& c, bool pair, int k, const BatchTraits& b, const RunKnobs& kn) {
    // replay launches of SharedString documents yield when their leaves or LRU heap could
    // overflow the launch's LDS, so they get `slack` leaves of room; matrix pairs (setCell
    // splits) and record mode (ops drawn once) keep room for every op of the launch
    const bool tight = !pair && !b.gen;
    // (a batch of fewer documents than CUs has LDS to spare: room for the whole launch, so a document
    // does not yield and wait for a round of its own)
    const int slack = kn.slack_env >= 0 ? kn.slack_env : (b.few_docs ? k + 8 : 8);
    int cap = tight ? round32(c.maxseg + slack + 8) : round64(c.maxseg + 2 * k + 8);
    // (a yielding launch above 1,024 leaves: the next multiple of 64, a capacity with a compile-time layout)
    if (tight && cap > 1024 && cap <= 1536) cap = round64(cap);
    if (cap > b.segcap) cap = b.segcap;
    // LRU heap: what the class holds now plus room for this launch's pushes; a document that
    // could overflow it stops before the op and asks for more (DocHdr.heap_need)
    // (matrix pairs replaying remote messages: a smaller floor -- a document whose op could overflow the heap
    // yields before it like any other, and two matrices of the larger classes then fit one CU's LDS)
    int lhcap = std::min<int>(b.hcap, pair && !b.gen ? std::max(cap / 16, round32(c.maxheap + 2 * k + 8))
                                       : std::max(cap / (tight ? kn.heap_div : 8),
                                                  tight ? round32(c.maxheap + slack + 8)
                                                        : round64(c.maxheap + 2 * k + 8)));
    size_t lds = lds_bytes(cap, lhcap, b.gen != 0);
    if (pair) lds = 2 * ((lds + 15) & ~size_t(15));
    const bool global_mode = lds > kn.lds_limit;
    if (global_mode) {
        // documents larger than LDS: leaves, heap and scan arrays stay in the HBM slab
        cap = b.segcap;
        lhcap = b.hcap;
        lds = lds_bytes_global_mode(b.segcap);
        if (pair) lds = 2 * ((lds + 15) & ~size_t(15));
    }
    const int kk = tight && !global_mode ? k : std::max(1, std::min(k, (cap - c.maxseg - 8) / 2));
    int av = -1;
    if (pair) {
        av = b.gen ? (global_mode ? AV_PAIR_HBM_GN : AV_PAIR_LDS_GN)  // record mode (mtr_generate_matrix)
             : b.deltas ? (global_mode ? AV_PAIR_HBM_DL : AV_PAIR_LDS_DL)  // a matrix tracked for its cells
             : (global_mode ? AV_PAIR_HBM : AV_PAIR_LDS);
        // replaying remote messages only: a wave per vector (run_pair2), if its exchange words fit
        if (!b.gen && !b.deltas && !b.has_ext && !b.pend_seen && !kn.pair1 &&
            lds + kPair2Xch <= size_t(std::max(b.dev_lds, 0))) {
            av = global_mode ? AV_PAIR2_HBM : AV_PAIR2_LDS;
            // (an LDS pair2 launch keeps no props arrays: remote messages only, Eng::NOPROPS)
            if (!global_mode) lds = 2 * ((lds_bytes(cap, lhcap, false, 7) + 15) & ~size_t(15));
            lds += kPair2Xch;
        }
    } else if (b.gen) {  // record mode: the generating instantiation
        av = global_mode ? AV_HBM_GN : AV_LDS_GN;
    } else if (b.deltas) {  // a batch with MTR_F_DELTA ops: the delta-reporting instantiation
        av = global_mode ? AV_HBM_DL : AV_LDS_DL;
    } else if (global_mode) {  // HBM-resident: the lean instantiation unless the batch has rare records
        av = b.has_ext ? AV_HBM_X : AV_HBM_LEAN;
    } else if (b.has_ext) {
        av = AV_LDS_X;
    } else if (kn.no_fixed_cap) {
        av = AV_LDS_LEAN;
    }
    const uint32_t region = !pair ? 0u : uint32_t((av == AV_PAIR2_LDS || av == AV_PAIR2_HBM ? lds - kPair2Xch : lds) / 2);
    return {cap, lhcap, lds, global_mode ? 1 : 0, kk, av, region, cap - c.maxseg - 8 < 2 && cap >= b.segcap};
}

// ------------------------------------------------------------------ the pipelined summaries stage
struct Trace {  // the host timeline of a pipelined run (MTR_PIPE_TRACE)
    bool on;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char* what, int a, int b) const {
        if (on)
            std::fprintf(stderr, "pipe %8.3f ms %s %d %d\n",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                         what, a, b);
    }
};

// pipelined summaries (mtr_replay_pipelined): a part whose documents have no ops left is summarized on the copy
// stream -- the size pass, its sizes read back into mapped memory, the offsets (parts in order), the write pass
// and the blobs' download into the caller's buffer -- while the other parts still apply.
// mtr_replay_handover (PipeRun::kHandover) keeps the records on the device and goes on behind the write pass: the
// part's blob table, ids, classify + state and scan (handover.hip's passes), their two read-backs through mapped words
// and an event like the sizes', then the gather of its first occurrences and the download of those bytes alone.
// Those passes carry a summary from part to part on the device -- the blob count, the summary's own id set, the chosen
// count and bytes -- so every one of them, the gathers and the downloads included, is issued in part order on the copy
// stream and on no other: a part's states and reps are final because no earlier part's pass can run after it.
struct PipeSummaries {
    mtr_engine* e;
    const Trace& trace;
    uint32_t PP = 0;          // the run's parts
    std::vector<int> pstate;  // per part: 0 applying, 1 done (pdone_ev recorded), 2 sizing, 3 downloading
    uint32_t next_size = 0, next_dl = 0;
    int64_t pbase = 0;
    // the hand-over: parts past their count / scan read-back, and what they have added up to (blobs, chosen, bytes)
    bool hand = false;
    uint32_t next_ids = 0, next_gather = 0;
    uint32_t blobs = 0, chosen = 0;
    int64_t bytes = 0;
    int rc = 0;  // a summary pass's error, sticky: no more passes, the apply runs out, then apply_run returns it

    int open(uint32_t parts) {
        PP = parts;
        e->summarized = false;
        e->drop_ids();
        hand = e->pipe.mode == mtr_engine::PipeRun::kHandover;
        if (summary_reserve(e) || e->out.ensure(size_t(e->pipe.cap) + 16) || e->pleft.ensure(PP) || e->h_pleft.ensure(PP) ||
            e->h_psize.ensure(e->n_docs) || e->pdone_ev.ensure(PP) || e->psize_ev.ensure(PP) || e->pwrite_ev.ensure(PP))
            return -1;
        pstate.assign(PP, 0);
        e->h_size.assign(e->n_docs, 0);
        e->h_off.assign(e->n_docs, 0);
        return 0;
    }
    // part p's documents are done with everything queued on `st` so far
    int part_done(uint32_t p, hipStream_t st) {
        HIPCHK(hipEventRecord(e->pdone_ev[p], st));
        pstate[p] = 1;
        return 0;
    }
    void step(bool apply_done) {
        if (!rc) rc = advance(apply_done);
    }
    void finish() {  // the last parts' summaries
        while (!rc && parts_out() < PP) {
            step(true);
            if (parts_out() < PP) std::this_thread::yield();
        }
    }
    uint32_t parts_out() const { return hand ? next_gather : next_dl; }  // parts whose last pass is issued
    // (the summary kernels run on the copy stream while the apply runs, on the idle engine stream once it is done,
    // so the last parts' passes do not queue behind the downloads)
    int advance(bool apply_done) {
        const mtr_engine::PipeRun& pr = e->pipe;
        hipStream_t ks = apply_done ? hipStream_t(e->stream) : pr.copy;
        while (next_size < PP && pstate[next_size] == 1) {  // size passes, parts in order
            const uint32_t p = next_size++, lo = pr.part_lo[p], hi = pr.part_lo[p + 1];
            HIPCHK(hipStreamWaitEvent(ks, e->pdone_ev[p], 0));
            if (summary_size_pass(e, lo, hi, ks)) return -1;
            words64_kernel<<<(hi - lo + 255) / 256, 256, 0, ks>>>(e->h_psize.dev + lo, e->out_size.p + lo, hi - lo);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(e->psize_ev[p], ks));
            pstate[p] = 2;
            trace("size", int(p), 0);
        }
        while (next_dl < next_size) {  // offsets, write pass, download, parts in order
            const hipError_t q = hipEventQuery(e->psize_ev[next_dl]);
            if (q == hipErrorNotReady) break;
            HIPCHK(q);
            const uint32_t p = next_dl++, lo = pr.part_lo[p], hi = pr.part_lo[p + 1];
            const int64_t base = pbase;
            for (uint32_t d = lo; d < hi; d++) {
                const int64_t z = e->h_psize.p[d];
                if (z < 0) {
                    set_err("document " + std::to_string(d) + " has more summary chunks than the engine's blob table");
                    return MTR_ERR_CAPACITY;
                }
                e->h_size[d] = z;
                e->h_off[d] = pbase;
                e->h_psize.p[d] = pbase;  // (the offsets go back through the same mapped words)
                pbase += z;
            }
            if (pbase > pr.cap) {
                // (the hand-over: cap is the device's record buffer, and the caller's buffers may still do --
                // mtr_replay_handover then takes the serial calls, unless the run fails for another reason)
                if (hand) e->hand.outgrown = true;
                set_err(std::string(hand ? "mtr_replay_handover: the device's record buffer holds "
                                         : "mtr_replay_pipelined: the output buffer holds ") +
                        std::to_string(pr.cap) + " bytes, the summaries need more");
                return MTR_ERR_CAPACITY;
            }
            words64_kernel<<<(hi - lo + 255) / 256, 256, 0, ks>>>(e->out_off.p + lo, e->h_psize.dev + lo, hi - lo);
            HIPCHK(hipGetLastError());
            if (summary_write_pass(e, lo, hi, ks)) return -1;
            if (ks != pr.copy) {
                HIPCHK(hipEventRecord(e->pwrite_ev[p], ks));
                HIPCHK(hipStreamWaitEvent(pr.copy, e->pwrite_ev[p], 0));
            }
            if (hand) {
                if (handover_count_pass(e, p, lo, hi, pr.copy)) return -1;
                pstate[p] = 3;
                trace("count", int(p), 0);
                continue;
            }
            if (pbase > base)
                HIPCHK(hipMemcpyAsync(pr.out + base, e->out.p + base, size_t(pbase - base), hipMemcpyDeviceToHost, pr.copy));
            pstate[p] = 3;
            trace("download", int(p), int((pbase - base) >> 20));
        }
        return hand ? advance_handover() : 0;
    }
    int too_small() const {
        set_err("mtr_replay_handover: the output buffers hold " + std::to_string(e->pipe.hand_cap_blobs) + " blobs and " +
                std::to_string(e->pipe.hand_cap_bytes) + " bytes, the summary's blobs or its new bytes need more");
        return MTR_ERR_CAPACITY;
    }
    // the parts behind their write pass, in order: each read-back is checked against the caller's bounds before the
    // pass that writes by it is issued (the per-blob buffers and the compact buffer are sized by those bounds)
    int advance_handover() {
        const mtr_engine::PipeRun& pr = e->pipe;
        for (; next_ids < next_dl; next_ids++) {  // the blob count is back: ids, classify + state, scan
            const hipError_t q = hipEventQuery(e->hand.count_ev[next_ids]);
            if (q == hipErrorNotReady) break;
            HIPCHK(q);
            const uint32_t p = next_ids;
            const int64_t* w = e->hand.words.p + 4 * size_t(p);
            if (w[1]) {
                set_err("mtr_replay_handover: a summary record's blob lengths do not add up to its size");
                return -1;
            }
            if (w[0] > pr.hand_cap_blobs) return too_small();
            const uint32_t b0 = blobs;
            blobs = uint32_t(w[0]);
            if (handover_ids_pass(e, p, pr.part_lo[p], pr.part_lo[p + 1], b0, blobs, pr.copy)) return -1;
            pstate[p] = 4;
            trace("ids", int(p), int(blobs - b0));
        }
        for (; next_gather < next_ids; next_gather++) {  // the chosen count and bytes are back: gather, download
            const hipError_t q = hipEventQuery(e->hand.scan_ev[next_gather]);
            if (q == hipErrorNotReady) break;
            HIPCHK(q);
            const uint32_t p = next_gather;
            const int64_t* w = e->hand.words.p + 4 * size_t(p);
            if (w[2] > int64_t(blobs) || w[3] > pr.hand_cap_bytes || (w[3] > 0 && !pr.hand_out)) return too_small();
            const uint32_t j0 = chosen;
            const int64_t o0 = bytes;
            chosen = uint32_t(w[2]);
            bytes = w[3];
            if (handover_gather_pass(e, p, j0, chosen, uint64_t(o0), uint64_t(bytes), pr.copy)) return -1;
            if (bytes > o0) {
                HIPCHK(hipMemcpyAsync(pr.hand_out + o0, e->novel.res.compact.p + o0, size_t(bytes - o0),
                                      hipMemcpyDeviceToHost, pr.copy));
                e->hand.copied += double(bytes - o0);
            }
            pstate[p] = 5;
            trace("gather", int(p), int((bytes - o0) >> 10));
        }
        return 0;
    }
    // after the run (the copy stream is idle): the parts' device times, and the ids and the novel result stand
    int commit_handover() {
        double t_ids = 0, t_novel = 0;
        for (uint32_t p = 0; p < PP; p++) {
            float a = 0, b = 0, c = 0;
            const Events& ev = e->hand.ev;
            HIPCHK(hipEventElapsedTime(&a, ev[5 * size_t(p)], ev[5 * size_t(p) + 1]));
            HIPCHK(hipEventElapsedTime(&b, ev[5 * size_t(p) + 1], ev[5 * size_t(p) + 2]));
            HIPCHK(hipEventElapsedTime(&c, ev[5 * size_t(p) + 3], ev[5 * size_t(p) + 4]));
            t_ids += a;
            t_novel += double(b) + double(c);
        }
        e->hand.t_ids = t_ids;
        e->hand.t_novel = t_novel;
        handover_commit(e, blobs);
        return 0;
    }
};

// ------------------------------------------------------------------ the round scheduler
struct Grp {  // one document group: the documents [lo, hi) run their own round loop
    uint32_t lo = 0, hi = 0;
    bool done = false;
    uint32_t p_lo = 0, p_hi = 0, waited = 0;  // pipelined: its parts [p_lo, p_hi), [waited, p_hi) not waited for
};

struct ApplyRun {
    static constexpr size_t ncls = 1 + 3 * kAllClasses;  // class counters of one group (classify_kernel's layout)
    mtr_engine* const e;
    const RunKnobs& kn = run_knobs();
    const Trace trace{kn.ptrace};
    KParams P{};
    BatchTraits traits{};
    uint32_t PP = 0;    // (a pipelined hand-over: its parts still landing; a group takes whole parts)
    bool psum = false;  // ... and their summaries stream out behind them (mtr_replay_pipelined / _handover)
    int Kr = 0;         // ops per launch
    int G = 1, L = 1;   // document groups; lanes (streams) per group
    int class_leaves = 64;
    std::vector<Grp> grp;
    int left = 0;  // groups still applying
    bool stuck = false;
    PipeSummaries sums{e, trace};

    explicit ApplyRun(mtr_engine* eng) : e(eng) {}

    // stream index of group g's lane l.  A pipelined run uses all four streams whatever MTR_LANES says: the last
    // one is the copy stream, a launch lane again once every part has landed -- group 0's lanes are streams 0 (and 1
    // with two groups), group 1's stream 2 and then 3; one group: streams 0-2, then 3
    int lane_si(int g, int l) const {
        if (PP && G == 2) return g == 0 ? l : 2 + l;
        return PP ? l : g * L + l;
    }
    hipStream_t lane_stream(int g, int l) const {
        const int si = lane_si(g, l);
        return si == 0 ? hipStream_t(e->stream) : hipStream_t(e->aux[si - 1]);
    }
    // the lanes group g launches on this round
    int lanes_of(int g) const {
        if (!PP) return L;
        const int base = G == 2 ? (g == 0 ? 2 : 1) : int(mtr_engine::kLanes) - 1;
        if ((G == 2 && g == 0) || psum) return base;  // (the copy stream: group 1's second lane; summaries' stream)
        const hipError_t q = hipEventQuery(e->part_ev[e->pipe.last]);
        return q == hipSuccess ? base + 1 : base;
    }

    // the kernels' parameters of this batch
    int fill_params(int gen) {
        P.hdr = e->hdr.p;
        P.seg = e->seg.p;
        P.heap = e->heap.p;
        P.text = e->text.p;
        P.prop = e->prop.p;
        P.rm = e->rm.p;
        P.segcap = int(e->caps.max_segments);
        P.hcap = int(e->caps.heap_entries);
        P.tcap = int(e->caps.text_units);
        P.pcap = int(e->caps.prop_words);
        P.rcap = int(e->caps.remover_cells);
        P.rtab = e->rtab;
        P.new_length_calc = e->opt.new_length_calc;
        P.n_docs = e->n_docs;
        P.ops = e->ops.p;
        P.docs = e->docs.p;
        P.btext = e->btext.p;
        P.propop_off = e->propop_off.p;
        P.propop_kv = e->propop_kv.p;
        P.key_index = e->key_index.p;
        P.val_eq = e->val_eq.p;
        P.stat_ops = e->stat.p;
        P.delta = e->delta.p;
        P.doff = e->has_delta ? e->doff.p : nullptr;
        P.dkind = e->dkind.p;
        P.dpart = e->dpart.p;
        P.pend = e->pend.p;
        P.refs = e->refs.p;
        P.refcap = int(e->caps.ref_slots);
        P.gen = gen;
#ifdef MTR_PROF
        if (!e->prof.p) {
            if (e->prof.ensure(64)) return -1;
            HIPCHK(hipMemset(e->prof.p, 0, 64 * sizeof(unsigned long long)));
        }
        P.prof = e->prof.p;
#endif
        if (gen) {
            P.gen_cfg = e->gcfg;
            P.gen_grow = int32_t(e->ggrow);
            P.gen_state = e->gstate.p;
            P.gen_ops = e->ops.p;
            P.gen_text = e->btext.p;
        }
        traits = {gen, P.segcap, P.hcap, e->n_docs <= uint32_t(std::max(e->n_cu, 1)), e->has_ext, e->pend_seen,
                  P.doff != nullptr, e->dev_lds};
        return 0;
    }

    // how the batch is run: class width, ops per launch, the document groups and their lanes
    void choose_groups() {
        const int K = int(e->caps.ops_per_launch ? e->caps.ops_per_launch : 0x7fffffff);
        bool any_pair = false;
        for (uint32_t d = 0; d < e->n_docs && d < e->h_kind.size(); d++) any_pair = any_pair || e->h_kind[d] != 0;
        PP = P.gen ? 0u : e->pipe.parts;
        psum = PP && e->pipe.mode != mtr_engine::PipeRun::kNoSummaries;
        // (round 6: two groups at 100,000 documents too -- 424.4 M against 418.5 M ops/s on one box; the per-launch
        // roofline figure that kept one group there is no longer the headline, the step span is; a pipelined hand-over
        // keeps one group, whose lanes take the landing parts in order)
        const int g_want = kn.groups_env > 0 ? kn.groups_env : (e->n_docs >= 4096u && !e->pipe.parts ? 2 : 1);
        // Default class width: 128 leaves for the batches that run two groups (4,096 to 60,000 documents) -- half the
        // launches per round of 64-leaf classes, which at those sizes cost more than the wider classes' LDS spread
        // (profiles/r04_class_sweep.json: 12,500 documents 379.0 M vs 341.4 M ops/s, 25,000 395.5 M vs 385.0 M);
        // 64 above (100,000: 407.7 M vs 400.5 M) and below; 128 for matrix pairs too (C4: 46.7 M vs 38.9 M ops/s,
        // profiles/r04_sched_sweep.json)
        class_leaves = kn.class_env > 0 ? kn.class_env
                                        : (any_pair || (e->n_docs >= 4096u && e->n_docs <= 60000u) ? 128 : 64);
        Kr = !PP ? K : kn.pipe_k_env > 0 ? kn.pipe_k_env : int(std::min<int64_t>(2 * int64_t(K), 0x7fffffff));
        G = any_pair ? 1 : std::max(1, std::min<int>(g_want, int(e->n_docs)));
        if (PP) G = std::min<int>(int(e->pipe.groups), int(PP));
        L = std::max(1, kn.nlanes / G);
        grp.assign(size_t(G), Grp{});
        for (int g = 0; g < G; g++) {
            Grp& gr = grp[size_t(g)];
            if (PP) {  // (mtr_submit_pipelined's split: two groups take [0, half) and [half, PP))
                const uint32_t half = (PP + 1) / 2;
                gr.waited = G == 2 && g == 1 ? half : 0u;
                gr.p_lo = gr.waited;
                gr.p_hi = G == 2 && g == 0 ? half : PP;
                gr.lo = e->pipe.part_lo[gr.waited];
                gr.hi = e->pipe.part_lo[gr.p_hi];
            } else {
                gr.lo = uint32_t(uint64_t(e->n_docs) * uint64_t(g) / uint64_t(G));
                gr.hi = uint32_t(uint64_t(e->n_docs) * uint64_t(g + 1) / uint64_t(G));
            }
        }
        left = G;
    }

    // buffers, the lanes' fork from the engine stream, and every group's first classify
    int start() {
        if (e->cls.ensure(ncls * mtr_engine::kLanes) || e->dlist.ensure(size_t(kAllClasses) * e->n_docs) ||
            e->h_cls.ensure(ncls * mtr_engine::kLanes))
            return -1;
        // the groups' lanes start after everything queued on the engine stream (the batch upload)
        HIPCHK(hipEventRecord(e->ev[0], e->stream));
        if (PP) {
            for (int si = 1; si < int(mtr_engine::kLanes); si++) HIPCHK(hipStreamWaitEvent(e->aux[si - 1], e->ev[0], 0));
        } else {
            for (int g = 0; g < G; g++)
                for (int l = 0; l < L; l++)
                    if (g * L + l > 0) HIPCHK(hipStreamWaitEvent(lane_stream(g, l), e->ev[0], 0));
        }
        if (psum && sums.open(PP)) return -1;
        HIPCHK(hipEventRecord(e->ev[1], e->stream));  // (timing start: after the forks above)
        for (int g = 0; g < G; g++)
            if ((PP && wait_part(g)) || classify(g)) return -1;
        return 0;
    }

    // classify group g (on its first lane) and read its class counts back
    int classify(int g) {
        Grp& gr = grp[size_t(g)];
        // (pipelined summaries: the parts that have landed by now count as waited for -- this classify sees all
        // of their documents, so a part it finds with no ops left is done)
        if (psum)
            while (gr.waited < gr.p_hi && hipEventQuery(e->part_ev[gr.waited]) == hipSuccess) gr.waited++;
        hipStream_t st = lane_stream(g, 0);
        int32_t* dcls = e->cls.p + size_t(g) * ncls;
        // (the counters are zeroed and read back by kernels, the read-back into mapped page-locked memory: a DMA
        // copy would queue behind mtr_submit_pipelined's uploads on the copy engine)
        words_kernel<<<1, 256, 0, st>>>(dcls, nullptr, int(ncls));
        if (psum) words_kernel<<<1, 256, 0, st>>>(e->pleft.p + gr.p_lo, nullptr, int(gr.p_hi - gr.p_lo));
        const uint32_t n = gr.hi - gr.lo;
        classify_kernel<<<(n + 255) / 256, 256, 0, st>>>(e->hdr.p, e->docs.p, gr.lo, gr.hi, e->dkind.p, e->dpart.p,
                                                         dcls, e->dlist.p + size_t(kAllClasses) * gr.lo, class_leaves,
                                                         psum ? e->pleft.p : nullptr, e->dpart_lo.p, PP);
        words_kernel<<<1, 256, 0, st>>>(e->h_cls.dev + size_t(g) * ncls, dcls, int(ncls));
        if (psum) words_kernel<<<1, 256, 0, st>>>(e->h_pleft.dev + gr.p_lo, e->pleft.p + gr.p_lo, int(gr.p_hi - gr.p_lo));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->grp_cls[g], st));
        return 0;
    }

    // HBM-resident launches need the scratch / chunk-record buffers: allocated by the first such launch
    int ensure_global() {
        if (e->scratch.ensure(size_t(e->n_docs) * 2 * P.segcap)) return -1;
        if (!e->csum.p) {  // for every document the engine may hold: it must never move
            const size_t n = size_t(std::max<uint32_t>(e->max_docs, 1)) * csum_ints(int(P.segcap));
            if (e->csum.ensure(n)) return -1;
            if (e->umap.ensure(size_t(std::max<uint32_t>(e->max_docs, 1)) * 2 * size_t(P.segcap))) return -1;
            HIPCHK(hipMemsetAsync(e->umap.p, 0xff, e->umap.n * sizeof(int32_t), e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
        }
        return 0;
    }

    // one round of group g: a launch per size class, spread over the group's lanes, joined on its first lane
    int issue_round(int g) {
        const Grp& gr = grp[size_t(g)];
        const int Lr = lanes_of(g);
        const int32_t* cls = e->h_cls.p + size_t(g) * ncls;
        const uint32_t n = gr.hi - gr.lo;
        const int k = std::min(Kr, cls[0]);
        hipStream_t st0 = lane_stream(g, 0);
        HIPCHK(hipEventRecord(e->grp_fork[g], st0));
        int nl = 0;  // launches of this round
        for (int c = kAllClasses - 1; c >= 0; c--) {  // one launch per size class: matrix pairs, then the
            const bool pair = c >= kClasses;              // SharedString classes, largest documents first
            const ClassLoad load{cls[1 + 3 * c], cls[2 + 3 * c], cls[3 + 3 * c]};
            if (load.cnt <= 0) continue;
            const LaunchPlan pl = plan_launch(load, pair, k, traits, kn);
            KParams Q = P;
            Q.global_mode = pl.global_mode;
            if (pl.global_mode) {
                if (ensure_global()) return -1;
                Q.csum = e->csum.p;
                Q.umap = e->umap.p;
                Q.scratch = e->scratch.p;
            }
            stuck = stuck || pl.stuck;
            Q.cap = pl.cap;
            Q.lhcap = pl.lhcap;
            Q.ops_this_launch = pl.ops_this_launch;
            Q.doc_list = e->dlist.p + size_t(kAllClasses) * gr.lo + size_t(c) * n;
            Q.n_launch = uint32_t(load.cnt);
            const int lane = nl % Lr;
            hipStream_t st = lane_stream(g, lane);
            if (lane != 0 && nl < Lr) HIPCHK(hipStreamWaitEvent(st, e->grp_fork[g], 0));
            const size_t q = size_t(e->launches);
            if (e->kev.ensure(2 * (q + 1))) return -1;
            HIPCHK(hipEventRecord(e->kev[2 * q], st));
            int av = pl.variant;
            if (av < 0 && !launch_fixed_cap_p0(pl.cap, Q.n_launch, pl.lds, st, Q) &&
                !launch_fixed_cap_p1(pl.cap, Q.n_launch, pl.lds, st, Q) &&
                !launch_fixed_cap_p2(pl.cap, Q.n_launch, pl.lds, st, Q))
                av = AV_LDS_LEAN;  // above the fixed classes: runtime layout, lean
            if (av >= 0 && !launch_variant(av, Q.n_launch, pl.lds, st, Q, pl.region)) {
                set_err("no apply kernel variant " + std::to_string(av));
                return -1;
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(e->kev[2 * q + 1], st));
            {  // the launch census (mtr_debug_launch_counts); av < 0: a fixed-capacity kernel took the launch
                mtr_engine::Census& cs = e->census;
                if (av >= 0) cs.variant[av]++;
                else cs.fixed_cap++;
                cs.global_mode += pl.global_mode;
                cs.min_cap = cs.min_cap ? std::min<int64_t>(cs.min_cap, pl.cap) : pl.cap;
                cs.max_cap = std::max<int64_t>(cs.max_cap, pl.cap);
                if (!pl.global_mode) cs.max_lds_cap = std::max<int64_t>(cs.max_lds_cap, pl.cap);
            }
            e->launches++;
            nl++;
        }
        for (int l = 1; l < std::min(nl, Lr); l++) {  // join the lanes
            const int si = lane_si(g, l);
            HIPCHK(hipEventRecord(e->lane_done[si], lane_stream(g, l)));
            HIPCHK(hipStreamWaitEvent(st0, e->lane_done[si], 0));
        }
        return 0;
    }

    // pipelined: a group classifies again once the next of its parts has landed (its lane 0 waits for it)
    int wait_part(int g) {
        Grp& gr = grp[size_t(g)];
        HIPCHK(hipStreamWaitEvent(lane_stream(g, 0), e->part_ev[gr.waited], 0));
        gr.waited++;
        return 0;
    }

    // every group's rounds, as its class counts come back, until no document has ops left (or one is stuck)
    int loop() {
        while (left > 0) {
            bool progressed = false;
            for (int g = 0; g < G; g++) {
                Grp& gr = grp[size_t(g)];
                if (gr.done) continue;
                const hipError_t q = hipEventQuery(e->grp_cls[g]);
                if (q == hipErrorNotReady) continue;
                HIPCHK(q);
                progressed = true;
                const int32_t* cls = e->h_cls.p + size_t(g) * ncls;
                if (psum) {  // parts classified after they landed with no ops left: done (before this round's launches)
                    for (uint32_t p = gr.p_lo; p < gr.waited; p++)
                        if (sums.pstate[p] == 0 && e->h_pleft.p[p] == 0) {
                            if (sums.part_done(p, lane_stream(g, 0))) return -1;
                            trace("done", int(p), g);
                        }
                }
                if (cls[0] <= 0) {
                    if (PP && gr.waited < gr.p_hi) {  // more of the group's documents are still landing
                        if (wait_part(g) || classify(g)) return -1;
                        continue;
                    }
                    gr.done = true;
                    trace("group-done", g, 0);
                    left--;
                    continue;
                }
                trace("round", g, cls[0]);
                if (issue_round(g)) return -1;
                if (stuck) break;
                if (classify(g)) return -1;  // queued behind the round's launches
            }
            if (stuck) break;
            if (psum) sums.step(left == 0);
            if (!progressed) std::this_thread::yield();
        }
        if (psum && !stuck) sums.finish();
        for (int g = 1; g < G; g++) {  // join every group into the engine stream
            HIPCHK(hipEventRecord(e->lane_done[lane_si(g, 0)], lane_stream(g, 0)));
            HIPCHK(hipStreamWaitEvent(e->stream, e->lane_done[lane_si(g, 0)], 0));
        }
        return 0;
    }
};

}  // namespace

int mtr::apply_run(mtr_engine* e, int gen) {
    struct ClearPipe {  // the hand-over is this run's alone, however the run ends
        mtr_engine* e;
        ~ClearPipe() { e->pipe = {}; }
    } clear_pipe{e};
    HIPCHK(hipSetDevice(e->device));
    if (e->n_docs == 0) return MTR_OK;
    e->launches = 0;
    e->t_apply = 0;
    e->t_kernels = 0;
    ApplyRun r(e);
    if (r.fill_params(gen)) return -1;
    r.choose_groups();
    if (r.start() || r.loop()) return -1;
    HIPCHK(hipEventRecord(e->ev[2], e->stream));
    HIPCHK(hipEventSynchronize(e->ev[2]));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->ev[1], e->ev[2]));
    e->t_apply += ms;
    for (size_t q = 0; q < size_t(e->launches); q++) {
        float kms = 0;
        HIPCHK(hipEventElapsedTime(&kms, e->kev[2 * q], e->kev[2 * q + 1]));
        e->t_kernels += kms;
    }
    if (r.PP) {  // the parts' op-scan bits: a part holding records the pipelined path does not run was not started
        HIPCHK(hipStreamSynchronize(e->pipe.copy));
        r.trace("end", r.sums.rc, 0);
        for (uint32_t p = 0; p < r.PP; p++)
            if (e->h_pflags.p[p]) {
                e->hand.outgrown = false;  // (the batch is not applied in full: nothing continues this run)
                set_err("mtr_submit_pipelined: documents " + std::to_string(e->pipe.part_lo[p]) + ".." +
                        std::to_string(e->pipe.part_lo[p + 1]) + " hold records beyond remote ops (MTR_F_DELTA, local ops, "
                        "local references or rare records); mtr_reset and submit the batch with mtr_submit");
                return MTR_ERR_UNSUPPORTED;
            }
        if (r.sums.rc) return r.sums.rc;  // (a summary pass's error: the batch is applied, the summaries are not built)
        if (r.psum && !r.stuck) {
            e->out_total = r.sums.pbase;
            e->drop_ids();
            e->summarized = true;
            // (the hand-over has hashed and classified every blob on the way: its ids and novel result are the summary's)
            if (r.sums.hand) return r.sums.commit_handover() ? -1 : MTR_OK;
        }
    }
    if (r.stuck) {
        set_err("document exceeds the leaf capacity");
        return MTR_ERR_CAPACITY;
    }
    if (!r.psum) e->summarized = false;
    e->drop_ids();
    return MTR_OK;
}
