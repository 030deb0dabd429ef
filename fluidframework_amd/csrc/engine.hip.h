// engine.hip.h -- internal to the engine's host translation units (mtr_engine.hip, apply_run.hip, handover.hip): the
// engine struct and the types that own its HIP resources.  Every buffer, event and stream of an engine is a member that
// frees itself, so mtr_engine_destroy is: set the device, synchronize the streams, delete.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mtr.h"
#include "../../include/mtr_synth.h"

namespace mtr {

struct DocHdr;   // apply.hip.h
struct KParams;  // apply.hip.h

void set_err(const std::string& s);  // (the thread's mtr_last_error text, mtr_engine.hip)

#define HIPCHK(x)                                                                  \
    do {                                                                           \
        hipError_t _e = (x);                                                       \
        if (_e != hipSuccess) {                                                    \
            set_err(std::string(#x) + ": " + hipGetErrorString(_e));               \
            return -1;                                                             \
        }                                                                          \
    } while (0)

// bytes currently held by every DevBuf and HostBuf of the process (mtr_debug_live_bytes)
inline std::atomic<int64_t> g_live_bytes{0};

// device memory, grow-only: ensure(n) keeps the buffer when it already holds n elements, else replaces it (the
// contents are not kept).  swap() is how a buffer is replaced by one that was filled beside it: a local takes the old
// one away with its scope, and every allocation stays counted once.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
    }
    int ensure(size_t want) {
        if (want <= n && p) return 0;
        release();
        const size_t bytes = std::max<size_t>(want, 1) * sizeof(T);
        if (hipMalloc(&p, bytes) != hipSuccess) {
            p = nullptr;
            set_err("hipMalloc failed for " + std::to_string(bytes) + " bytes");
            return -1;
        }
        n = std::max<size_t>(want, 1);
        g_live_bytes += int64_t(bytes);
        return 0;
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            g_live_bytes -= int64_t(n * sizeof(T));
        }
        p = nullptr;
        n = 0;
    }
};

// page-locked host memory, grow-only like DevBuf; the hipHostMalloc flags are fixed at construction, and a mapped
// buffer (hipHostMallocMapped) carries the address kernels write it by
template <class T>
struct HostBuf {
    T* p = nullptr;
    T* dev = nullptr;  // the device's address of p (mapped buffers only)
    size_t n = 0;
    const unsigned flags;
    explicit HostBuf(unsigned f) : flags(f) {}
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() { release(); }
    int ensure(size_t want) {
        if (want <= n && p) return 0;
        release();
        const size_t bytes = std::max<size_t>(want, 1) * sizeof(T);
        if (hipHostMalloc((void**)&p, bytes, flags) != hipSuccess) {
            p = nullptr;
            set_err("hipHostMalloc failed for " + std::to_string(bytes) + " bytes");
            return -1;
        }
        n = std::max<size_t>(want, 1);
        g_live_bytes += int64_t(bytes);
        if (flags & hipHostMallocMapped) HIPCHK(hipHostGetDevicePointer((void**)&dev, p, 0));
        return 0;
    }
    void release() {
        if (p) {
            (void)hipHostFree(p);
            g_live_bytes -= int64_t(n * sizeof(T));
        }
        p = dev = nullptr;
        n = 0;
    }
};

// events with one set of creation flags: a fixed group (ensure(k) once) or a list that grows with the work
struct Events {
    std::vector<hipEvent_t> v;
    const unsigned flags;
    explicit Events(unsigned f = hipEventDefault) : flags(f) {}
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
    ~Events() {
        for (hipEvent_t x : v) (void)hipEventDestroy(x);
    }
    int ensure(size_t want) {
        while (v.size() < want) {
            hipEvent_t x;
            HIPCHK(hipEventCreateWithFlags(&x, flags));
            v.push_back(x);
        }
        return 0;
    }
    hipEvent_t operator[](size_t i) const { return v[i]; }
};

// a non-blocking stream; reads as the hipStream_t it owns
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    int create() {
        HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return 0;
    }
    operator hipStream_t() const { return s; }
};

// ---- the summary hand-over's state (handover.hip), one struct per group; each group's events are made at first use

// git blob ids of the summary blobs (mtr_summary_blob_ids): hashed for every document on the first call after a
// summary, kept until the next call that rewrites `out` or clears `summarized`
struct BlobIds {
    DevBuf<uint32_t> first;  // [n_docs + 2]: each document's first blob, the count, a malformed-record flag
    DevBuf<uint64_t> boff;   // per blob: byte offset in `out`
    DevBuf<uint32_t> blen;   // per blob: length
    DevBuf<uint32_t> ids;    // per blob: the 20 id bytes
    int64_t count = -1;      // blobs of the current summary, -1 = ids not computed
    double t = 0;            // device time of the last id computation (table kernels + id kernel)
};

// mtr_git_blob_ids: the caller's bytes and their table
struct RawIds {
    DevBuf<uint8_t> bytes;
    DevBuf<uint64_t> off;
    DevBuf<uint32_t> len, ids;
};

// incremental hand-over (mtr_summary_delta).  The baseline: blob ids keyed by (document, blob index), set by
// mtr_summary_set_baseline[_ids]; content-addressed, so it outlives batches, summaries and mtr_reset.
struct Baseline {
    DevBuf<uint32_t> first;  // [docs + 1]: each baseline document's first id
    DevBuf<uint32_t> ids;    // per baseline blob: the 20 id bytes
    uint32_t docs = 0;       // 0 = no baseline: every blob counts as changed
};

// What a flags-scan-gather pass over the current summary's blobs leaves on the device, built for every document at
// once and kept.  The engine holds one for the delta against the baseline (chosen = new or different; rebuilt on the
// first call after the summary or the baseline changed) and one inside Novel.
struct Compacted {
    DevBuf<uint8_t> flags;     // per blob: 1 = chosen
    DevBuf<uint64_t> off;      // [blobs + 1]: each blob's offset in `compact` (a blob that is not chosen is empty)
    DevBuf<uint32_t> rank;     // [blobs + 1]: the chosen blobs before each blob
    DevBuf<uint64_t> chg_off, chg_src, tot;  // the chosen blobs: offset in `compact`, offset in `out`; the totals
    DevBuf<uint8_t> compact;   // the chosen blobs back to back (+ 16 bytes: the gather's last store)
    Events ev;                 // [4], timed: around the scan (the delta: flags + scan), around the gather
    bool valid = false;
    float t_scan = 0, t_gather = 0;  // device time (ms) of the last build between ev[0] and ev[1], and of its gather
};

// git tree ids (mtr_summary_tree_ids / mtr_git_tree_ids, tree_id.hip): the host-made entries as uploaded (sorted),
// their per-tree ranges, and the work buffers.  Nothing is cached: the host's entries may differ from call to call.
struct TreeWork {
    DevBuf<mtr_tree_entry> x;
    DevBuf<uint32_t> x_first, off, out;
    DevBuf<uint8_t> body;  // the tree bodies back to back (+ 16 bytes: the id kernel's aligned loads)
    Events ev;             // [2], timed
    double t = 0;          // device time of the last tree-id computation (all its kernels)
};

// the blob-id cache (mtr_blob_cache_*, blob_cache.hip): the set of ids storage holds, under any path of any
// document -- the stand-in for SummaryTreeUploadManager's blobsShaCache.  Content-addressed like the baseline and
// independent of it: it outlives batches, summaries and mtr_reset; only the mtr_blob_cache_* calls change it.
struct BlobCache {
    DevBuf<uint32_t> ids;      // the distinct ids in the order they were first added, 5 words each (a trim alone removes)
    DevBuf<uint32_t> slots;    // [nslots] open addressing: entry index + 1, 0 = empty; at most half used
    uint32_t count = 0;        // entries of ids
    uint64_t nslots = 0;       // a power of two, 0 = no slot array yet
    DevBuf<uint32_t> in;       // the host's ids of one add / has call
    DevBuf<uint32_t> where, rank, tot;  // per source id: its slot, the new ids before it; their count
    DevBuf<uint8_t> isnew;     // per source id of an add: 1 = appended; per id of a has: 1 = held
    // the cache's life cycle (mtr_blob_cache_trim / _ages / _export / _import): when each entry was last referenced
    DevBuf<uint32_t> stamp;    // per entry of ids: the generation that last offered the id; grows with the table
    uint32_t gen = 0;          // acknowledged summaries so far (mtr_blob_cache_add_summary); clear resets it
    DevBuf<uint32_t> age;      // the host's ages of one import call
    DevBuf<uint8_t> keep;      // per entry of a trim: 1 = it stays
    DevBuf<uint32_t> newidx;   // [count + 1] per entry of a trim: the survivors before it
    DevBuf<unsigned long long> hist;  // [1024] age buckets, [1024] a trim_to search's count
    Events ev;                 // [6], timed: a trim's flags + scan, its compaction + rebuild; the age histogram
    double t_trim = 0, t_ages = 0;  // device time of the last trim (without its read-back) and of the last histogram
    // an empty cache at generation 0 that holds no device memory, work buffers included: every DevBuf above is named
    // here (tests/test_blob_cache_trim.py counts the live bytes); the events and the times stay
    void release() {
        for (DevBuf<uint32_t>* b : {&ids, &slots, &in, &where, &rank, &tot, &stamp, &age, &newidx}) b->release();
        for (DevBuf<uint8_t>* b : {&isnew, &keep}) b->release();
        hist.release();
        nslots = count = gen = 0;
    }
};

// the novel result of the current summary against the cache (mtr_summary_novel): built for every document on the
// first call after the summary or the cache changed, kept on the device.  Buffers of its own: a cached delta stays.
struct Novel {
    DevBuf<uint32_t> slots;    // the summary's own id set: smallest blob index + 1 per distinct id the cache lacks
    DevBuf<uint32_t> where;    // per blob: its slot there (kNoSlot: the cache holds the id)
    DevBuf<uint8_t> state;     // per blob: 0 held, 1 first occurrence, 2 repeats an earlier blob of the summary
    DevBuf<uint32_t> rep;      // per blob: the first occurrence's index (0xFFFFFFFF for state 0)
    Compacted res;             // chosen = state 1; its ev[0] is "classified", so its t_scan is the scan alone
    Events ev;                 // [1], timed: the start
    float t_classify = 0;      // device time (ms) of the last build's classify + state kernels
};

}  // namespace mtr

using mtr::DevBuf, mtr::DocHdr, mtr::Events, mtr::HostBuf, mtr::Stream;  // (the users are `using namespace mtr`)

struct mtr_engine {
    static constexpr unsigned kMapped = hipHostMallocMapped | hipHostMallocCoherent;

    mtr_options opt{};
    mtr_caps caps{};
    int32_t rtab = 64;  // remover-head table entries per document (power of two >= 2 * remover_cells)
    int device = 0;
    uint32_t max_docs = 0;
    Stream stream;
    Events ev;  // [4], timed
    // size-class launches of one apply round run concurrently: class i on lane[i % kLanes]
    // (lane 0 = `stream`), joined back into `stream` before the next round
    static constexpr int kLanes = 4;
    Stream aux[kLanes - 1];
    Events lane_done{hipEventDisableTiming};  // [kLanes]
    // per document group [kLanes]: round start, class counts read
    Events grp_fork{hipEventDisableTiming}, grp_cls{hipEventDisableTiming};
    Events kev;  // per-launch start/stop events (kernel durations)
    // persistent document state
    DevBuf<DocHdr> hdr;
    DevBuf<uint32_t> seg, heap, prop, rm;
    DevBuf<uint16_t> text;
    // current batch (device copies)
    uint32_t n_docs = 0;
    uint32_t max_ops_per_doc = 0;
    DevBuf<mtr_doc_desc> docs;
    DevBuf<mtr_op> ops;
    DevBuf<uint16_t> btext;
    DevBuf<uint32_t> propop_off, propop_kv, key_off, key_index, val_off, val_eq, client_off;
    DevBuf<uint8_t> key_bytes, val_bytes, client_bytes;
    DevBuf<unsigned long long> stat;  // [0] ops applied
    DevBuf<uint32_t> delta;           // delta ranges of the MTR_F_DELTA ops of the current batch
    DevBuf<uint64_t> doff;            // [doc + 1] record offsets into delta (exact per-batch bound)
    std::vector<uint64_t> h_doff;
    bool has_delta = false;
    bool has_ext = false;             // the batch holds rare records (op_scan_kernel): no fixed-capacity kernels
    bool pend_seen = false;           // a batch since mtr_reset held local ops while collaborating or acks:
                                      // documents may hold pending segments, so every launch is an X kernel
    DevBuf<uint32_t> pend;            // [doc][kPendRing][4] pending SegmentGroups (allocated on first use)
    int dev_lds = 0;                  // the device's LDS per workgroup (bytes; 0 = unknown)
    int n_cu = 0;                     // the device's compute units
    bool refs_seen = false;           // a batch since mtr_reset created local references: they follow splits,
                                      // appends and removals in the X kernels only, so every launch is one
    DevBuf<uint32_t> refs;            // [doc][3][ref_slots] local references (allocated on first use)
    DevBuf<int32_t> qbuf;             // query results (reference positions)
    DevBuf<int32_t> csum;             // [doc][csum_ints(segcap)] chunk records + superchunk rows (first HBM-resident launch)
    DevBuf<int32_t> umap;             // [doc][2 * segcap] uid -> slot hints (with csum)
    DevBuf<int32_t> red;              // small reduction / query-result buffer
    DevBuf<unsigned long long> prof;  // phase-timer sums (-DMTR_PROF builds)
    DevBuf<int32_t> cls;              // size-class counters of one apply round (classify_kernel)
    DevBuf<uint32_t> dlist;           // [class][n_docs] document lists of one apply round
    HostBuf<int32_t> h_cls{kMapped};  // mapped host copy of cls (written by words_kernel)
    DevBuf<uint32_t> scratch;         // E/V arrays for HBM-resident (global-mode) launches
    DevBuf<mtr_synth_state> gstate;   // record mode generator state
    // SharedMatrix pairs (mtr_set_matrix): per document kind (0 SharedString, 1 rows vector, 2 cols
    // vector) and partner; they survive mtr_reset
    DevBuf<uint32_t> dkind, dpart;
    std::vector<uint32_t> h_kind, h_part;
    mtr_synth_cfg gcfg{};
    uint32_t ggrow = 0;  // pre-grown records of the record-mode run in progress
    // summaries
    DevBuf<int64_t> out_size, out_off;
    DevBuf<uint8_t> s_kind;                       // summary scratch (size pass -> write pass)
    DevBuf<uint32_t> s_start, s_len, s_bytes, s_lb, s_fl, s_sid, s_bb;
    DevBuf<int32_t> s_blob;
    DevBuf<unsigned long long> out_hash;
    DevBuf<uint8_t> out;
    std::vector<int64_t> h_off, h_size;
    std::vector<uint32_t> h_val_eq;  // host copy for export hashes
    int64_t out_total = 0;
    bool summarized = false;
    // the summary hand-over (handover.hip), one value per group
    mtr::BlobIds ids;
    mtr::RawIds raw;
    mtr::Baseline base;
    mtr::Compacted summary_delta;  // (mtr_summary_delta; `delta` above is the apply side's)
    mtr::TreeWork tree;
    mtr::BlobCache cache;
    mtr::Novel novel;
    void drop_ids() {  // the summary records are gone or rewritten
        ids.count = -1;
        summary_delta.valid = false;
        novel.res.valid = false;
    }
    // pipelined hand-over: the batch mtr_submit_pipelined left for the next apply run, as one value.  That call fills
    // it; mtr_submit, mtr_reset and every exit of apply_run clear it, so no run sees another batch's parts.
    struct PipeRun {
        uint32_t parts = 0;             // 0 = no pipelined batch waits for its run
        uint32_t groups = 1;            // document groups of the run (their parts are uploaded alternately)
        uint32_t last = 0;              // the part uploaded last
        std::vector<uint32_t> part_lo;  // [parts + 1] the parts' first documents (+ n_docs)
        hipStream_t copy = nullptr;     // (= aux[kLanes - 2]: the last launch lane; not owned)
        // pipelined summaries (mtr_replay_pipelined): a part is summarized and downloaded into the caller's buffer
        // once its documents are done; null = the run builds no summaries
        uint8_t* out = nullptr;
        int64_t cap = 0;
        // what the summaries stage sends to the host: nothing, the records of every part (mtr_replay_pipelined: out /
        // cap above are the caller's), or the first occurrences of every part's blobs alone (mtr_replay_handover: cap is
        // what the device's record buffer holds, the caller's bounds follow)
        enum Mode { kNoSummaries, kRecords, kHandover } mode = kNoSummaries;
        uint8_t* hand_out = nullptr;  // the caller's buffer for the state-1 bytes, back to back
        int64_t hand_cap_bytes = 0, hand_cap_blobs = 0;
    } pipe;
    // mtr_replay_handover (handover.hip: the hand-over passes; apply_run.hip: the stage that issues them)
    struct Handover {
        HostBuf<int64_t> words{kMapped};  // per part [4]: the blobs so far, a malformed record; the chosen blobs, their bytes
        Events ev;                        // per part [5], timed: ids start, ids end, scan end; around the gather
        Events count_ev{hipEventDisableTiming}, scan_ev{hipEventDisableTiming};  // per part: its two read-backs
        double copied = 0;                // blob bytes the last hand-over sent to the host
        double t_ids = 0, t_novel = 0;    // summed device time (ms) of its parts' id passes; classify + scan + gather
        bool outgrown = false;            // the last run stopped because the records outgrew the device's buffer
        int64_t rec_want = 0;             // ... and the record bytes the next run's buffer is to hold (with headroom)
        bool ranges = false;              // the last hand-over ran its ranges (false: the serial calls inside)
    } hand;
    // batched position queries (mtr_get_containing_segments, query.hip): the work buffers of one call, grown on demand
    struct SegmentQueries {
        DevBuf<mtr_view_query> q;  // the queries as uploaded
        DevBuf<int32_t> rows;      // per query: Eng::containing's 11 result words
        DevBuf<uint64_t> len;      // [2 n]: text units per query, then property words per query
        DevBuf<int64_t> off;       // [2 n + 3]: their exclusive scans with totals, then the error flag
        DevBuf<int32_t> flag;      // a reference outside an arena (bits, query.hip)
        DevBuf<uint16_t> text;     // the queries' text units back to back
        DevBuf<uint32_t> props;    // the queries' property words back to back
        // position transforms (mtr_transform_positions): the queries as uploaded, one 16-byte row per query
        DevBuf<mtr_position_query> pq;
        DevBuf<mtr_position> pos;
    } squery;
    // batched reference queries (mtr_get_refs, query.hip): the work buffers of one call, grown on demand
    struct RefQueries {
        DevBuf<uint32_t> list;   // the listed documents as uploaded (unused for documents 0 .. n - 1)
        DevBuf<uint64_t> len;    // [2 n]: 64-reference blocks per listed document, then references
        DevBuf<int64_t> off;     // [2 n + 3]: their exclusive scans with totals, then the error flag
        DevBuf<int32_t> flag;    // a header that claims more references than the table holds
        DevBuf<uint32_t> work;   // per 64-reference block, two words: the listed index, the block in its document
        DevBuf<int32_t> words;   // the references' words back to back
    } rquery;
    // batched range queries (mtr_get_range_segments, query.hip): the work buffers of one call, grown on demand
    struct RangeQueries {
        DevBuf<mtr_range_query> q;  // the queries as uploaded
        DevBuf<uint64_t> cnt;       // [3 n]: segments per query, then text units, then property words
        DevBuf<int32_t> first;      // per query [4]: the first round holding a segment, the view's length and the live
                                    // leaves ahead of that round (where the write pass starts)
        DevBuf<int64_t> off;        // [3 n + 4]: the three exclusive scans with totals, then the error flag
        DevBuf<int32_t> flag;       // a reference outside an arena (bits, query.hip)
        DevBuf<int32_t> rows;       // per segment: Eng::leaf_row's 11 words
        DevBuf<int64_t> toff, poff; // per segment: its first unit / first word in the compact buffers
        DevBuf<uint16_t> text;      // the ranges' text units back to back
        DevBuf<uint32_t> props;     // the segments' property words back to back
    } range;
    // batched delta records (mtr_get_deltas_batch, query.hip): the work buffers of one call, grown on demand
    struct DeltaQueries {
        DevBuf<uint32_t> list;    // the listed documents as uploaded (unused for documents 0 .. n - 1)
        DevBuf<uint64_t> len;     // [2 n]: property words per listed document, then records
        DevBuf<int64_t> off;      // [2 n + 3]: their exclusive scans with totals, then the error flag
        DevBuf<int32_t> flag;     // a corrupted header, a reference outside the property arena (bits, query.hip)
        DevBuf<mtr_delta> recs;   // the listed documents' records back to back
        DevBuf<int64_t> poff;     // per record: its first word in `props`
        DevBuf<uint32_t> props;   // the records' property words back to back
    } dquery;
    // batched interval queries (mtr_query_intervals, query.hip): the work buffers of one call, grown on demand
    struct IntervalQueries {
        DevBuf<uint32_t> up;     // the one upload: the sets (4 words each), the queries, the keys kernel's work list
                                 // (set, block), the reference ids
        DevBuf<int32_t> keys;    // per endpoint of a 32-interval block, four words: position, key, offset, 0
        DevBuf<uint64_t> len;    // [2 n]: hits per query, then status words
        DevBuf<int64_t> off;     // [2 n + 3]: their exclusive scans with totals, then the flag word
        DevBuf<int32_t> flag;    // a reference id its document does not have, a corrupted header (query.hip)
        DevBuf<int32_t> work;    // per query [8]: the keys of its two positions, the PREVIOUS / NEXT answer, its ties
        DevBuf<mtr_interval_hit> hits;  // the queries' rows back to back
    } ivquery;
    // batched marker search (mtr_find_markers, query.hip): the work buffers of one call, grown on demand
    struct MarkerQueries {
        DevBuf<uint32_t> up;     // the one upload: the labels (3 words each), the value ids, the queries (6 words each)
        DevBuf<int32_t> rows;    // [6 n + 1]: per query its mtr_marker_hit, then the flag (a reference outside the
                                 // property arena)
        HostBuf<uint32_t> h_up{hipHostMallocDefault};   // page-locked staging of `up`
        HostBuf<int32_t> h_rows{hipHostMallocDefault};  // ... and of `rows`: nothing reaches the caller on an error
    } mkquery;
    // per part its landing event and op-scan bits (device, then page-locked host copy)
    Events part_ev{hipEventDisableTiming};
    DevBuf<int32_t> pflags;
    HostBuf<int32_t> h_pflags{hipHostMallocDefault};
    DevBuf<mtr_doc_desc> pdocs;  // the descriptors as uploaded (part_ready_kernel enables them)
    DevBuf<int32_t> pleft;             // per part: documents with ops left (classify_kernel)
    DevBuf<uint32_t> dpart_lo;         // the parts' first documents (+ n_docs), for classify_kernel
    HostBuf<int32_t> h_pleft{kMapped};  // (mapped copy of pleft)
    HostBuf<int64_t> h_psize{kMapped};  // per document: summary sizes read back, then offsets
    // per part: documents done, sizes read back, written
    Events pdone_ev{hipEventDisableTiming}, psize_ev{hipEventDisableTiming}, pwrite_ev{hipEventDisableTiming};
    // timing
    double t_apply = 0, t_summary = 0;
    double t_kernels = 0;  // sum of the apply launches' own durations (they overlap across lanes)
    int launches = 0;
    // launch census since create / mtr_reset (mtr_debug_launch_counts): launches per runtime-layout variant (enum
    // ApplyVariant), of the fixed-capacity kernels and HBM-resident, and the leaf capacities launched
    static constexpr int kCensusVariants = 16;
    struct Census {
        int64_t variant[kCensusVariants] = {};
        int64_t fixed_cap = 0, global_mode = 0;
        int64_t min_cap = 0, max_cap = 0, max_lds_cap = 0;  // (0: no launch yet)
    } census;
};

namespace mtr {

// The apply run (apply_run.hip): every round of size-class launches until no document of the batch has ops left;
// gen = record mode.  Behind mtr_run, mtr_generate_grown, mtr_generate_matrix, mtr_replay_pipelined and mtr_replay_handover.
int apply_run(mtr_engine* e, int gen);

// The summary passes over the documents [lo, hi) on stream s: the sizes into out_size; the records at out_off into
// `out`.  summary_reserve sizes their scratch for the batch, so that no pass allocates.  (mtr_engine.hip:
// summary.hip.h defines its kernels, so one unit alone includes it.)
int summary_reserve(mtr_engine* e);
int summary_size_pass(mtr_engine* e, uint32_t lo, uint32_t hi, hipStream_t s);
int summary_write_pass(mtr_engine* e, uint32_t lo, uint32_t hi, hipStream_t s);

// The hand-over passes of mtr_replay_handover's summaries stage (handover.hip), all asynchronous on stream s.  They
// continue one summary from part to part -- the blob table, the summary's own id set and the compaction carry on the
// device what the earlier parts left -- so the stage issues them part by part in document order on ONE stream.
// handover_reserve sizes every buffer they write from the caller's bounds, for n documents in `parts` parts, and zeroes
// the carried state on s, so that no pass allocates.  mtr_replay_handover calls it on the engine stream before the
// batch's uploads are queued: a buffer that is replaced frees device memory, which waits for the device, and the copy
// stream starts behind the engine stream's work.
//   count  the blob table of the part's documents [lo, hi); hand.words[4 p + 0 / 1] = blobs so far / malformed flag
//   ids    the part's blobs [b0, b1): offsets and lengths, ids, classify + state, the scan with carry;
//          hand.words[4 p + 2 / 3] = chosen blobs so far / their bytes
//   gather its chosen blobs [j0, j1) into the compact buffer at [o0, o1)
// The host checks every read-back against the caller's bounds before it issues the pass that writes by it.
// handover_commit marks the ids and the novel result of the finished summary as built (nb blobs).
int handover_reserve(mtr_engine* e, uint32_t n, uint32_t parts, int64_t cap_blobs, int64_t cap_bytes, hipStream_t s);
int handover_count_pass(mtr_engine* e, uint32_t p, uint32_t lo, uint32_t hi, hipStream_t s);
int handover_ids_pass(mtr_engine* e, uint32_t p, uint32_t lo, uint32_t hi, uint32_t b0, uint32_t b1, hipStream_t s);
int handover_gather_pass(mtr_engine* e, uint32_t p, uint32_t j0, uint32_t j1, uint64_t o0, uint64_t o1, hipStream_t s);
void handover_commit(mtr_engine* e, uint32_t nb);
// after the run: the whole summary's per-blob tables to the caller (ids 20 bytes a blob; the rest as mtr_summary_novel)
int handover_tables(mtr_engine* e, uint8_t* ids, uint8_t* state, int64_t* rep, int64_t* blob_off, int64_t* doc_first);

// The position queries (query.hip; mtr_get_containing_segment and the reference queries in mtr_engine.hip use both).
// query_params: the kernel parameters a query on the documents' HBM state needs (the state slabs and their
// capacities; nothing of a batch).  segment_info_from_row: Eng::containing's 11 result words of a query at `pos` as
// the mtr_segment_info the C ABI reports.
void query_params(const mtr_engine* e, KParams& P);
void segment_info_from_row(const int32_t* r, int32_t pos, mtr_segment_info* info);

// the calls over the documents [lo, hi) of the current summary start with this check; `fn` names the call
inline int summary_range(const mtr_engine* e, const char* fn, uint32_t lo, uint32_t hi) {
    if (e && e->summarized && hi <= e->n_docs && lo <= hi) return 0;
    set_err(std::string(fn) + ": bad range or no summary (call mtr_summarize first)");
    return -1;
}

}  // namespace mtr
