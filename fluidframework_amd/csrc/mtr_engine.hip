// mtr_engine.hip -- host side of the MI355X merge-tree replay engine: the C ABI of
// include/mtr.h, device memory management and kernel launches.
//
// Memory layout in HBM (one slab per document, sized by mtr_caps):
//   DocHdr                      64 B                  (collaboration window + arena cursors)
//   leaves  [NF][segcap] u32    len seq rseq meta text props uid   (SoA, tree order)
//   heap    [2][hcap]    u32    zamboni LRU heap (seq, uid), 1-based
//   text    [tcap]       u16    UTF-16 text arena (segments hold offsets)
//   props   [pcap]       u32    immutable property-set entries [n, k0, v0, ...]
//   removers[rcap]       u32    cons cells of overlapping removers (client<<24 | next), then the
//           [2*rtab]     u32    uid -> list head table (open addressing, key uid+1)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mtr.h"
#include "../../include/mtr_synth.h"
#include "apply.hip.h"
#include "engine.hip.h"
#include "summary.hip.h"

using namespace mtr;

namespace {

thread_local std::string g_err;

}  // namespace

// ------------------------------------------------------------------ small kernels
__global__ void reset_kernel(DocHdr* h, uint32_t n) {
    uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    DocHdr z{};
    z.height = 1;
    z.local = -1;
    z.fail_op = -1;
    h[d] = z;
}

__global__ void cursor_reset_kernel(DocHdr* h, const mtr_doc_desc* docs, uint32_t n) {
    uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < n) {
        h[d].op_cursor = 0;
        h[d].dused = 0;  // delta ranges are per batch
        // more short client ids than the engine's 8-bit client field holds: the document stays on
        // the TypeScript Client (MTR_MAX_CLIENTS)
        if (docs[d].n_clients > MTR_MAX_CLIENTS && h[d].status == MTR_OK) {
            h[d].status = MTR_ERR_UNSUPPORTED;
            h[d].fail_op = 0;
        }
    }
}

// mtr_submit_pipelined: the documents [lo, hi) of part p have landed; enable them (copy the descriptor, op_count
// last, after a fence: classify_kernel reads op_count and a launch the rest) unless the part's op scan found
// records the pipelined path does not run (they then never start; mtr_run reports MTR_ERR_UNSUPPORTED)
__global__ void part_ready_kernel(DocHdr* h, mtr_doc_desc* docs, const mtr_doc_desc* src, uint32_t lo, uint32_t hi,
                                  const int32_t* flags) {
    const uint32_t d = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= hi || *flags != 0) return;
    mtr_doc_desc x = src[d];
    h[d].op_cursor = 0;
    h[d].dused = 0;
    if (x.n_clients > MTR_MAX_CLIENTS && h[d].status == MTR_OK) {  // (cursor_reset_kernel's check)
        h[d].status = MTR_ERR_UNSUPPORTED;
        h[d].fail_op = 0;
    }
    const uint32_t cnt = x.op_count;
    x.op_count = 0;
    docs[d] = x;
    __threadfence();
    docs[d].op_count = cnt;
}

// bit 3: local-reference records (MTR_OP_REF_*, and an interval collection's MTR_OP_REBASE_POS / MTR_OP_LSEQ)
// bit 0: an op flagged MTR_F_DELTA (the host sizes delta buffers only then); bit 1: a rare record the
// fixed-capacity kernels do not carry (Eng::X: relative positions, handle-table loads, combining
// annotates, marker ordinals); bit 2: the local-op path (MTR_OP_ACK, or a local op recorded while
// collaborating: seq = UnassignedSequenceNumber)
__global__ void op_scan_kernel(const mtr_op* ops, uint64_t n, int32_t* out) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    bool any = false, ext = false, pend = false, refs = false;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const mtr_op op = ops[i];
        any = any || (op.flags & MTR_F_DELTA) != 0;
        refs = refs || op.type == MTR_OP_REF_CREATE || op.type == MTR_OP_REF_REMOVE || op.type == MTR_OP_REF_ACK ||
               op.type == MTR_OP_REBASE_POS || op.type == MTR_OP_LSEQ;
        pend = pend || op.type == MTR_OP_ACK || op.type == MTR_OP_ROLLBACK || op.type == MTR_OP_REGENERATE ||
               (op.type >= MTR_OP_LOCAL_INSERT && op.type <= MTR_OP_LOCAL_ANNOTATE && op.seq == -1);
        ext = ext || op.type == MTR_OP_RELPOS || op.type == MTR_OP_HANDLES || (op.flags & MTR_F_REL) ||
              op.type == MTR_OP_LOCAL_SETCELL ||
              (op.type == MTR_OP_ANNOTATE && op.payload2 != 0) ||
              ((op.flags & MTR_F_MARKER) && op.payload2 != 0 &&
               (op.type == MTR_OP_INSERT || op.type == MTR_OP_LOCAL_INSERT || op.type == MTR_OP_LOAD));
    }
    const int bits = (__ballot(any) ? 1 : 0) | (__ballot(ext) ? 2 : 0) | (__ballot(pend) ? 4 : 0) |
                     (__ballot(refs) ? 8 : 0);
    if (bits && (threadIdx.x & 63) == 0) atomicOr(out, bits);
}

// out[0] = max nseg, out[1] = max remaining ops, out[2] = max heapn
__global__ void scan_state_kernel(const DocHdr* h, const mtr_doc_desc* docs, uint32_t n, int32_t* out) {
    uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    const DocHdr x = h[d];
    atomicMax(&out[0], x.nseg);
    int rem = x.status == MTR_OK ? int(docs[d].op_count) - x.op_cursor : 0;
    atomicMax(&out[1], rem);
    atomicMax(&out[2], x.heapn);
}

// local-reference positions (or one reference's info) of a document's HBM state (mtr_get_ref_positions / _info)
__global__ void __launch_bounds__(NT) refs_kernel(KParams P, uint32_t d, int32_t* out, int info_id) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Eng<true>::ref_query(smem, P, d, out, info_id);
}

// one getContainingSegment query on a document's HBM state (mtr_get_containing_segment)
__global__ void __launch_bounds__(NT) containing_kernel(KParams P, uint32_t d, int pos, int ref, int client,
                                                        int32_t* out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Eng<true>::containing(smem, P, d, pos, ref, client, out);
}

template <class T>
static int upload(mtr_engine* e, DevBuf<T>& dst, const T* src, size_t n) {
    if (dst.ensure(n)) return -1;
    if (n) HIPCHK(hipMemcpyAsync(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice, e->stream));
    return 0;
}

// What mtr_submit and mtr_submit_pipelined share: the batch's extent (n_docs, max_ops_per_doc) and its tables (small).
static int upload_tables(mtr_engine* e, const mtr_batch* b) {
    e->n_docs = b->n_docs;
    uint32_t mx = 0;
    size_t ncl = 0;  // client-name offsets: one past the last client any document names
    for (uint32_t d = 0; d < b->n_docs; d++) {
        mx = std::max(mx, b->docs[d].op_count);
        ncl = std::max<size_t>(ncl, size_t(b->docs[d].client_base) + b->docs[d].n_clients);
    }
    ncl += 1;
    e->max_ops_per_doc = mx;
    const size_t nkv = b->n_propops ? size_t(b->propop_off[b->n_propops]) * 2 : 0;
    if (upload(e, e->propop_off, b->propop_off, size_t(b->n_propops) + 1) || upload(e, e->propop_kv, b->propop_kv, nkv) ||
        upload(e, e->key_off, b->key_off, size_t(b->n_keys) + 1) ||
        upload(e, e->key_bytes, b->key_bytes, b->n_keys ? size_t(b->key_off[b->n_keys]) : 0) ||
        upload(e, e->key_index, b->key_index, b->n_keys) || upload(e, e->val_off, b->val_off, size_t(b->n_vals) + 1) ||
        upload(e, e->val_bytes, b->val_bytes, b->n_vals ? size_t(b->val_off[b->n_vals]) : 0) ||
        upload(e, e->val_eq, b->val_eq, b->n_vals) || upload(e, e->client_off, b->client_off, ncl) ||
        upload(e, e->client_bytes, b->client_bytes, size_t(b->client_off[ncl - 1])))
        return -1;
    e->h_val_eq.assign(b->val_eq, b->val_eq + b->n_vals);
    return 0;
}

// A pipelined hand-over that never ran is dropped by the next submit or reset: whatever the engine stream does next
// waits for the uploads still on the copy stream (the last part's landing event is that stream's last work).
static int drop_pipe(mtr_engine* e) {
    if (e->pipe.parts) HIPCHK(hipStreamWaitEvent(e->stream, e->part_ev[e->pipe.last], 0));
    e->pipe = {};
    return 0;
}

void mtr::set_err(const std::string& s) { g_err = s; }

// mtr_engine_create's device side: the streams, the fixed events and the documents' slabs.  Whatever it has made when
// it fails is the engine's to free.
static int engine_open(mtr_engine* e) {
    const mtr_caps& c = e->caps;
    if (hipSetDevice(e->device) != hipSuccess || e->stream.create()) {
        set_err("cannot open HIP device " + std::to_string(e->device));
        return -1;
    }
    {  // HBM-resident launches (and the query kernels) still keep per-chunk rows in LDS: about segcap / 8
       // bytes (twice for a matrix pair: mtr_set_matrix checks that) -- a capacity whose rows exceed the device's
       // LDS is refused here rather than failing every later launch with a generic HIP error
        int dev_lds = 0;
        if (hipDeviceGetAttribute(&dev_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, e->device) != hipSuccess) dev_lds = 0;
        e->dev_lds = dev_lds;
        const size_t need = (lds_bytes_global_mode(int(c.max_segments)) + 15) & ~size_t(15);
        if (dev_lds > 0 && need > size_t(dev_lds)) {
            set_err("mtr_engine_create: max_segments " + std::to_string(c.max_segments) + " needs " +
                    std::to_string(need) + " bytes of LDS in HBM-resident mode (device: " + std::to_string(dev_lds) + ")");
            return -1;
        }
    }
    HIPCHK(hipDeviceGetAttribute(&e->n_cu, hipDeviceAttributeMultiprocessorCount, e->device));
    for (auto& x : e->aux)
        if (x.create()) return -1;
    if (e->ev.ensure(4) || e->lane_done.ensure(mtr_engine::kLanes) || e->grp_fork.ensure(mtr_engine::kLanes) ||
        e->grp_cls.ensure(mtr_engine::kLanes))
        return -1;
    const size_t D = std::max<uint32_t>(e->max_docs, 1);
    e->h_kind.assign(D, 0);
    e->h_part.assign(D, 0);
    if (e->dkind.ensure(D) || e->dpart.ensure(D)) return -1;
    HIPCHK(hipMemset(e->dkind.p, 0, D * sizeof(uint32_t)));
    HIPCHK(hipMemset(e->dpart.p, 0, D * sizeof(uint32_t)));
    if (e->hdr.ensure(D) || e->seg.ensure(D * NF * c.max_segments) || e->heap.ensure(D * 2 * c.heap_entries) ||
        e->text.ensure(D * c.text_units) || e->prop.ensure(D * c.prop_words) || e->rm.ensure(D * (c.remover_cells + 2 * size_t(e->rtab))) ||
        e->stat.ensure(D * 4) || e->red.ensure(16))
        return -1;
    return mtr_reset(e) == MTR_OK ? 0 : -1;
}

extern "C" {

const char* mtr_last_error(void) { return g_err.c_str(); }

mtr_engine* mtr_engine_create(const mtr_options* opt, int device, uint32_t max_docs, const mtr_caps* caps) {
    auto* e = new mtr_engine();
    e->opt = opt ? *opt : mtr_options{0, 1, 10000, 0};
    if (e->opt.chunk_size <= 0) e->opt.chunk_size = 10000;
    mtr_caps c{4096, 2048, 65536, 16384, 4096, 256, 1024};
    if (caps) {
        if (caps->max_segments) c.max_segments = caps->max_segments;
        if (caps->heap_entries) c.heap_entries = caps->heap_entries;
        if (caps->text_units) c.text_units = caps->text_units;
        if (caps->prop_words) c.prop_words = caps->prop_words;
        if (caps->remover_cells) c.remover_cells = caps->remover_cells;
        if (caps->ops_per_launch) c.ops_per_launch = caps->ops_per_launch;
        if (caps->ref_slots) c.ref_slots = caps->ref_slots;
    }
    c.max_segments = (c.max_segments + 63) & ~63u;
    c.heap_entries = (c.heap_entries + 63) & ~63u;
    if (c.remover_cells > 0xfffffe) c.remover_cells = 0xfffffe;
    e->caps = c;
    while (e->rtab < 2 * int32_t(c.remover_cells)) e->rtab *= 2;
    e->device = device;
    e->max_docs = max_docs;
    if (engine_open(e)) {  // (the one failure exit: destroy frees whatever was made, and keeps the error text)
        mtr_engine_destroy(e);
        return nullptr;
    }
    return e;
}

// The members free themselves (engine.hip.h); all destroy adds is that no stream still runs work that uses them.
int mtr_engine_destroy(mtr_engine* e) {
    if (!e) return 0;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto& x : e->aux)
        if (x) (void)hipStreamSynchronize(x);
    delete e;
    return 0;
}

int mtr_reset(mtr_engine* e) {
    HIPCHK(hipSetDevice(e->device));
    if (drop_pipe(e)) return -1;
    const uint32_t n = std::max<uint32_t>(e->max_docs, 1);
    reset_kernel<<<(n + 255) / 256, 256, 0, e->stream>>>(e->hdr.p, n);
    // remover-head tables start empty (their keys are uids, which restart at 0)
    HIPCHK(hipMemsetAsync(e->rm.p, 0, e->rm.n * sizeof(uint32_t), e->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(e->stat.p, 0, e->stat.n * sizeof(unsigned long long), e->stream));
    e->summarized = false;
    e->drop_ids();
    e->pend_seen = false;
    e->refs_seen = false;
    e->census = {};
    return MTR_OK;
}

int mtr_submit(mtr_engine* e, const mtr_batch* b) {
    HIPCHK(hipSetDevice(e->device));
    if (b->n_docs > e->max_docs) {
        set_err("batch has more documents than the engine was created for");
        return MTR_ERR_BAD_OP;
    }
    if (drop_pipe(e) || upload(e, e->docs, b->docs, b->n_docs) || upload(e, e->ops, b->ops, b->n_ops) ||
        upload(e, e->btext, b->text, b->n_text) || upload_tables(e, b))
        return -1;
    // delta records (MTR_F_DELTA): per-document slices sized by an exact bound of this batch's records.
    // SharedString: an insert reports its one segment; a remove / annotate at most one range per unit
    // of its range and per segment.  SharedMatrix tracked for its cells (any flagged op): one record
    // per flagged set-cell, and per vector one per unlinked segment -- at most the segments present
    // at the batch start plus two per op (split + insert / load)
    e->has_delta = false;
    e->has_ext = false;
    e->h_doff.assign(size_t(b->n_docs) + 1, 0);
    bool any = false;
    if (b->n_ops) {  // one pass over the uploaded ops on the device instead of the host
        HIPCHK(hipMemsetAsync(e->red.p, 0, sizeof(int32_t), e->stream));
        const uint64_t blocks = std::min<uint64_t>((b->n_ops + 255) / 256, 4096);
        op_scan_kernel<<<uint32_t(blocks), 256, 0, e->stream>>>(e->ops.p, b->n_ops, e->red.p);
        HIPCHK(hipGetLastError());
        int32_t flag = 0;
        HIPCHK(hipMemcpyAsync(&flag, e->red.p, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        any = (flag & 1) != 0;
        e->has_ext = (flag & 2) != 0;
        if (flag & 4) {
            if (!e->pend.p) {
                if (e->pend.ensure(size_t(std::max<uint32_t>(e->max_docs, 1)) * kPendRing * 4)) return -1;
            }
            e->pend_seen = true;
        }
        if (flag & 8) {
            if (!e->refs.p &&
                e->refs.ensure(size_t(std::max<uint32_t>(e->max_docs, 1)) * 3 * size_t(e->caps.ref_slots)))
                return -1;
            e->refs_seen = true;
        }
    }
    e->has_ext = e->has_ext || e->pend_seen || e->refs_seen;
    if (any) {
        std::vector<uint64_t> need(b->n_docs, 0);
        for (uint32_t d = 0; d < b->n_docs; d++) {
            const mtr_doc_desc& dd = b->docs[d];
            const uint32_t kind = d < e->h_kind.size() ? e->h_kind[d] : 0;
            if (kind == 2) continue;  // a cols vector: sized with its rows document
            // (record mode submits op lists that are only written on the device: n_ops bounds the scan)
            const uint64_t end = std::min<uint64_t>(dd.op_begin + dd.op_count, b->n_ops);
            bool flagged = false;
            for (uint64_t i = dd.op_begin; i < end; i++) {
                const mtr_op& op = b->ops[i];
                if (!(op.flags & MTR_F_DELTA)) continue;
                flagged = true;
                if (kind == 1) {
                    if (op.type == MTR_OP_SETCELL || op.type == MTR_OP_LOCAL_SETCELL) need[d] += 1;
                    // (a vector's reconnect records: regenerate, two per member; rebasePosition, one)
                    const uint32_t dv = (op.flags & MTR_F_COLS) && e->h_part[d] < b->n_docs ? e->h_part[d] : d;
                    if (op.type == MTR_OP_REGENERATE) need[dv] += 2 * uint64_t(e->caps.max_segments);
                    if (op.type == MTR_OP_REBASE_POS) need[dv] += 1;
                } else if (op.type == MTR_OP_INSERT) {
                    need[d] += 1;
                } else if (op.type == MTR_OP_REMOVE || op.type == MTR_OP_ANNOTATE) {
                    need[d] += uint64_t(std::min<int64_t>(std::max<int64_t>(int64_t(op.pos2) - op.pos1, 0),
                                                          int64_t(e->caps.max_segments)));
                } else if (op.type == MTR_OP_REGENERATE) {  // two records per member of the group
                    need[d] += 2 * uint64_t(e->caps.max_segments);
                } else if (op.type == MTR_OP_REBASE_POS) {
                    need[d] += 1;
                }
            }
            if (kind == 1 && flagged) {
                // (+ undo tracking reports: a link per delta segment of a local vector op, a split-off half per
                // split, a merge per appended segment)
                const uint64_t recycle = 3 * uint64_t(e->caps.max_segments) + 6 * uint64_t(dd.op_count);
                need[d] += recycle;
                const uint32_t d1 = e->h_part[d];
                if (d1 < b->n_docs) need[d1] += recycle;
            }
        }
        for (uint32_t d = 0; d < b->n_docs; d++) e->h_doff[d + 1] = e->h_doff[d] + need[d];
    }
    if (e->h_doff[b->n_docs]) {
        e->has_delta = true;
        if (e->delta.ensure(size_t(e->h_doff[b->n_docs]) * 4) || e->doff.ensure(size_t(b->n_docs) + 1)) return -1;
        HIPCHK(hipMemcpyAsync(e->doff.p, e->h_doff.data(), (size_t(b->n_docs) + 1) * sizeof(uint64_t),
                              hipMemcpyHostToDevice, e->stream));
    }
    if (b->n_docs) {  // (an empty batch launches nothing: a 0-block grid is an invalid launch)
        cursor_reset_kernel<<<(b->n_docs + 255) / 256, 256, 0, e->stream>>>(e->hdr.p, e->docs.p, b->n_docs);
        HIPCHK(hipGetLastError());
    }
    e->summarized = false;
    e->drop_ids();
    return MTR_OK;
}

// mtr_submit_pipelined; for mtr_replay_pipelined `one_group` (below) and `out` / `cap`, the caller's buffer that the
// run streams the parts' summaries into; for mtr_replay_handover `hand`: the caller's buffer for the new blobs' bytes
// and its two bounds (cap is then what the device's record buffer is to hold, out null)
struct HandBounds {
    uint8_t* out;
    int64_t cap_bytes, cap_blobs;
};
static int submit_pipelined(mtr_engine* e, const mtr_batch* b, uint32_t parts, bool one_group, uint8_t* out, int64_t cap,
                            const HandBounds* hand = nullptr) {
    HIPCHK(hipSetDevice(e->device));
    const uint32_t n = b->n_docs;
    parts = std::min(parts, n);
    // documents laid out in order (each one's records and text after the previous one's), no matrix pairs
    bool plain = parts > 1 && n <= e->max_docs;
    for (uint32_t d = 1; d < n && plain; d++)
        plain = b->docs[d].op_begin >= b->docs[d - 1].op_begin + b->docs[d - 1].op_count &&
                b->docs[d].text_base >= b->docs[d - 1].text_base + b->docs[d - 1].text_count;
    for (uint32_t d = 0; d < n && plain && d < e->h_kind.size(); d++) plain = e->h_kind[d] == 0;
    if (!plain) return mtr_submit(e, b);
    if (drop_pipe(e) || upload_tables(e, b) || upload(e, e->pdocs, b->docs, n)) return -1;
    e->has_delta = false;
    e->has_ext = e->pend_seen || e->refs_seen;
    e->h_doff.assign(size_t(n) + 1, 0);
    if (e->ops.ensure(b->n_ops) || e->btext.ensure(b->n_text) || e->docs.ensure(n) || e->pflags.ensure(parts)) return -1;
    // every document starts disabled (op_count 0: classify_kernel passes it over) until its part has landed
    HIPCHK(hipMemsetAsync(e->docs.p, 0, size_t(n) * sizeof(mtr_doc_desc), e->stream));
    HIPCHK(hipMemsetAsync(e->pflags.p, 0, size_t(parts) * sizeof(int32_t), e->stream));
    // the copy stream is the last launch lane, which mtr_run leaves idle while parts are landing: a stream of its
    // own would share a hardware queue with the engine stream (GPU_MAX_HW_QUEUES = 4 = the launch lanes), and the
    // copies would then hold back every launch queued behind them there
    mtr_engine::PipeRun pr;  // (the engine's once every part is on its way)
    pr.parts = parts;
    pr.out = out;
    pr.cap = cap;
    pr.mode = hand ? mtr_engine::PipeRun::kHandover
                   : (out ? mtr_engine::PipeRun::kRecords : mtr_engine::PipeRun::kNoSummaries);
    if (hand) {
        pr.hand_out = hand->out;
        pr.hand_cap_bytes = hand->cap_bytes;
        pr.hand_cap_blobs = hand->cap_blobs;
    }
    pr.copy = e->aux[mtr_engine::kLanes - 2];
    if (e->part_ev.ensure(parts) || e->h_pflags.ensure(parts)) return -1;
    HIPCHK(hipEventRecord(e->ev[0], e->stream));  // (the copy stream starts after the tables)
    HIPCHK(hipStreamWaitEvent(pr.copy, e->ev[0], 0));
    pr.part_lo.assign(size_t(parts) + 1, 0);
    for (uint32_t p = 0; p <= parts; p++) pr.part_lo[p] = uint32_t(uint64_t(n) * p / parts);
    // two document groups (mtr_run's default above 4,096 documents), each with half the parts: the upload
    // alternates between them, so both start within the first two parts
    // (mtr_replay_pipelined: one group unless MTR_PIPE_GROUPS=2 -- the group's documents run their rounds in
    // lockstep, so its parts finish in the order they landed, a part's width apart, and their summaries and
    // downloads stream out behind them; two groups finish at two times, the second's parts all together)
    int pg = (n >= 4096u && parts >= 2) ? 2 : 1;
    if (one_group) {
        const char* v = std::getenv("MTR_PIPE_GROUPS");
        pg = std::min(pg, v && *v ? std::max(1, std::atoi(v)) : 1);
    }
    pr.groups = uint32_t(pg);
    // (a ramp -- the first two parts a quarter and a half of the others' size -- measured slower end to end:
    // 263.5 against 260.9 ms on C3, profiles/r06_e2e_sweep.json)
    if (e->dpart_lo.ensure(size_t(parts) + 1)) return -1;
    HIPCHK(hipMemcpyAsync(e->dpart_lo.p, pr.part_lo.data(), (size_t(parts) + 1) * sizeof(uint32_t),
                          hipMemcpyHostToDevice, e->stream));
    const uint32_t half = (parts + 1) / 2;
    for (uint32_t q = 0; q < parts; q++) {
        const uint32_t p = pr.groups == 2 ? ((q & 1) ? half + q / 2 : q / 2) : q;
        const uint32_t lo = pr.part_lo[p], hi = pr.part_lo[p + 1];
        const mtr_doc_desc &a = b->docs[lo], &z = b->docs[hi - 1];
        const uint64_t o0 = a.op_begin, o1 = std::min<uint64_t>(z.op_begin + z.op_count, b->n_ops);
        const uint64_t t0 = a.text_base, t1 = std::min<uint64_t>(z.text_base + z.text_count, b->n_text);
        if (o1 > o0) {
            HIPCHK(hipMemcpyAsync(e->ops.p + o0, b->ops + o0, (o1 - o0) * sizeof(mtr_op), hipMemcpyHostToDevice, pr.copy));
            const uint64_t blocks = std::min<uint64_t>((o1 - o0 + 255) / 256, 4096);
            op_scan_kernel<<<uint32_t(blocks), 256, 0, pr.copy>>>(e->ops.p + o0, o1 - o0, e->pflags.p + p);
        }
        if (t1 > t0)
            HIPCHK(hipMemcpyAsync(e->btext.p + t0, b->text + t0, (t1 - t0) * sizeof(uint16_t), hipMemcpyHostToDevice, pr.copy));
        part_ready_kernel<<<(hi - lo + 255) / 256, 256, 0, pr.copy>>>(e->hdr.p, e->docs.p, e->pdocs.p, lo, hi, e->pflags.p + p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(e->h_pflags.p + p, e->pflags.p + p, sizeof(int32_t), hipMemcpyDeviceToHost, pr.copy));
        HIPCHK(hipEventRecord(e->part_ev[p], pr.copy));
    }
    pr.last = pr.groups == 2 ? ((parts & 1) ? half - 1 : parts - 1) : parts - 1;  // (uploaded last)
    e->pipe = std::move(pr);
    e->summarized = false;
    e->drop_ids();
    return MTR_OK;
}

int mtr_submit_pipelined(mtr_engine* e, const mtr_batch* b, uint32_t parts) {
    return submit_pipelined(e, b, parts, false, nullptr, 0);
}

static int summary_params(mtr_engine* e, SParams& P);

int mtr_run(mtr_engine* e) { return apply_run(e, 0); }

int64_t mtr_get_deltas(mtr_engine* e, uint32_t doc, mtr_delta* out, int64_t cap) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (doc >= e->max_docs) {
        set_err("mtr_get_deltas: bad document");
        return -1;
    }
    DocHdr h;
    HIPCHK(hipMemcpy(&h, e->hdr.p + doc, sizeof(DocHdr), hipMemcpyDeviceToHost));
    const int64_t n = h.dused;
    if (n > cap) return -n;
    if (n && e->has_delta && doc < e->n_docs)
        HIPCHK(hipMemcpy(out, e->delta.p + e->h_doff[doc] * 4, size_t(n) * sizeof(mtr_delta),
                         hipMemcpyDeviceToHost));
    return n;
}

int64_t mtr_get_props(mtr_engine* e, uint32_t doc, uint32_t ref, uint32_t* out, int64_t cap) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const uint64_t pw = e->caps.prop_words;
    if (doc >= e->max_docs || ref >= pw) {
        set_err("mtr_get_props: bad document or properties reference");
        return -1;
    }
    const uint32_t* base = e->prop.p + size_t(doc) * pw;
    uint32_t n = 0;
    HIPCHK(hipMemcpy(&n, base + ref, 4, hipMemcpyDeviceToHost));
    const int64_t words = 1 + 2 * int64_t(n);
    if (uint64_t(ref) + uint64_t(words) > pw) {
        set_err("mtr_get_props: reference outside the property arena");
        return -1;
    }
    if (words > cap) return -words;
    HIPCHK(hipMemcpy(out, base + ref, size_t(words) * 4, hipMemcpyDeviceToHost));
    return words;
}

int mtr_set_matrix(mtr_engine* e, uint32_t rows_doc, uint32_t cols_doc) {
    HIPCHK(hipSetDevice(e->device));
    if (rows_doc >= e->h_kind.size() || cols_doc >= e->h_kind.size() || rows_doc == cols_doc ||
        e->h_kind[rows_doc] || e->h_kind[cols_doc]) {
        set_err("mtr_set_matrix: bad or already paired documents");
        return MTR_ERR_BAD_OP;
    }
    {  // a pair's HBM-resident launches hold two documents' chunk rows in LDS
        const size_t need = 2 * ((lds_bytes_global_mode(int(e->caps.max_segments)) + 15) & ~size_t(15));
        if (e->dev_lds > 0 && need > size_t(e->dev_lds)) {
            set_err("mtr_set_matrix: max_segments " + std::to_string(e->caps.max_segments) + " needs " +
                    std::to_string(need) + " bytes of LDS for a matrix pair in HBM-resident mode (device: " +
                    std::to_string(e->dev_lds) + ")");
            return MTR_ERR_CAPACITY;
        }
    }
    e->h_kind[rows_doc] = 1;
    e->h_kind[cols_doc] = 2;
    e->h_part[rows_doc] = cols_doc;
    e->h_part[cols_doc] = rows_doc;
    HIPCHK(hipMemcpyAsync(e->dkind.p, e->h_kind.data(), e->h_kind.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                          e->stream));
    HIPCHK(hipMemcpyAsync(e->dpart.p, e->h_part.data(), e->h_part.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MTR_OK;
}

int64_t mtr_replay_pipelined(mtr_engine* e, const mtr_batch* b, uint32_t parts, uint8_t* out, int64_t cap,
                             int64_t* doc_off) {
    const uint32_t n = b->n_docs;
    // a range of fewer than ~3,000 documents keeps too few in flight while the ranges land (one document group, every
    // round small): C2's 10,000 documents in 2 / 4 / 8 / 16 ranges measured 490 / 472 / 482 / 476 ms end to end
    // against 464 ms for the serial calls, C3's 100,000 in 16 ranges 258 against 322 ms (profiles/r06_e2e_sweep.json)
    const char* mpd = std::getenv("MTR_PIPE_MIN_PART_DOCS");
    const uint32_t min_part_docs = mpd ? uint32_t(std::max(0, std::atoi(mpd))) : 3000u;
    if (parts > 1 && n / parts < min_part_docs) parts = 1;  // (mtr_submit_pipelined: parts <= 1 is mtr_submit)
    if (submit_pipelined(e, b, parts, true, out, cap) != MTR_OK) return -1;
    if (e->pipe.parts) {
        if (apply_run(e, 0) != MTR_OK) return -1;
        if (doc_off) {
            for (uint32_t d = 0; d < n; d++) doc_off[d] = e->h_off[d];
            doc_off[n] = e->out_total;
        }
        return e->out_total;
    }
    // (a batch the pipelined path does not take: mtr_submit's, then the ordinary summarize and download)
    if (mtr_run(e) != MTR_OK || mtr_summarize(e) != MTR_OK) return -1;
    const int64_t r = mtr_get_summaries(e, 0, n, out, cap, doc_off);
    if (r < -1) set_err("mtr_replay_pipelined: the output buffer holds " + std::to_string(cap) + " bytes, the summaries "
                        "need " + std::to_string(-r));
    return r < 0 ? -1 : r;
}

int64_t mtr_replay_handover(mtr_engine* e, const mtr_batch* b, uint32_t parts, uint8_t* out, int64_t cap_bytes,
                            uint8_t* ids, uint8_t* state, int64_t* rep, int64_t* blob_off, int64_t cap_blobs,
                            int64_t* doc_first) {
    static const char* fn = "mtr_replay_handover";
    if (!e || !b || cap_bytes < 0 || cap_blobs < 0 || cap_blobs > (int64_t(1) << 30) || !blob_off ||
        (cap_bytes > 0 && !out) || (cap_blobs > 0 && (!ids || !state || !rep))) {
        set_err(std::string(fn) + ": null argument, or a bound that is negative or above 2^30 blobs");
        return -1;
    }
    const uint32_t n = b->n_docs;
    const char* mpd = std::getenv("MTR_PIPE_MIN_PART_DOCS");  // (mtr_replay_pipelined's screen, for its reasons)
    const uint32_t min_part_docs = mpd ? uint32_t(std::max(0, std::atoi(mpd))) : 3000u;
    if (parts > 1 && n / parts < min_part_docs) parts = 1;
    e->hand.outgrown = false;
    e->hand.copied = e->hand.t_ids = e->hand.t_novel = 0;
    // The records stay on the device.  Their buffer is sized before the run like everything else: a summary whose
    // blobs fit the caller's bounds has at most cap_bytes of blob bytes when every blob is new, and a record adds 4
    // bytes and 4 a blob; a buffer an earlier summary left larger is kept.  A summary that outgrows it (the cache holds
    // much of it, and the caller sized cap_bytes for the rest) stops the stage, and the serial calls below take over.
    // An outgrown run leaves the size it met, with a quarter of headroom, for the next call (rec_want): the serial
    // summarize below sizes the buffer to its records exactly, and a fleet that grows would outgrow that every time.
    const int64_t rec_cap = std::max({int64_t(e->out.n) - 16, cap_bytes + 4 * (int64_t(n) + cap_blobs), e->hand.rec_want});
    e->hand.ranges = false;
    bool outgrown = false;
    if (parts > 1 && n > 1) {
        // every buffer of the run, before the uploads are queued (engine.hip.h: handover_reserve)
        HIPCHK(hipSetDevice(e->device));
        e->summarized = false;
        if (handover_reserve(e, n, std::min(parts, n), cap_blobs, cap_bytes, e->stream) || e->out.ensure(size_t(rec_cap) + 16))
            return -1;
    }
    const HandBounds hb{out, cap_bytes, cap_blobs};
    if (submit_pipelined(e, b, parts, true, nullptr, rec_cap, &hb) != MTR_OK) return -1;
    if (e->pipe.parts) {
        const int rc = apply_run(e, 0);
        if (rc == MTR_OK) {
            if (handover_tables(e, ids, state, rep, blob_off, doc_first)) return -1;
            e->hand.ranges = true;
            return int64_t(e->hand.copied);
        }
        // only a run that stopped for the record buffer alone goes on: its batch is applied in full
        // (PipeSummaries::rc).  Any other failure -- a refused range above all -- is the caller's.
        outgrown = rc == MTR_ERR_CAPACITY && e->hand.outgrown;
        e->hand.outgrown = false;
        if (!outgrown) return -1;
    } else if (mtr_run(e) != MTR_OK) {  // (a batch the pipelined path does not take: mtr_submit's)
        return -1;
    }
    if (mtr_summarize(e) != MTR_OK) return -1;
    if (outgrown) e->hand.rec_want = e->out_total + e->out_total / 4;
    const int64_t r = n ? mtr_summary_novel(e, 0, n, out, cap_bytes, state, rep, blob_off, cap_blobs, doc_first) : 0;
    if (r == MTR_SUMMARY_TOO_SMALL)
        set_err(std::string(fn) + ": the output buffers hold " + std::to_string(cap_blobs) + " blobs and " +
                std::to_string(cap_bytes) + " bytes, the summary's blobs or its new bytes need more");
    if (r < 0) return -1;
    if (n == 0) {
        blob_off[0] = 0;
        if (doc_first) doc_first[0] = 0;
        return 0;
    }
    if (mtr_summary_blob_ids(e, 0, n, ids, cap_blobs, nullptr) < 0) return -1;
    e->hand.copied = double(r);
    return r;
}

__global__ void synth_init_kernel(mtr_synth_cfg cfg, mtr_synth_state* st, uint32_t n) {
    uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < n) mtr_synth_init(&cfg, d, &st[d]);
}
__global__ void synth_text_count_kernel(const mtr_synth_state* st, mtr_doc_desc* docs, uint32_t n) {
    uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < n) docs[d].text_count = st[d].text_used;
}

// the pre-grown documents' snapshot header segments (the oracle's generate_impl writes the same records):
// segment k of every document is the two units ('a' + k % 26, 'A' + k / 26 % 26), NonCollabClient, no merge info
__global__ void synth_grow_kernel(mtr_op* ops, uint16_t* text, mtr_synth_state* st, uint32_t n, uint32_t per,
                                  uint32_t text_cap, uint32_t grow) {
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= uint64_t(n) * (grow + 1)) return;
    const uint32_t d = uint32_t(t / (grow + 1)), k = uint32_t(t % (grow + 1));
    mtr_op op{};
    if (k < grow) {
        op.type = MTR_OP_LOAD;
        op.client = uint16_t(MTR_CLIENT_NONCOLLAB);
        op.ref_seq = -1;
        op.pos2 = -1;
        op.payload = 2 * k;
        op.payload2 = 2;
        text[uint64_t(d) * text_cap + 2 * k] = uint16_t('a' + k % 26);
        text[uint64_t(d) * text_cap + 2 * k + 1] = uint16_t('A' + (k / 26) % 26);
    } else {
        op.type = MTR_OP_START_COLLAB;
        st[d].text_used = 2 * grow;
    }
    ops[uint64_t(d) * per + k] = op;
}

int mtr_generate(mtr_engine* e, const mtr_synth_cfg* cfg, const mtr_batch* tables) {
    return mtr_generate_grown(e, cfg, tables, 0);
}

int mtr_generate_grown(mtr_engine* e, const mtr_synth_cfg* cfg, const mtr_batch* tables, uint32_t grow) {
    HIPCHK(hipSetDevice(e->device));
    if (cfg->n_docs > e->max_docs || cfg->writers > MTR_SYNTH_MAX_WRITERS || cfg->writers + 1 > 0xfd ||
        uint64_t(cfg->text_cap) < 2ull * grow) {
        set_err("mtr_generate: bad configuration");
        return MTR_ERR_BAD_OP;
    }
    const uint32_t n = cfg->n_docs, per = grow + cfg->ops_per_doc + 1;
    if (n == 0) return mtr_reset(e);
    std::vector<mtr_doc_desc> docs(n);
    for (uint32_t d = 0; d < n; d++) {
        docs[d].op_begin = uint64_t(d) * per;
        docs[d].op_count = per;
        docs[d].text_base = uint64_t(d) * cfg->text_cap;
        docs[d].text_count = 0;
        docs[d].client_base = 0;
        docs[d].n_clients = cfg->writers + 1;
    }
    mtr_batch b = *tables;
    b.n_docs = n;
    b.docs = docs.data();
    b.n_ops = 0;
    b.n_text = 0;
    if (mtr_reset(e) != MTR_OK || mtr_submit(e, &b) != MTR_OK) return -1;
    if (e->ops.ensure(size_t(n) * per) || e->btext.ensure(size_t(n) * cfg->text_cap) || e->gstate.ensure(n)) return -1;
    e->gcfg = *cfg;
    e->ggrow = grow;
    synth_init_kernel<<<(n + 255) / 256, 256, 0, e->stream>>>(*cfg, e->gstate.p, n);
    HIPCHK(hipGetLastError());
    if (grow) {
        const uint64_t total = uint64_t(n) * (grow + 1);
        synth_grow_kernel<<<uint32_t((total + 255) / 256), 256, 0, e->stream>>>(e->ops.p, e->btext.p, e->gstate.p, n,
                                                                               per, cfg->text_cap, grow);
        HIPCHK(hipGetLastError());
    }
    const int rc = apply_run(e, 1);
    e->ggrow = 0;
    if (rc != MTR_OK) return -1;
    synth_text_count_kernel<<<(n + 255) / 256, 256, 0, e->stream>>>(e->gstate.p, e->docs.p, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return MTR_OK;
}

// matrix m's generator state lives with its rows vector (engine document 2m), seeded as matrix m
__global__ void synth_init_matrix_kernel(mtr_synth_cfg cfg, mtr_synth_state* st, uint32_t n) {
    uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < 2 * n) mtr_synth_init(&cfg, d / 2, &st[d]);
}

int mtr_generate_matrix(mtr_engine* e, const mtr_synth_cfg* cfg, const mtr_batch* tables) {
    HIPCHK(hipSetDevice(e->device));
    const uint32_t n = cfg->n_docs, per = cfg->ops_per_doc + 1;
    if (2ull * n > e->max_docs || cfg->writers > MTR_SYNTH_MAX_WRITERS || cfg->writers + 1 > 0xfd) {
        set_err("mtr_generate_matrix: bad configuration");
        return MTR_ERR_BAD_OP;
    }
    if (n == 0) return mtr_reset(e);
    for (uint32_t m = 0; m < n; m++) {  // pair the vectors (mtr_set_matrix) unless already paired so
        const uint32_t r = 2 * m, c = 2 * m + 1;
        if (e->h_kind[r] == 1 && e->h_part[r] == c) continue;
        if (e->h_kind[r] || e->h_kind[c]) {
            set_err("mtr_generate_matrix: documents 2m, 2m+1 are paired otherwise");
            return MTR_ERR_BAD_OP;
        }
        e->h_kind[r] = 1;
        e->h_kind[c] = 2;
        e->h_part[r] = c;
        e->h_part[c] = r;
    }
    HIPCHK(hipMemcpyAsync(e->dkind.p, e->h_kind.data(), e->h_kind.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                          e->stream));
    HIPCHK(hipMemcpyAsync(e->dpart.p, e->h_part.data(), e->h_part.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                          e->stream));
    std::vector<mtr_doc_desc> docs(2 * size_t(n));
    for (uint32_t m = 0; m < n; m++) {
        for (uint32_t w = 0; w < 2; w++) {
            mtr_doc_desc& x = docs[2 * m + w];
            x.op_begin = uint64_t(m) * per;
            x.op_count = w == 0 ? per : 0;  // the cols vector has no op list of its own
            x.text_base = 0;
            x.text_count = 0;
            x.client_base = 0;
            x.n_clients = cfg->writers + 1;
        }
    }
    mtr_batch b = *tables;
    b.n_docs = 2 * n;
    b.docs = docs.data();
    b.n_ops = 0;
    b.n_text = 0;
    if (mtr_reset(e) != MTR_OK || mtr_submit(e, &b) != MTR_OK) return -1;
    if (e->ops.ensure(size_t(n) * per) || e->btext.ensure(1) || e->gstate.ensure(2 * size_t(n))) return -1;
    e->gcfg = *cfg;
    e->gcfg.text_cap = 0;  // the matrix recipe draws no text
    synth_init_matrix_kernel<<<(2 * n + 255) / 256, 256, 0, e->stream>>>(*cfg, e->gstate.p, n);
    HIPCHK(hipGetLastError());
    if (apply_run(e, 1) != MTR_OK) return -1;
    HIPCHK(hipStreamSynchronize(e->stream));
    return MTR_OK;
}

int mtr_download_batch(mtr_engine* e, uint32_t lo, uint32_t hi, mtr_doc_desc* docs, mtr_op* ops, uint16_t* text,
                       uint64_t text_cap) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (hi > e->n_docs || lo > hi) {
        set_err("mtr_download_batch: bad range");
        return -1;
    }
    std::vector<mtr_doc_desc> dd(hi - lo);
    if (hi > lo) HIPCHK(hipMemcpy(dd.data(), e->docs.p + lo, (hi - lo) * sizeof(mtr_doc_desc), hipMemcpyDeviceToHost));
    // op lists: one copy per run of documents whose lists are adjacent on the device (a recorded
    // batch is one run); empty lists (matrix cols vectors) never break a run
    uint64_t op_at = 0, text_at = 0, text_need = 0;
    if (ops) {
        uint64_t run_src = 0, run_dst = 0, run_n = 0;
        for (uint32_t i = 0; i < hi - lo; i++) {
            const mtr_doc_desc& x = dd[i];
            if (x.op_count == 0) continue;
            if (run_n && x.op_begin != run_src + run_n) {
                HIPCHK(hipMemcpy(ops + run_dst, e->ops.p + run_src, run_n * sizeof(mtr_op), hipMemcpyDeviceToHost));
                run_n = 0;
            }
            if (!run_n) {
                run_src = x.op_begin;
                run_dst = op_at;
            }
            run_n += x.op_count;
            op_at += x.op_count;
        }
        if (run_n) HIPCHK(hipMemcpy(ops + run_dst, e->ops.p + run_src, run_n * sizeof(mtr_op), hipMemcpyDeviceToHost));
    }
    for (uint32_t i = 0; i < hi - lo; i++) text_need += dd[i].text_count;
    if (text && text_need && text_need <= text_cap) {
        // texts: one copy of the span when the gaps between documents are small, then compacted
        uint64_t t0 = UINT64_MAX, t1 = 0;
        for (uint32_t i = 0; i < hi - lo; i++)
            if (dd[i].text_count) {
                t0 = std::min<uint64_t>(t0, dd[i].text_base);
                t1 = std::max<uint64_t>(t1, dd[i].text_base + dd[i].text_count);
            }
        if (t1 - t0 <= 4 * text_need + (1u << 20)) {
            std::vector<uint16_t> span(t1 - t0);
            HIPCHK(hipMemcpy(span.data(), e->btext.p + t0, span.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < hi - lo; i++) {
                std::memcpy(text + text_at, span.data() + (dd[i].text_base - t0), dd[i].text_count * sizeof(uint16_t));
                text_at += dd[i].text_count;
            }
        } else {
            for (uint32_t i = 0; i < hi - lo; i++) {
                if (dd[i].text_count)
                    HIPCHK(hipMemcpy(text + text_at, e->btext.p + dd[i].text_base, dd[i].text_count * sizeof(uint16_t),
                                     hipMemcpyDeviceToHost));
                text_at += dd[i].text_count;
            }
        }
    }
    op_at = 0;
    text_at = 0;
    for (uint32_t i = 0; i < hi - lo; i++) {
        mtr_doc_desc x = dd[i];
        x.op_begin = op_at;
        x.text_base = text_at;
        op_at += x.op_count;
        text_at += x.text_count;
        if (docs) docs[i] = x;
    }
    return MTR_OK;
}

// the summary kernels' parameters for every document of the batch (scratch buffers sized)
static int summary_params(mtr_engine* e, SParams& P) {
    const uint32_t n = e->n_docs;
    if (e->out_size.ensure(n) || e->out_off.ensure(n) || e->out_hash.ensure(n)) return -1;
    P = SParams{};
    P.hdr = e->hdr.p;
    P.seg = e->seg.p;
    P.text = e->text.p;
    P.prop = e->prop.p;
    P.rm = e->rm.p;
    P.segcap = int(e->caps.max_segments);
    P.tcap = int(e->caps.text_units);
    P.pcap = int(e->caps.prop_words);
    P.rcap = int(e->caps.remover_cells);
    P.rtab = e->rtab;
    P.snapshot_v1 = e->opt.snapshot_v1;
    P.chunk_size = e->opt.chunk_size;
    P.new_length_calc = e->opt.new_length_calc;
    P.n_docs = n;
    P.docs = e->docs.p;
    P.key_off = e->key_off.p;
    P.key_bytes = e->key_bytes.p;
    P.val_off = e->val_off.p;
    P.val_bytes = e->val_bytes.p;
    P.val_eq = e->val_eq.p;
    P.client_off = e->client_off.p;
    P.client_bytes = e->client_bytes.p;
    P.dkind = e->dkind.p;
    P.out_size = e->out_size.p;
    P.out_off = e->out_off.p;
    P.out_hash = e->out_hash.p;
    {
        const size_t sc = size_t(P.segcap);
        P.maxb = int(std::min<int64_t>(int64_t(sc) + 1, std::max<int64_t>(int64_t(P.tcap) / std::max(1, P.chunk_size) + 4, 64)));
        if (e->s_kind.ensure(n * sc) || e->s_start.ensure(n * (sc + 1)) || e->s_len.ensure(n * sc) ||
            e->s_bytes.ensure(n * sc) || e->s_blob.ensure(n * (4 + 4 * size_t(P.maxb))) || e->s_lb.ensure(n * sc) ||
            e->s_fl.ensure(n * sc) || e->s_sid.ensure(n * sc) || e->s_bb.ensure(n * sc))
            return -1;
        P.s_kind = e->s_kind.p;
        P.s_start = e->s_start.p;
        P.s_len = e->s_len.p;
        P.s_bytes = e->s_bytes.p;
        P.s_lb = e->s_lb.p;
        P.s_fl = e->s_fl.p;
        P.s_sid = e->s_sid.p;
        P.s_bb = e->s_bb.p;
        P.s_blob = e->s_blob.p;
    }
    return 0;
}

int mtr_summarize(mtr_engine* e) {
    HIPCHK(hipSetDevice(e->device));
    const uint32_t n = e->n_docs;
    if (n == 0) return MTR_OK;
    e->drop_ids();  // (the records are rewritten)
    if (summary_reserve(e)) return -1;  // (allocations stay out of the timed span)
    {  // (timing probes: MTR_SUM_DEBUG, summary.hip.h g_sdbg)
        const char* v = std::getenv("MTR_SUM_DEBUG");
        const int dbg = v ? std::atoi(v) : 0;
        static int last = 0;
        if (dbg != last) {
            HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_sdbg), &dbg, sizeof(int)));
            last = dbg;
        }
    }
    HIPCHK(hipEventRecord(e->ev[2], e->stream));
    if (summary_size_pass(e, 0, n, e->stream)) return -1;
    e->h_size.resize(n);
    e->h_off.resize(n);
    HIPCHK(hipMemcpyAsync(e->h_size.data(), e->out_size.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    int64_t tot = 0;
    for (uint32_t d = 0; d < n; d++) {
        if (e->h_size[d] < 0) {
            set_err("document " + std::to_string(d) + " has more summary chunks than the engine's blob table");
            return MTR_ERR_CAPACITY;
        }
        e->h_off[d] = tot;
        tot += e->h_size[d];
    }
    e->out_total = tot;
    if (e->out.ensure(size_t(tot) + 16)) return -1;
    HIPCHK(hipMemcpyAsync(e->out_off.p, e->h_off.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
    if (summary_write_pass(e, 0, n, e->stream)) return -1;
    HIPCHK(hipEventRecord(e->ev[3], e->stream));
    HIPCHK(hipEventSynchronize(e->ev[3]));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->ev[2], e->ev[3]));
    e->t_summary = ms;
    e->summarized = true;
    return MTR_OK;
}

int mtr_sync(mtr_engine* e) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MTR_OK;
}

// one document's summary record in the output buffer: u32 nb, u32 len[nb], blob bytes
static int summary_record(mtr_engine* e, uint32_t doc, std::vector<uint8_t>& buf) {
    if (!e->summarized || doc >= e->n_docs) {
        set_err("no summary for this document (call mtr_summarize first)");
        return -1;
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    buf.resize(size_t(e->h_size[doc]));
    HIPCHK(hipMemcpy(buf.data(), e->out.p + e->h_off[doc], buf.size(), hipMemcpyDeviceToHost));
    return 0;
}

int mtr_summary_info(mtr_engine* e, uint32_t doc, int64_t* n_blobs, int64_t* n_bytes) {
    if (!e->summarized || doc >= e->n_docs) {
        set_err("no summary for this document (call mtr_summarize first)");
        return -1;
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    uint32_t nb = 0;
    HIPCHK(hipMemcpy(&nb, e->out.p + e->h_off[doc], 4, hipMemcpyDeviceToHost));
    if (n_blobs) *n_blobs = nb;
    if (n_bytes) *n_bytes = e->h_size[doc] - 4 - 4 * int64_t(nb);
    return MTR_OK;
}

int64_t mtr_get_summary(mtr_engine* e, uint32_t doc, uint8_t* out, int64_t cap, int64_t* blob_len, int32_t max_blobs) {
    std::vector<uint8_t> buf;
    if (summary_record(e, doc, buf)) return -1;
    uint32_t nb;
    std::memcpy(&nb, buf.data(), 4);
    const int64_t payload = int64_t(buf.size()) - 4 - 4 * int64_t(nb);
    if (payload > cap || int64_t(nb) > int64_t(max_blobs) || (payload > 0 && !out) || !blob_len) {
        set_err("mtr_get_summary: buffers smaller than mtr_summary_info reports");
        return MTR_SUMMARY_TOO_SMALL;
    }
    int64_t off = 4 + 4 * int64_t(nb);
    int64_t w = 0;
    for (uint32_t k = 0; k < nb; k++) {
        uint32_t len;
        std::memcpy(&len, buf.data() + 4 + 4 * k, 4);
        blob_len[k] = len;
        std::memcpy(out + w, buf.data() + off, len);
        off += len;
        w += len;
    }
    return int64_t(nb);
}

int64_t mtr_get_summaries(mtr_engine* e, uint32_t lo, uint32_t hi, uint8_t* out, int64_t cap, int64_t* doc_off) {
    if (summary_range(e, "mtr_get_summaries", lo, hi)) return -1;
    if (lo == hi) {
        if (doc_off) doc_off[0] = 0;
        return 0;
    }
    const int64_t base = e->h_off[lo];
    const int64_t total = e->h_off[hi - 1] + e->h_size[hi - 1] - base;  // documents are laid out in order
    if (total > cap) return -total;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, e->out.p + base, size_t(total), hipMemcpyDeviceToHost));
    if (doc_off) {
        for (uint32_t d = lo; d < hi; d++) doc_off[d - lo] = e->h_off[d] - base;
        doc_off[hi - lo] = total;
    }
    return total;
}

void* mtr_host_alloc(uint64_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, std::max<uint64_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) {
        set_err("hipHostMalloc failed for " + std::to_string(bytes) + " bytes");
        return nullptr;
    }
    return p;
}

int mtr_host_free(void* p) {
    if (p && hipHostFree(p) != hipSuccess) return -1;
    return MTR_OK;
}

int mtr_summary_hashes(mtr_engine* e, uint64_t* out, uint32_t n_docs) {
    if (!e->summarized) return -1;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpy(out, e->out_hash.p, std::min(n_docs, e->n_docs) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return MTR_OK;
}

int64_t mtr_summary_bytes(mtr_engine* e) { return e->summarized ? e->out_total : -1; }

// ---- host-side decoding of one document's slabs (parity checks, getText)
struct HostDoc {
    DocHdr h;
    std::vector<uint32_t> seg;
    std::vector<uint16_t> text;
    std::vector<uint32_t> prop, rm, rt;
    // head of leaf i's later-removers list (the device's uid table)
    uint32_t rm_head(uint32_t uid) const {
        const uint32_t mask = uint32_t(rt.size() / 2 - 1);
        uint32_t h = rtab_hash(uid) & mask;
        for (size_t n = 0; n <= mask; n++) {
            if (rt[2 * h] == uid + 1) return rt[2 * h + 1];
            if (rt[2 * h] == 0) break;
            h = (h + 1) & mask;
        }
        return 0xffffffu;
    }
};

static int fetch_doc(mtr_engine* e, uint32_t doc, HostDoc& hd) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(&hd.h, e->hdr.p + doc, sizeof(DocHdr), hipMemcpyDeviceToHost));
    const size_t sc = e->caps.max_segments;
    hd.seg.resize(NF * sc);
    HIPCHK(hipMemcpy(hd.seg.data(), e->seg.p + size_t(doc) * NF * sc, NF * sc * 4, hipMemcpyDeviceToHost));
    hd.text.resize(std::max(hd.h.textused, 1));
    HIPCHK(hipMemcpy(hd.text.data(), e->text.p + size_t(doc) * e->caps.text_units, hd.text.size() * 2,
                     hipMemcpyDeviceToHost));
    hd.prop.resize(std::max(hd.h.propused, 1));
    HIPCHK(hipMemcpy(hd.prop.data(), e->prop.p + size_t(doc) * e->caps.prop_words, hd.prop.size() * 4,
                     hipMemcpyDeviceToHost));
    const size_t rs = e->caps.remover_cells + 2 * size_t(e->rtab);
    hd.rm.resize(std::max(hd.h.rmused, 1));
    HIPCHK(hipMemcpy(hd.rm.data(), e->rm.p + size_t(doc) * rs, hd.rm.size() * 4, hipMemcpyDeviceToHost));
    hd.rt.resize(2 * size_t(e->rtab));
    HIPCHK(hipMemcpy(hd.rt.data(), e->rm.p + size_t(doc) * rs + e->caps.remover_cells, hd.rt.size() * 4,
                     hipMemcpyDeviceToHost));
    return 0;
}

// MergeTreeTextHelper.getText (MergeTreeTextHelper.ts:20-81) at the local view, on the device: one wave
// per document [lo, lo + gridDim.x) walks its leaves 64 at a time (text segments that are not removed;
// markers add nothing), an add-scan places each leaf's units, and the wave copies them leaf by leaf
// (coalesced runs from the document's text arena).  Pass 1 (out == nullptr) writes the lengths to
// lens[doc - lo]; pass 2 writes the units at off[doc - lo].
__global__ void __launch_bounds__(NT) text_kernel(const DocHdr* hdr, const uint32_t* seg, const uint16_t* text,
                                                  int segcap, int tcap, uint32_t lo, int64_t* lens,
                                                  const int64_t* off, uint16_t* out) {
    const uint32_t d = lo + blockIdx.x;
    const int S = __builtin_amdgcn_readfirstlane(hdr[d].nseg);
    const int ln = threadIdx.x;
    const uint32_t* g = seg + size_t(d) * NF * segcap;
    const uint16_t* tx = text + size_t(d) * tcap;
    int64_t carry = out ? off[blockIdx.x] : 0;
    for (int base = 0; base < S; base += 64) {
        const int i = base + ln;
        int len = 0;
        uint32_t t = 0;
        if (i < S && int(g[F_RSEQ * segcap + i]) == RNONE && !(g[F_META * segcap + i] & M_MARKER)) {
            len = int(g[F_LEN * segcap + i]);
            t = g[F_TEXT * segcap + i];
        }
        const int inc = wave_incl_scan(len);
        if (out) {
            const int n = min(64, S - base);
            for (int l = 0; l < n; l++) {
                const int ll = __builtin_amdgcn_readlane(len, l);
                const uint32_t tl = uint32_t(__builtin_amdgcn_readlane(int(t), l));
                const int64_t o = carry + __builtin_amdgcn_readlane(inc, l) - ll;
                for (int k = ln; k < ll; k += 64) out[o + k] = tx[tl + k];
            }
        }
        carry += __builtin_amdgcn_readlane(inc, 63);
    }
    if (!out && ln == 0) lens[blockIdx.x] = carry;
}

// texts of documents [lo, hi): out = the concatenated units, doc_off[i] = start of document lo + i
// (doc_off[hi - lo] = total); returns the total (nothing written when out is NULL), -1 when cap is
// too small or on error
int64_t mtr_get_texts(mtr_engine* e, uint32_t lo, uint32_t hi, uint16_t* out, int64_t cap, int64_t* doc_off) {
    HIPCHK(hipSetDevice(e->device));
    if (hi > e->max_docs || lo > hi) {
        set_err("mtr_get_texts: bad document range");
        return -1;
    }
    const uint32_t n = hi - lo;
    if (doc_off) doc_off[0] = 0;
    if (n == 0) return 0;
    DevBuf<int64_t> lens, offs;
    if (lens.ensure(n) || offs.ensure(size_t(n) + 1)) return -1;
    text_kernel<<<n, NT, 0, e->stream>>>(e->hdr.p, e->seg.p, e->text.p, int(e->caps.max_segments),
                                         int(e->caps.text_units), lo, lens.p, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> hl(n), ho(size_t(n) + 1, 0);
    HIPCHK(hipMemcpyAsync(hl.data(), lens.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (uint32_t i = 0; i < n; i++) ho[i + 1] = ho[i] + hl[i];
    const int64_t total = ho[n];
    if (doc_off) std::copy(ho.begin(), ho.end(), doc_off);
    if (!out || total == 0) return total;
    if (total > cap) {
        set_err("mtr_get_texts: output buffer too small");
        return -1;
    }
    DevBuf<uint16_t> dev;
    if (dev.ensure(size_t(total))) return -1;
    HIPCHK(hipMemcpyAsync(offs.p, ho.data(), (size_t(n) + 1) * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
    text_kernel<<<n, NT, 0, e->stream>>>(e->hdr.p, e->seg.p, e->text.p, int(e->caps.max_segments),
                                         int(e->caps.text_units), lo, lens.p, offs.p, dev.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dev.p, size_t(total) * sizeof(uint16_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return total;
}

int64_t mtr_get_text(mtr_engine* e, uint32_t doc, uint16_t* out, int64_t cap) {
    if (doc >= e->max_docs) {
        set_err("mtr_get_text: bad document");
        return -1;
    }
    int64_t off[2];
    const int64_t n = mtr_get_texts(e, doc, doc + 1, nullptr, 0, off);
    if (n <= 0 || !out || n > cap) return n;
    return mtr_get_texts(e, doc, doc + 1, out, cap, off);
}

int mtr_get_containing_segment(mtr_engine* e, uint32_t doc, int32_t pos, int32_t ref_seq, int32_t client,
                               mtr_segment_info* info, uint16_t* text, int64_t text_cap) {
    HIPCHK(hipSetDevice(e->device));
    if (doc >= e->max_docs || !info) {
        set_err("mtr_get_containing_segment: bad document");
        return -1;
    }
    KParams P;
    query_params(e, P);
    if (e->red.ensure(16)) return -1;
    containing_kernel<<<1, NT, lds_bytes_global_mode(int(P.segcap)), e->stream>>>(P, doc, pos, ref_seq, client, e->red.p);
    HIPCHK(hipGetLastError());
    int32_t r[11];
    HIPCHK(hipMemcpyAsync(r, e->red.p, sizeof(r), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    segment_info_from_row(r, pos, info);
    if (info->leaf < 0) return MTR_OK;
    const bool has_text = !info->marker && e->h_kind[doc] == 0;
    if (text && has_text && info->length > 0 && text_cap >= info->length)
        HIPCHK(hipMemcpy(text, e->text.p + size_t(doc) * e->caps.text_units + uint32_t(r[7]),
                         size_t(info->length) * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return MTR_OK;
}

static int ref_query(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap, int info_id) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (doc >= e->max_docs) {
        set_err("local references: bad document");
        return -1;
    }
    DocHdr h;
    HIPCHK(hipMemcpy(&h, e->hdr.p + doc, sizeof(DocHdr), hipMemcpyDeviceToHost));
    const int64_t n = e->refs.p ? h.nrefs : 0;
    const int64_t words = info_id >= 0 ? 4 : info_id == -3 ? 4 * n : info_id == -2 ? 2 * n : n;
    if (info_id < 0 && (words > cap || n == 0 || !out)) return int(n);
    KParams P;
    query_params(e, P);
    P.refs = e->refs.p;
    P.refcap = int(e->caps.ref_slots);
    if (e->qbuf.ensure(size_t(std::max<int64_t>(words, 4)))) return -1;
    refs_kernel<<<1, NT, lds_bytes_global_mode(int(P.segcap)), e->stream>>>(P, doc, e->qbuf.p, info_id);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, e->qbuf.p, size_t(words) * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return int(n);
}

int64_t mtr_get_ref_positions(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap) {
    return ref_query(e, doc, out, cap, -1);
}

int64_t mtr_get_ref_states(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap) {
    return ref_query(e, doc, out, cap, -2);
}

int64_t mtr_get_ref_keys(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap) {
    return ref_query(e, doc, out, cap, -3);
}

int32_t mtr_get_ref_info(mtr_engine* e, uint32_t doc, uint32_t id, int32_t* out) {
    if (!out) return -2;
    out[0] = -1;
    out[1] = out[2] = out[3] = 0;
    if (id > uint32_t(INT32_MAX)) {  // (a negative id would run the positions query instead)
        set_err("mtr_get_ref_info: reference id out of range");
        return -2;
    }
    if (ref_query(e, doc, out, 4, int(id)) < 0) return -2;
    return out[0];
}

int32_t mtr_pending_groups(mtr_engine* e, uint32_t doc) {
    if (doc >= e->max_docs) return -1;
    DocHdr h;
    (void)hipSetDevice(e->device);
    if (hipStreamSynchronize(e->stream) != hipSuccess ||
        hipMemcpy(&h, e->hdr.p + doc, sizeof(DocHdr), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return h.ptail - h.phead;  // (ring entries [phead, ptail): one per pending SegmentGroup)
}

int mtr_doc_status(mtr_engine* e, uint32_t doc, int32_t* op_index) {
    if (doc >= e->max_docs) return -1;
    DocHdr h;
    (void)hipSetDevice(e->device);
    if (hipStreamSynchronize(e->stream) != hipSuccess ||
        hipMemcpy(&h, e->hdr.p + doc, sizeof(DocHdr), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    if (op_index) *op_index = h.fail_op;
    return h.status;
}

int64_t mtr_export(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap, int32_t* height) {
    HostDoc hd;
    if (doc >= e->max_docs || fetch_doc(e, doc, hd)) return -1;
    const size_t sc = e->caps.max_segments;
    if (height) *height = hd.h.height;
    if (hd.h.nseg - hd.h.holes > cap) return -int64_t(hd.h.nseg - hd.h.holes);
    int k = 0;  // leaf ordinal (hole slots of HBM-resident documents are skipped)
    for (int i = 0; i < hd.h.nseg; i++) {
        const uint32_t m = hd.seg[F_META * sc + i];
        if (hd.h.holes && (m & M_DEL)) continue;
        const int32_t rs = int32_t(hd.seg[F_RSEQ * sc + i]);
        int nrem = 0;
        if (rs != RNONE) {
            nrem = 1;
            if (m & M_OVERLAP) {
                uint32_t c = hd.rm_head(hd.seg[F_UID * sc + i]);
                while (c != 0xffffffu) {
                    nrem++;
                    c = hd.rm[c] & 0xffffffu;
                }
            }
        }
        uint32_t h = 0;
        const uint32_t pr = hd.seg[F_PROPS * sc + i] & ~MTR_PROPS_NEVER;  // (index flag)
        if (hd.seg[F_PROPS * sc + i] != NONE32 && !e->h_kind[doc]) {  // (a matrix vector's: a tracking id)
            h = 2166136261u ^ 1u;
            for (uint32_t q = 0; q < hd.prop[pr]; q++) {  // same hash as the oracle export
                const uint32_t v = hd.prop[pr + 2 + 2 * q];
                h = (h ^ hd.prop[pr + 1 + 2 * q]) * 16777619u;
                h = (h ^ (v < e->h_val_eq.size() ? e->h_val_eq[v] : v)) * 16777619u;
            }
        }
        int32_t* r = out + 8 * k++;
        // (pending local values are kept above every sequence number, LOCAL_BASE + localSeq: reported as the
        // reference holds them, UnassignedSequenceNumber, as the oracle export does)
        const int32_t sq = int32_t(hd.seg[F_SEQ * sc + i]);
        r[0] = int32_t(hd.seg[F_LEN * sc + i]);
        r[1] = sq >= LOCAL_BASE ? -1 : sq;
        r[2] = dec_client(m & M_CLIENT_MASK);
        r[3] = rs == RNONE ? INT32_MIN : (rs >= LOCAL_BASE ? -1 : rs);
        r[4] = nrem;
        r[5] = int32_t((m & M_BND_MASK) >> M_BND_SHIFT);
        // PermutationSegment: its start handle (the oracle export does the same)
        r[6] = e->h_kind[doc] ? int32_t(hd.seg[F_TEXT * sc + i]) : ((m & M_MARKER) ? 1 : 0);
        r[7] = int32_t(h);
    }
    return k;
}

int64_t mtr_get_leaves(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap) {
    HostDoc hd;
    if (doc >= e->max_docs || !e->h_kind[doc]) {
        set_err("mtr_get_leaves: not a matrix vector document");
        return -1;
    }
    if (fetch_doc(e, doc, hd)) return -1;
    const size_t sc = e->caps.max_segments;
    if (!out || hd.h.nseg - hd.h.holes > cap) return hd.h.nseg - hd.h.holes;  // (a size query)
    int k = 0;
    for (int i = 0; i < hd.h.nseg; i++) {
        const uint32_t m = hd.seg[F_META * sc + i];
        if (hd.h.holes && (m & M_DEL)) continue;
        const uint32_t t = hd.seg[F_PROPS * sc + i];
        int32_t* r = out + 5 * k++;
        r[0] = int32_t(hd.seg[F_LEN * sc + i]);
        r[1] = int32_t(hd.seg[F_RSEQ * sc + i]) != RNONE ? 1 : 0;
        r[2] = int32_t(hd.seg[F_TEXT * sc + i]);
        r[3] = t == NONE32 ? -1 : int32_t(t);
        r[4] = t == NONE32 || t >= hd.prop.size() ? 0 : int32_t(hd.prop[t]);
    }
    return k;
}

// debug: the scan arrays (E, V) an HBM-resident document's last op left in the scratch slab
int64_t mtr_debug_scan(mtr_engine* e, uint32_t doc, int32_t* out, int64_t n) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const size_t sc = e->caps.max_segments;
    if (!e->scratch.p || doc >= e->n_docs || n > int64_t(sc)) return -1;
    HIPCHK(hipMemcpy(out, e->scratch.p + size_t(doc) * 2 * sc, size_t(n) * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) {  // the scan array keeps the undefined flag in bit 31
        const int32_t ei = out[i], ep = i ? (out[i - 1] & 0x7fffffff) : 0;
        out[n + i] = ei < 0 ? -1 : ei - ep;
    }
    for (int64_t i = 0; i < n; i++) out[i] &= 0x7fffffff;
    return n;
}

int64_t mtr_debug_live_bytes(void) { return g_live_bytes.load(); }

// (the order include/mtr.h documents and Engine.launch_counts names)
static_assert(AV_COUNT == mtr_engine::kCensusVariants && AV_LDS_X == 0 && AV_HBM_X == 1 && AV_LDS_LEAN == 2 &&
                  AV_HBM_LEAN == 3 && AV_LDS_DL == 4 && AV_HBM_DL == 5 && AV_LDS_GN == 6 && AV_HBM_GN == 7 &&
                  AV_PAIR_LDS == 8 && AV_PAIR_HBM == 9 && AV_PAIR_LDS_DL == 10 && AV_PAIR_HBM_DL == 11 &&
                  AV_PAIR_LDS_GN == 12 && AV_PAIR_HBM_GN == 13 && AV_PAIR2_LDS == 14 && AV_PAIR2_HBM == 15,
              "mtr_debug_launch_counts: enum ApplyVariant changed, update include/mtr.h and engine.py");

int mtr_debug_launch_counts(mtr_engine* e, int64_t* out, int n) {
    constexpr int kWords = mtr_engine::kCensusVariants + 5;
    if (!e || (!out && n > 0)) return -1;
    const mtr_engine::Census& cs = e->census;
    int64_t v[kWords];
    for (int i = 0; i < mtr_engine::kCensusVariants; i++) v[i] = cs.variant[i];
    v[16] = cs.fixed_cap;
    v[17] = cs.min_cap;
    v[18] = cs.max_cap;
    v[19] = cs.global_mode;
    v[20] = cs.max_lds_cap;
    for (int i = 0; i < n && i < kWords; i++) out[i] = v[i];
    return kWords;
}

int mtr_stats(mtr_engine* e, int64_t* out, int32_t n) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<DocHdr> h(e->n_docs);
    if (e->n_docs) HIPCHK(hipMemcpy(h.data(), e->hdr.p, e->n_docs * sizeof(DocHdr), hipMemcpyDeviceToHost));
    unsigned long long st[3] = {0, 0, 0};
    {  // per-document counters [doc][4]: ops applied, sum of leaves before ops, inserted units
        std::vector<unsigned long long> sd(size_t(e->n_docs) * 4);
        if (e->n_docs) HIPCHK(hipMemcpy(sd.data(), e->stat.p, sd.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (uint32_t d = 0; d < e->n_docs; d++)
            for (int q = 0; q < 3; q++) st[q] += sd[size_t(d) * 4 + q];
    }
    int64_t v[10] = {int64_t(st[0]), e->n_docs, 0, 0, 0, e->launches, 0, 0, int64_t(st[1]), int64_t(st[2])};
    for (auto& x : h) {
        v[2] = std::max<int64_t>(v[2], x.nseg);
        v[3] += x.nseg;
        v[4] += x.status != MTR_OK;
        v[6] = std::max<int64_t>(v[6], x.max_heap);
        v[7] = std::max<int64_t>(v[7], x.textused);
    }
    for (int i = 0; i < n && i < 10; i++) out[i] = v[i];
    return MTR_OK;
}

int mtr_last_timing(mtr_engine* e, double* out, int32_t n) {
    // a delta build's time: flags + scan, and the gather; a novel build's: classify, scan, gather
    const mtr::Compacted &d = e->summary_delta, &nv = e->novel.res;
    const double t_delta = double(d.t_scan) + double(d.t_gather);
    const double t_novel = double(e->novel.t_classify) + double(nv.t_scan) + double(nv.t_gather);
    double v[17] = {e->t_apply,  e->t_summary, e->launches * 1.0, e->t_kernels, e->ids.t,
                    t_delta,     d.t_gather,   e->tree.t,         t_novel,      nv.t_gather,
                    e->novel.t_classify, e->cache.t_trim, e->cache.t_ages,
                    e->hand.copied, e->hand.t_ids, e->hand.t_novel, e->hand.ranges ? 1.0 : 0.0};
    for (int i = 0; i < n && i < 17; i++) out[i] = v[i];
    return MTR_OK;
}

int mtr_profile(mtr_engine* e, uint64_t* out, int32_t n, int32_t reset) {
    if (!e || !out) return MTR_ERR_BAD_OP;
    unsigned long long v[64] = {0};
#ifdef MTR_PROF
    if (hipStreamSynchronize(e->stream) != hipSuccess) return MTR_ERR_ASSERT;
    if (!e->prof.p) {
        if (e->prof.ensure(64) || hipMemset(e->prof.p, 0, sizeof(v)) != hipSuccess) return MTR_ERR_ASSERT;
    }
    if (hipMemcpy(v, e->prof.p, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return MTR_ERR_ASSERT;
    if (reset && hipMemset(e->prof.p, 0, sizeof(v)) != hipSuccess) return MTR_ERR_ASSERT;
#else
    (void)reset;
#endif
    for (int i = 0; i < n && i < 64; i++) out[i] = v[i];
#ifdef MTR_PROF
    return MTR_OK;
#else
    return MTR_ERR_UNSUPPORTED;
#endif
}

}  // extern "C"

int mtr::summary_reserve(mtr_engine* e) {
    SParams P;
    return summary_params(e, P);
}

int mtr::summary_size_pass(mtr_engine* e, uint32_t lo, uint32_t hi, hipStream_t s) {
    SParams P;
    if (summary_params(e, P)) return -1;
    P.doc_base = lo;
    summary_size_kernel<<<hi - lo, 64, 0, s>>>(P);
    HIPCHK(hipGetLastError());
    return 0;
}

int mtr::summary_write_pass(mtr_engine* e, uint32_t lo, uint32_t hi, hipStream_t s) {
    SParams P;
    if (summary_params(e, P)) return -1;
    P.doc_base = lo;
    P.out = e->out.p;
    summary_write_kernel<<<hi - lo, 64, 0, s>>>(P);
    HIPCHK(hipGetLastError());
    return 0;
}
