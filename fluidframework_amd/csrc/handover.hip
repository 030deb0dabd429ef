// handover.hip -- host side of the summary hand-over calls of include/mtr.h: git blob ids (blob_id.hip), git tree
// ids (tree_id.hip), the incremental delta against a baseline (summary_delta.hip) and the blob-id cache with its novel
// pass (blob_cache.hip).  Orchestration only: it sizes the engine's hand-over structs (engine.hip.h), calls those
// units' launchers and reads results back; it has no kernel of its own and does not see the apply kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "blob_cache.hip.h"
#include "blob_id.hip.h"
#include "engine.hip.h"
#include "summary_delta.hip.h"
#include "tree_id.hip.h"

using namespace mtr;

// the ids of every document's blobs, into e->ids.ids (blob_id.hip): the blob table from the records (the serial and the
// pipelined summary leave the same layout: out_off / out_size per document on the device), one read-back of the
// blob count to size the buffers, then one lane per blob
static int blob_ids_build(mtr_engine* e) {
    BlobIds& b = e->ids;
    if (b.count >= 0) return 0;
    const uint32_t n = e->n_docs;
    if (b.first.ensure(size_t(n) + 2)) return -1;
    HIPCHK(hipEventRecord(e->ev[2], e->stream));
    HIPCHK(blob_table_count(e->out.p, e->out_off.p, e->out_size.p, n, b.first.p, e->stream));
    uint32_t tail[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(tail, b.first.p + n, sizeof(tail), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (tail[1]) {
        set_err("mtr_summary_blob_ids: a summary record's blob lengths do not add up to its size");
        return -1;
    }
    const uint32_t nb = tail[0];
    if (b.boff.ensure(nb) || b.blen.ensure(nb) || b.ids.ensure(size_t(nb) * 5)) return -1;
    HIPCHK(blob_table_fill(e->out.p, e->out_off.p, b.first.p, n, b.boff.p, b.blen.p, e->stream));
    HIPCHK(git_blob_ids_launch(e->out.p, b.boff.p, b.blen.p, nb, b.ids.p, e->stream));
    HIPCHK(hipEventRecord(e->ev[3], e->stream));
    HIPCHK(hipEventSynchronize(e->ev[3]));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->ev[2], e->ev[3]));
    b.t = ms;
    b.count = nb;
    return 0;
}

// first = ids.first[lo .. hi]: the first blob of each document of the range, and the range's end
static int read_first(mtr_engine* e, uint32_t lo, uint32_t hi, std::vector<uint32_t>& first) {
    first.resize(size_t(hi - lo) + 1);
    HIPCHK(hipMemcpyAsync(first.data(), e->ids.first.p + lo, first.size() * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

int64_t mtr_summary_blob_ids(mtr_engine* e, uint32_t lo, uint32_t hi, uint8_t* out, int64_t cap_blobs,
                             int64_t* doc_first) {
    if (summary_range(e, "mtr_summary_blob_ids", lo, hi)) return -1;
    if (lo == hi) {
        if (doc_first) doc_first[0] = 0;
        return 0;
    }
    HIPCHK(hipSetDevice(e->device));
    std::vector<uint32_t> first;
    if (blob_ids_build(e) || read_first(e, lo, hi, first)) return -1;
    const int64_t count = int64_t(first[hi - lo]) - int64_t(first[0]);
    if (count > cap_blobs || (count > 0 && !out)) return -count;
    if (count)
        HIPCHK(hipMemcpy(out, e->ids.ids.p + size_t(first[0]) * 5, size_t(count) * MTR_BLOB_ID_BYTES,
                         hipMemcpyDeviceToHost));
    if (doc_first)
        for (uint32_t d = lo; d <= hi; d++) doc_first[d - lo] = int64_t(first[d - lo]) - int64_t(first[0]);
    return count;
}

int mtr_git_blob_ids(mtr_engine* e, const uint8_t* bytes, const int64_t* off, uint32_t n, uint8_t* out) {
    if (n == 0) return MTR_OK;
    if (!bytes || !off || !out || off[0] < 0) {
        set_err("mtr_git_blob_ids: null argument or negative offset");
        return -1;
    }
    // the upload starts at a 16-byte boundary of the caller's offsets, so a blob keeps its alignment
    const int64_t base = off[0] & ~int64_t(15);
    std::vector<uint64_t> boff(n);
    std::vector<uint32_t> blen(n);
    for (uint32_t i = 0; i < n; i++) {
        const int64_t len = off[i + 1] - off[i];
        if (len < 0 || len > int64_t(UINT32_MAX)) {
            set_err("mtr_git_blob_ids: blob " + std::to_string(i) + " has a negative length or more than 2^32 - 1 bytes");
            return -1;
        }
        boff[i] = uint64_t(off[i] - base);
        blen[i] = uint32_t(len);
    }
    const size_t total = size_t(off[n] - base);
    HIPCHK(hipSetDevice(e->device));
    RawIds& r = e->raw;
    if (r.bytes.ensure(total + 16) || r.off.ensure(n) || r.len.ensure(n) || r.ids.ensure(size_t(n) * 5)) return -1;
    if (total) HIPCHK(hipMemcpyAsync(r.bytes.p, bytes + base, total, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(r.off.p, boff.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(r.len.p, blen.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(git_blob_ids_launch(r.bytes.p, r.off.p, r.len.p, n, r.ids.p, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));  // (also: boff / blen may go out of scope)
    HIPCHK(hipMemcpy(out, r.ids.p, size_t(n) * MTR_BLOB_ID_BYTES, hipMemcpyDeviceToHost));
    return MTR_OK;
}

// ---- git tree ids (tree_id.hip): the tree a summarizer uploads, named before storage answers
namespace {

// the name git sorts a tree entry by: a subtree compares as its name followed by '/'
std::string tree_sort_name(const mtr_tree_entry& x) {
    std::string s(x.name, x.name_len);
    if (x.mode == 040000u) s.push_back('/');
    return s;
}

// Validates the entries [a, b) of one tree (mode, name length, no NUL or '/' in a name, no name twice; `taken` says
// whether the engine makes an entry of that name) and appends them to `sorted` in git's order.  `what` names the tree
// in the error message.
int tree_entries_sorted(const char* fn, const std::string& what, const mtr_tree_entry* x, int64_t a, int64_t b,
                        const std::function<bool(const std::string&)>& taken, std::vector<mtr_tree_entry>& sorted) {
    const size_t base = sorted.size();
    for (int64_t i = a; i < b; i++) {
        const mtr_tree_entry& v = x[i];
        const std::string at = std::string(fn) + ": " + what + ", entry " + std::to_string(i - a);
        if (v.mode != 0100644u && v.mode != 040000u) {
            set_err(at + ": mode is neither 0100644 (blob) nor 040000 (subtree)");
            return -1;
        }
        if (v.name_len < 1 || v.name_len > MTR_TREE_NAME_MAX) {
            set_err(at + ": name length " + std::to_string(int(v.name_len)) + " is outside 1.." +
                    std::to_string(MTR_TREE_NAME_MAX));
            return -1;
        }
        const std::string name(v.name, v.name_len);
        if (name.find('\0') != std::string::npos || name.find('/') != std::string::npos) {
            set_err(at + ": the name holds a NUL or a '/'");
            return -1;
        }
        if (taken(name)) {
            set_err(at + ": the name '" + name + "' repeats an entry the engine makes");
            return -1;
        }
        sorted.push_back(v);
    }
    std::sort(sorted.begin() + base, sorted.end(),
              [](const mtr_tree_entry& p, const mtr_tree_entry& q) { return tree_sort_name(p) < tree_sort_name(q); });
    // (equal names are neighbours unless they differ in kind: "a" the blob and "a" the subtree sort as "a" and "a/")
    std::vector<std::string> names;
    for (size_t i = base; i < sorted.size(); i++) names.emplace_back(sorted[i].name, sorted[i].name_len);
    std::sort(names.begin(), names.end());
    for (size_t i = 1; i < names.size(); i++)
        if (names[i] == names[i - 1]) {
            set_err(std::string(fn) + ": " + what + ": the name '" + names[i] + "' appears twice");
            return -1;
        }
    return 0;
}

// is `name` "body_<k>" with k a decimal number without leading zeros below `chunks`
bool is_chunk_name(const std::string& name, uint32_t chunks) {
    if (name.size() < 6 || name.size() > 15 || name.compare(0, 5, "body_") != 0) return false;
    if (name[5] == '0' && name.size() > 6) return false;
    uint64_t k = 0;
    for (size_t i = 5; i < name.size(); i++) {
        if (name[i] < '0' || name[i] > '9') return false;
        k = k * 10 + uint64_t(name[i] - '0');
    }
    return k < chunks;
}

// uploads the sorted host entries and their per-tree ranges, sizes the work buffers (body_bound: an upper bound of
// all tree bodies together) and fills the job's pointers to them
int tree_job_buffers(mtr_engine* e, const char* fn, const std::vector<mtr_tree_entry>& sorted,
                     const std::vector<uint32_t>& x_first, uint32_t n, uint64_t body_bound, TreeJob& job) {
    if (body_bound > uint64_t(UINT32_MAX) - 64) {
        set_err(std::string(fn) + ": the tree bodies may exceed 2^32 bytes together; ask for a smaller range");
        return -1;
    }
    if (e->tree.ev.ensure(2) || e->tree.off.ensure(size_t(n) + 1) || e->tree.body.ensure(size_t(body_bound) + 16) ||
        e->tree.out.ensure(size_t(n) * 5))
        return -1;
    job.x_first = nullptr;
    job.x = nullptr;
    if (!sorted.empty()) {
        if (e->tree.x.ensure(sorted.size()) || e->tree.x_first.ensure(x_first.size())) return -1;
        HIPCHK(hipMemcpyAsync(e->tree.x.p, sorted.data(), sorted.size() * sizeof(mtr_tree_entry), hipMemcpyHostToDevice,
                              e->stream));
        HIPCHK(hipMemcpyAsync(e->tree.x_first.p, x_first.data(), x_first.size() * sizeof(uint32_t),
                              hipMemcpyHostToDevice, e->stream));
        // (pageable sources: the copies have left the host vectors when the calls return)
        job.x_first = e->tree.x_first.p;
        job.x = e->tree.x.p;
    }
    job.n = n;
    job.off = e->tree.off.p;
    job.body = e->tree.body.p;
    job.out = e->tree.out.p;
    return 0;
}

// the ids of the job's trees, n x 20 bytes, to the host; level 1 follows when some document is a matrix vector
int tree_job_run(mtr_engine* e, TreeJob& job, bool two_levels, uint8_t* out) {
    HIPCHK(hipEventRecord(e->tree.ev[0], e->stream));
    job.level = 0;
    HIPCHK(tree_ids_launch(job, e->stream));
    if (two_levels) {
        job.level = 1;
        HIPCHK(tree_ids_launch(job, e->stream));
    }
    HIPCHK(hipEventRecord(e->tree.ev[1], e->stream));
    HIPCHK(hipMemcpyAsync(out, e->tree.out.p, size_t(job.n) * MTR_BLOB_ID_BYTES, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->tree.ev[0], e->tree.ev[1]));
    e->tree.t = ms;
    return 0;
}

}  // namespace

int64_t mtr_summary_tree_ids(mtr_engine* e, uint32_t lo, uint32_t hi, const mtr_tree_entry* extra,
                             const int64_t* extra_first, uint8_t* out) {
    static const char* fn = "mtr_summary_tree_ids";
    if (summary_range(e, fn, lo, hi)) return -1;
    if (lo == hi) return 0;
    const uint32_t n = hi - lo;
    if (!out || (extra && !extra_first)) {
        set_err("mtr_summary_tree_ids: out is null, or extra is given without extra_first");
        return -1;
    }
    if (extra)
        for (uint32_t i = 0; i < n; i++)
            if (extra_first[i + 1] < extra_first[i] || extra_first[0] < 0) {
                set_err("mtr_summary_tree_ids: extra_first is negative or decreases at document " + std::to_string(lo + i));
                return -1;
            }
    HIPCHK(hipSetDevice(e->device));
    std::vector<uint32_t> first;
    if (blob_ids_build(e) || read_first(e, lo, hi, first)) return -1;
    const bool v1 = e->opt.snapshot_v1 != 0;
    bool any_vec = false;
    std::vector<mtr_tree_entry> sorted;
    std::vector<uint32_t> x_first(size_t(n) + 1, 0);
    uint64_t bound = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t d = lo + i, nb = first[i + 1] - first[i];
        const bool vec = d < e->h_kind.size() && e->h_kind[d] != 0;
        any_vec = any_vec || vec;
        const uint32_t segs = vec ? (nb ? nb - 1 : 0) : nb;  // the blobs named header, body...
        if (!v1 && segs > 2) {
            set_err("mtr_summary_tree_ids: document " + std::to_string(d) + " has " + std::to_string(segs) +
                    " blobs, but the legacy format names two (header, body)");
            return -1;
        }
        if (extra) {
            auto taken = [&](const std::string& name) {
                if (vec) return nb > 0 && (name == "segments" || name == "handleTable");
                if (segs > 0 && name == "header") return true;
                return v1 ? is_chunk_name(name, segs ? segs - 1 : 0) : (segs > 1 && name == "body");
            };
            if (tree_entries_sorted(fn, "document " + std::to_string(d), extra, extra_first[i], extra_first[i + 1], taken,
                                    sorted))
                return -1;
        }
        if (sorted.size() > size_t(UINT32_MAX)) {
            set_err("mtr_summary_tree_ids: more than 2^32 - 1 extra entries");
            return -1;
        }
        x_first[i + 1] = uint32_t(sorted.size());
        // (a matrix vector's two trees share the body buffer one after the other: the larger of the two bounds it)
        bound += kTreeEngineEntryMax * std::max<uint64_t>(segs, 2);
    }
    bound += uint64_t(sorted.size()) * (7 + MTR_TREE_NAME_MAX + 1 + MTR_BLOB_ID_BYTES);
    TreeJob job{};
    job.v1 = v1;
    job.first = e->ids.first.p + lo;
    job.kind = any_vec ? e->dkind.p + lo : nullptr;
    job.blob_ids = e->ids.ids.p;
    if (tree_job_buffers(e, fn, sorted, x_first, n, bound, job)) return -1;
    // (out is written by the one copy at the end: an error before it leaves it untouched)
    if (tree_job_run(e, job, any_vec, out)) return -1;
    return int64_t(n);
}

int mtr_git_tree_ids(mtr_engine* e, const mtr_tree_entry* entries, const int64_t* first, uint32_t n, uint8_t* out) {
    static const char* fn = "mtr_git_tree_ids";
    if (n == 0) return MTR_OK;
    if (!first || !out || first[0] < 0 || (!entries && first[n] != first[0])) {
        set_err("mtr_git_tree_ids: null argument or negative offset");
        return -1;
    }
    std::vector<mtr_tree_entry> sorted;
    std::vector<uint32_t> x_first(size_t(n) + 1, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (first[i + 1] < first[i]) {
            set_err("mtr_git_tree_ids: first decreases at tree " + std::to_string(i));
            return -1;
        }
        if (tree_entries_sorted(fn, "tree " + std::to_string(i), entries, first[i], first[i + 1],
                                [](const std::string&) { return false; }, sorted))
            return -1;
        if (sorted.size() > size_t(UINT32_MAX)) {
            set_err("mtr_git_tree_ids: more than 2^32 - 1 entries");
            return -1;
        }
        x_first[i + 1] = uint32_t(sorted.size());
    }
    if (!e) {
        set_err("mtr_git_tree_ids: no engine");
        return -1;
    }
    HIPCHK(hipSetDevice(e->device));
    TreeJob job{};
    if (tree_job_buffers(e, fn, sorted, x_first, n,
                         uint64_t(sorted.size()) * (7 + MTR_TREE_NAME_MAX + 1 + MTR_BLOB_ID_BYTES), job))
        return -1;
    if (tree_job_run(e, job, false, out)) return -1;
    return MTR_OK;
}

// ---- incremental hand-over: a baseline of blob ids, and the current summary's delta against it
int mtr_summary_set_baseline(mtr_engine* e) {
    if (!e->summarized) {
        set_err("mtr_summary_set_baseline: no summary (call mtr_summarize first)");
        return -1;
    }
    HIPCHK(hipSetDevice(e->device));
    if (blob_ids_build(e)) return -1;
    const uint32_t n = e->n_docs;
    const size_t nb = size_t(e->ids.count);
    e->summary_delta.valid = false;
    e->base.docs = 0;
    if (e->base.first.ensure(size_t(n) + 1) || e->base.ids.ensure(nb * 5)) return -1;
    HIPCHK(hipMemcpyAsync(e->base.first.p, e->ids.first.p, (size_t(n) + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                          e->stream));
    if (nb)
        HIPCHK(hipMemcpyAsync(e->base.ids.p, e->ids.ids.p, nb * MTR_BLOB_ID_BYTES, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->base.docs = n;
    return MTR_OK;
}

int mtr_summary_set_baseline_ids(mtr_engine* e, const uint8_t* ids, const int64_t* doc_first, uint32_t n_docs) {
    if (!doc_first || doc_first[0] != 0) {
        set_err("mtr_summary_set_baseline_ids: doc_first is null or does not start at 0");
        return -1;
    }
    std::vector<uint32_t> first(size_t(n_docs) + 1);
    for (uint32_t d = 0; d <= n_docs; d++) {
        if (doc_first[d] > int64_t(UINT32_MAX) || (d && doc_first[d] < doc_first[d - 1])) {
            set_err("mtr_summary_set_baseline_ids: doc_first decreases at document " + std::to_string(d) +
                    " or counts more than 2^32 - 1 blobs");
            return -1;
        }
        first[d] = uint32_t(doc_first[d]);
    }
    const size_t nb = first[n_docs];
    if (nb && !ids) {
        set_err("mtr_summary_set_baseline_ids: ids is null");
        return -1;
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->summary_delta.valid = false;
    e->base.docs = 0;
    if (e->base.first.ensure(first.size()) || e->base.ids.ensure(nb * 5)) return -1;
    HIPCHK(hipMemcpy(e->base.first.p, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (nb) HIPCHK(hipMemcpy(e->base.ids.p, ids, nb * MTR_BLOB_ID_BYTES, hipMemcpyHostToDevice));
    e->base.docs = n_docs;
    return MTR_OK;
}

int mtr_summary_clear_baseline(mtr_engine* e) {
    e->summary_delta.valid = false;
    e->base.docs = 0;
    return MTR_OK;
}

// ---- what the delta and the novel result share: a Compacted, built by the flags-scan-gather pass of summary_delta.hip

// the buffers a pass over nb blobs writes before its gather, and the pass's events
static int compacted_reserve(Compacted& c, uint32_t nb) {
    const bool failed = c.ev.ensure(4) || c.flags.ensure(nb) || c.off.ensure(size_t(nb) + 1) || c.tot.ensure(2) ||
                        c.rank.ensure(size_t(nb) + 1) || c.chg_off.ensure(size_t(nb) + 1) || c.chg_src.ensure(nb);
    return failed ? -1 : 0;
}

// The pass from the scan on; the caller has recorded c.ev[0] and launched the kernels that fill c.flags and the chosen
// blobs' lengths in c.off, and sets c.valid afterwards.  The 64-bit scan, one read-back of (chosen blobs, their bytes)
// to size the compact buffer, then the gather; the read-back and the allocation lie between the two timed spans.
// `too_many` is the caller's error text for a count above nb.
static int compacted_finish(mtr_engine* e, Compacted& c, uint32_t nb, const char* too_many) {
    HIPCHK(delta_scan_launch(c.flags.p, e->ids.boff.p, nb, c.off.p, c.rank.p, c.chg_off.p, c.chg_src.p, c.tot.p,
                             e->stream));
    HIPCHK(hipEventRecord(c.ev[1], e->stream));
    uint64_t tot[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(tot, c.tot.p, sizeof(tot), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (tot[0] > nb) {
        set_err(too_many);
        return -1;
    }
    if (c.compact.ensure(size_t(tot[1]) + 16)) return -1;
    HIPCHK(hipEventRecord(c.ev[2], e->stream));
    HIPCHK(delta_gather_launch(e->out.p, c.chg_off.p, c.chg_src.p, uint32_t(tot[0]), tot[1], c.compact.p, e->stream));
    HIPCHK(hipEventRecord(c.ev[3], e->stream));
    HIPCHK(hipEventSynchronize(c.ev[3]));
    HIPCHK(hipEventElapsedTime(&c.t_scan, c.ev[0], c.ev[1]));
    HIPCHK(hipEventElapsedTime(&c.t_gather, c.ev[2], c.ev[3]));
    return 0;
}

// the blob range [b0, b1) of documents [lo, hi), its chosen blobs and its byte range in the compact buffer
struct DeltaRange {
    std::vector<uint32_t> first;  // ids.first[lo .. hi]
    int64_t b0 = 0, count = 0, changed = 0, o0 = 0, bytes = 0;
};
static int compacted_range(mtr_engine* e, Compacted& c, uint32_t lo, uint32_t hi, DeltaRange& r) {
    if (read_first(e, lo, hi, r.first)) return -1;
    const uint32_t b0 = r.first[0], b1 = r.first[hi - lo];
    uint64_t off[2] = {0, 0};
    uint32_t rank[2] = {0, 0};
    HIPCHK(hipMemcpy(&off[0], c.off.p + b0, sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&off[1], c.off.p + b1, sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&rank[0], c.rank.p + b0, sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&rank[1], c.rank.p + b1, sizeof(uint32_t), hipMemcpyDeviceToHost));
    r.b0 = b0;
    r.count = int64_t(b1) - int64_t(b0);
    r.changed = int64_t(rank[1]) - int64_t(rank[0]);
    r.o0 = int64_t(off[0]);
    r.bytes = int64_t(off[1] - off[0]);
    return 0;
}

// the range to the caller's buffers, which the caller has checked: its chosen bytes, contiguous in the compact buffer
// (it is built for all documents in order; a null `out` leaves them where they are), the caller's byte per blob
// (`mark`: all blobs on the device; the delta's flags, the novel states), each blob's offset in the bytes, and each
// document's first blob
static int compacted_copy_out(const Compacted& c, const DeltaRange& r, uint8_t* out, const uint8_t* mark,
                              uint8_t* mark_out, int64_t* blob_off, int64_t* doc_first) {
    if (out && r.bytes) HIPCHK(hipMemcpy(out, c.compact.p + r.o0, size_t(r.bytes), hipMemcpyDeviceToHost));
    if (r.count) HIPCHK(hipMemcpy(mark_out, mark + r.b0, size_t(r.count), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(blob_off, c.off.p + r.b0, (size_t(r.count) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k <= r.count; k++) blob_off[k] -= r.o0;
    if (doc_first)
        for (size_t d = 0; d < r.first.size(); d++) doc_first[d] = int64_t(r.first[d]) - r.b0;
    return 0;
}

// the delta of every document against the baseline: flags and changed lengths (summary_delta.hip), then the shared pass
static int delta_build(mtr_engine* e) {
    if (blob_ids_build(e)) return -1;
    Compacted& c = e->summary_delta;
    if (c.valid) return 0;
    const uint32_t nb = uint32_t(e->ids.count);
    if (compacted_reserve(c, nb)) return -1;
    HIPCHK(hipEventRecord(c.ev[0], e->stream));
    HIPCHK(delta_flag_launch(e->ids.first.p, e->n_docs, e->ids.blen.p, e->ids.ids.p, nb, e->base.first.p, e->base.ids.p,
                             e->base.docs, c.flags.p, c.off.p, e->stream));
    if (compacted_finish(e, c, nb, "mtr_summary_delta: internal error: more changed blobs than blobs")) return -1;
    c.valid = true;
    return 0;
}

int mtr_summary_delta_info(mtr_engine* e, uint32_t lo, uint32_t hi, int64_t* n_blobs, int64_t* n_changed,
                           int64_t* changed_bytes) {
    if (summary_range(e, "mtr_summary_delta_info", lo, hi)) return -1;
    DeltaRange r;
    if (lo < hi) {
        HIPCHK(hipSetDevice(e->device));
        if (delta_build(e) || compacted_range(e, e->summary_delta, lo, hi, r)) return -1;
    }
    if (n_blobs) *n_blobs = r.count;
    if (n_changed) *n_changed = r.changed;
    if (changed_bytes) *changed_bytes = r.bytes;
    return MTR_OK;
}

int64_t mtr_summary_delta(mtr_engine* e, uint32_t lo, uint32_t hi, uint8_t* out, int64_t cap_bytes, uint8_t* flags,
                          int64_t* blob_off, int64_t cap_blobs, int64_t* doc_first) {
    if (summary_range(e, "mtr_summary_delta", lo, hi)) return -1;
    if (lo == hi) {
        if (doc_first) doc_first[0] = 0;
        if (blob_off) blob_off[0] = 0;
        return 0;
    }
    HIPCHK(hipSetDevice(e->device));
    DeltaRange r;
    if (delta_build(e) || compacted_range(e, e->summary_delta, lo, hi, r)) return -1;
    if (r.bytes > cap_bytes || r.count > cap_blobs || (r.bytes > 0 && !out) || (r.count > 0 && !flags) || !blob_off) {
        set_err("mtr_summary_delta: buffers smaller than mtr_summary_delta_info reports");
        return MTR_SUMMARY_TOO_SMALL;
    }
    const Compacted& c = e->summary_delta;
    if (compacted_copy_out(c, r, out, c.flags.p, flags, blob_off, doc_first)) return -1;
    return r.bytes;
}

// ---- the blob-id cache: the set of ids storage holds, and the current summary sorted against it (blob_cache.hip)
namespace {

constexpr uint64_t kCacheMaxEntries = 0x7fffffffull;  // 2^31 - 1

// an empty cache without buffers, work buffers included, and at generation 0 (BlobCache::release):
// mtr_blob_cache_clear, and the way out of an add that failed half way.  The next add starts small again.
void cache_reset(mtr_engine* e) {
    if (e->cache.count) e->novel.res.valid = false;
    e->cache.release();
}

// a fresh id table for `entries` ids, never smaller than what fills the first slot array by half, and a stamp word for
// each entry it has room for
int cache_table_alloc(DevBuf<uint32_t>& table, DevBuf<uint32_t>& stamps, size_t entries) {
    return table.ensure(std::max<size_t>(entries, kCacheMinSlots / 2) * 5) || stamps.ensure(table.n / 5) ? -1 : 0;
}

// the slots that keep `entries` ids at most half full, starting from `from`
uint64_t cache_slots_for(uint64_t from, uint64_t entries) {
    uint64_t want = from;
    while (want < 2 * entries) want <<= 1;
    return want;
}

// a slot array that keeps `entries` ids at most half full: doubled from its present size (kCacheMinSlots at first),
// and the id table re-inserted into the new one by the insert kernel
int cache_reserve_slots(mtr_engine* e, uint64_t entries) {
    BlobCache& bc = e->cache;
    const uint64_t want = cache_slots_for(bc.nslots ? bc.nslots : kCacheMinSlots, entries);
    if (want == bc.nslots) return 0;
    HIPCHK(hipStreamSynchronize(e->stream));
    bc.nslots = 0;
    if (bc.slots.ensure(size_t(want))) {
        cache_reset(e);  // (the old slot array is gone)
        return -1;
    }
    HIPCHK(hipMemsetAsync(bc.slots.p, 0, size_t(want) * sizeof(uint32_t), e->stream));
    HIPCHK(cache_insert_launch(nullptr, 0, bc.ids.p, bc.count, bc.slots.p, uint32_t(want - 1), nullptr, e->stream));
    bc.nslots = want;
    return 0;
}

// an id table of at least `entries` entries and a stamp word for each; the present ones are kept (DevBuf::ensure
// alone would drop them)
int cache_reserve_table(mtr_engine* e, uint64_t entries) {
    BlobCache& bc = e->cache;
    if (bc.ids.p && bc.ids.n >= size_t(entries) * 5) return 0;
    DevBuf<uint32_t> grown, stamps;  // (at least doubled: ids.n is five words for each entry there is room for)
    if (cache_table_alloc(grown, stamps, std::max<size_t>(size_t(entries), 2 * (bc.ids.n / 5)))) return -1;
    if (bc.count) {
        HIPCHK(hipMemcpyAsync(grown.p, bc.ids.p, size_t(bc.count) * MTR_BLOB_ID_BYTES, hipMemcpyDeviceToDevice,
                              e->stream));
        HIPCHK(hipMemcpyAsync(stamps.p, bc.stamp.p, size_t(bc.count) * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                              e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    bc.ids.swap(grown);  // (the locals free the old table and stamps, and their share of the live bytes)
    bc.stamp.swap(stamps);
    return 0;
}

// adds the n ids at src (device memory, written by an earlier operation on the stream), then stamps every one of
// them, held or new: with the generation, or with generation - age[i] (age: device memory, an import's)
int cache_add_device(mtr_engine* e, const char* fn, const uint32_t* src, uint64_t n, const uint32_t* age = nullptr) {
    BlobCache& bc = e->cache;
    if (n == 0) return 0;
    if (uint64_t(bc.count) + n > kCacheMaxEntries) {
        set_err(std::string(fn) + ": the cache would pass 2^31 - 1 entries");
        return -1;
    }
    const uint32_t held = bc.count, cnt = uint32_t(n);
    if (cache_reserve_slots(e, uint64_t(held) + n) || bc.where.ensure(cnt) || bc.isnew.ensure(cnt) ||
        bc.rank.ensure(size_t(cnt) + 1) || bc.tot.ensure(1))
        return -1;
    const uint32_t mask = uint32_t(bc.nslots - 1);
    HIPCHK(cache_insert_launch(bc.ids.p, held, src, cnt, bc.slots.p, mask, bc.where.p, e->stream));
    HIPCHK(cache_rank_launch(bc.slots.p, bc.where.p, held, cnt, bc.isnew.p, bc.rank.p, bc.tot.p, e->stream));
    uint32_t fresh = 0;
    HIPCHK(hipMemcpyAsync(&fresh, bc.tot.p, sizeof(fresh), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (fresh > cnt) {
        set_err(std::string(fn) + ": internal error: more new ids than ids");
        return -1;
    }
    if (fresh) {  // (else every id was held: the set and what was built from it stand)
        e->novel.res.valid = false;
        // (from here the slots name source ids: a failure before the commit has run leaves no usable set)
        if (cache_reserve_table(e, uint64_t(held) + fresh) ||
            cache_commit_launch(src, bc.isnew.p, bc.rank.p, bc.where.p, held, cnt, bc.ids.p, bc.slots.p, e->stream) !=
                hipSuccess ||
            hipMemsetAsync(bc.stamp.p + held, 0, size_t(fresh) * sizeof(uint32_t), e->stream) != hipSuccess ||
            hipStreamSynchronize(e->stream) != hipSuccess) {
            cache_reset(e);
            set_err(std::string(fn) + ": appending the new ids failed; the cache is now empty");
            return -1;
        }
        bc.count = held + fresh;
    }
    // membership is settled; the stamps move alone and drop nothing that was built from the set
    HIPCHK(cache_stamp_launch(bc.ids.p, bc.slots.p, mask, src, age, bc.gen, cnt, bc.stamp.p, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
}

// the caller's n ids to cache.in
int cache_upload(mtr_engine* e, const uint8_t* ids, uint64_t n) {
    if (e->cache.in.ensure(size_t(n) * 5)) return -1;
    HIPCHK(hipMemcpyAsync(e->cache.in.p, ids, size_t(n) * MTR_BLOB_ID_BYTES, hipMemcpyHostToDevice, e->stream));
    return 0;
}

int cache_engine(const mtr_engine* e, const char* fn) {
    if (e) return 0;
    set_err(std::string(fn) + ": no engine");
    return -1;
}

int cache_args(const mtr_engine* e, const char* fn, const void* ids, int64_t n) {
    if (e && n >= 0 && (n == 0 || ids) && uint64_t(n) <= kCacheMaxEntries) return 0;
    set_err(std::string(fn) + ": no engine, null ids, or a count that is negative or above 2^31 - 1");
    return -1;
}

}  // namespace

int mtr_blob_cache_add(mtr_engine* e, const uint8_t* ids, int64_t n) {
    static const char* fn = "mtr_blob_cache_add";
    if (cache_args(e, fn, ids, n)) return -1;
    if (n == 0) return MTR_OK;
    HIPCHK(hipSetDevice(e->device));
    if (cache_upload(e, ids, uint64_t(n)) || cache_add_device(e, fn, e->cache.in.p, uint64_t(n))) return -1;
    return MTR_OK;
}

int mtr_blob_cache_add_summary(mtr_engine* e) {
    static const char* fn = "mtr_blob_cache_add_summary";
    if (!e || !e->summarized) {
        set_err("mtr_blob_cache_add_summary: no summary (call mtr_summarize first)");
        return -1;
    }
    if (e->cache.gen == UINT32_MAX) {
        set_err("mtr_blob_cache_add_summary: the cache is at generation 2^32 - 1");
        return -1;
    }
    HIPCHK(hipSetDevice(e->device));
    if (blob_ids_build(e)) return -1;
    e->cache.gen++;  // one acknowledged summary, one generation: its blobs are stamped with the new one
    if (cache_add_device(e, fn, e->ids.ids.p, uint64_t(e->ids.count))) return -1;
    return MTR_OK;
}

int mtr_blob_cache_clear(mtr_engine* e) {
    if (cache_engine(e, "mtr_blob_cache_clear")) return -1;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    cache_reset(e);
    return MTR_OK;
}

int64_t mtr_blob_cache_size(mtr_engine* e) {
    if (cache_engine(e, "mtr_blob_cache_size")) return -1;
    return int64_t(e->cache.count);
}

int mtr_blob_cache_has(mtr_engine* e, const uint8_t* ids, int64_t n, uint8_t* out) {
    static const char* fn = "mtr_blob_cache_has";
    if (cache_args(e, fn, ids, n)) return -1;
    if (n == 0) return MTR_OK;
    if (!out) {
        set_err("mtr_blob_cache_has: out is null");
        return -1;
    }
    if (e->cache.count == 0) {
        std::fill(out, out + n, uint8_t(0));
        return MTR_OK;
    }
    HIPCHK(hipSetDevice(e->device));
    if (cache_upload(e, ids, uint64_t(n)) || e->cache.isnew.ensure(size_t(n))) return -1;
    HIPCHK(cache_has_launch(e->cache.ids.p, e->cache.slots.p, uint32_t(e->cache.nslots - 1), e->cache.in.p, uint32_t(n),
                            e->cache.isnew.p, e->stream));
    HIPCHK(hipMemcpyAsync(out, e->cache.isnew.p, size_t(n), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return MTR_OK;
}

// ---- the cache's life cycle: generations, the age histogram, trim, export and import
namespace {

constexpr int32_t kCacheAgeBuckets = 1024;

// bc.hist[0 .. n) = the age histogram of the entries (count > 0); timed into t_ages
int cache_ages_device(mtr_engine* e, uint32_t n, unsigned long long* host) {
    BlobCache& bc = e->cache;
    if (bc.ev.ensure(6) || bc.hist.ensure(size_t(kCacheAgeBuckets) + 1)) return -1;
    HIPCHK(hipEventRecord(bc.ev[4], e->stream));
    HIPCHK(hipMemsetAsync(bc.hist.p, 0, size_t(n) * sizeof(unsigned long long), e->stream));
    HIPCHK(cache_age_hist_launch(bc.stamp.p, bc.count, bc.gen, n, bc.hist.p, e->stream));
    HIPCHK(hipEventRecord(bc.ev[5], e->stream));
    HIPCHK(hipMemcpyAsync(host, bc.hist.p, size_t(n) * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, bc.ev[4], bc.ev[5]));
    bc.t_ages = ms;
    return 0;
}

// the entries with stamp >= cutoff, counted on the device
int cache_count_device(mtr_engine* e, uint64_t cutoff, uint64_t& count) {
    if (e->cache.hist.ensure(size_t(kCacheAgeBuckets) + 1)) return -1;
    unsigned long long* cell = e->cache.hist.p + kCacheAgeBuckets;
    unsigned long long got = 0;
    HIPCHK(hipMemsetAsync(cell, 0, sizeof(got), e->stream));
    HIPCHK(cache_count_launch(e->cache.stamp.p, e->cache.count, cutoff, cell, e->stream));
    HIPCHK(hipMemcpyAsync(&got, cell, sizeof(got), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    count = got;
    return 0;
}

// drops the entries with stamp < cutoff; returns how many.  Flags and their scan, one read-back of the kept count,
// then the survivors into a fresh table and a fresh slot array filled from it; the old buffers are released.  Until
// the new buffers stand, a failure leaves the cache as it was.
int64_t cache_trim_device(mtr_engine* e, uint64_t cutoff) {
    BlobCache& bc = e->cache;
    const uint32_t count = bc.count;
    if (count == 0) return 0;
    if (bc.ev.ensure(6) || bc.keep.ensure(count) || bc.newidx.ensure(size_t(count) + 1) || bc.tot.ensure(1)) return -1;
    HIPCHK(hipEventRecord(bc.ev[0], e->stream));
    HIPCHK(cache_keep_launch(bc.stamp.p, count, cutoff, bc.keep.p, bc.newidx.p, bc.tot.p, e->stream));
    HIPCHK(hipEventRecord(bc.ev[1], e->stream));
    uint32_t kept = 0;
    HIPCHK(hipMemcpyAsync(&kept, bc.tot.p, sizeof(kept), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    float ms_flag = 0, ms_build = 0;
    HIPCHK(hipEventElapsedTime(&ms_flag, bc.ev[0], bc.ev[1]));
    if (kept > count) {
        set_err("mtr_blob_cache_trim: internal error: more survivors than entries");
        return -1;
    }
    if (kept == 0) {  // as mtr_blob_cache_clear leaves it, but for the generation
        const uint32_t gen = bc.gen;
        cache_reset(e);
        bc.gen = gen;
    } else if (kept < count) {
        const uint64_t nslots = cache_slots_for(kCacheMinSlots, kept);
        DevBuf<uint32_t> table, stamps, slots;
        if (cache_table_alloc(table, stamps, kept) || slots.ensure(size_t(nslots))) return -1;
        HIPCHK(hipEventRecord(bc.ev[2], e->stream));
        HIPCHK(cache_compact_launch(bc.ids.p, bc.stamp.p, bc.keep.p, bc.newidx.p, count, table.p, stamps.p, e->stream));
        HIPCHK(hipMemsetAsync(slots.p, 0, size_t(nslots) * sizeof(uint32_t), e->stream));
        HIPCHK(cache_insert_launch(nullptr, 0, table.p, kept, slots.p, uint32_t(nslots - 1), nullptr, e->stream));
        HIPCHK(hipEventRecord(bc.ev[3], e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipEventElapsedTime(&ms_build, bc.ev[2], bc.ev[3]));
        bc.ids.swap(table);  // (the locals free the old table, stamps and slots)
        bc.stamp.swap(stamps);
        bc.slots.swap(slots);
        bc.count = kept;
        bc.nslots = nslots;
        e->novel.res.valid = false;
    }
    bc.keep.release();  // (sized by the entries before the trim: a trim gives memory back)
    bc.newidx.release();
    bc.t_trim = double(ms_flag) + double(ms_build);
    return int64_t(count) - int64_t(kept);
}

}  // namespace

int64_t mtr_blob_cache_generation(mtr_engine* e) {
    if (cache_engine(e, "mtr_blob_cache_generation")) return -1;
    return int64_t(e->cache.gen);
}

int mtr_blob_cache_ages(mtr_engine* e, int64_t* out, int32_t n) {
    if (cache_engine(e, "mtr_blob_cache_ages")) return -1;
    if (!out || n < 1 || n > kCacheAgeBuckets) {
        set_err("mtr_blob_cache_ages: out is null, or n = " + std::to_string(n) + " is outside 1..1024");
        return -1;
    }
    std::fill(out, out + n, int64_t(0));
    if (e->cache.count == 0) return MTR_OK;
    HIPCHK(hipSetDevice(e->device));
    unsigned long long h[kCacheAgeBuckets];
    if (cache_ages_device(e, uint32_t(n), h)) return -1;
    for (int32_t a = 0; a < n; a++) out[a] = int64_t(h[a]);
    return MTR_OK;
}

int64_t mtr_blob_cache_trim(mtr_engine* e, int64_t min_generation) {
    if (cache_engine(e, "mtr_blob_cache_trim")) return -1;
    HIPCHK(hipSetDevice(e->device));
    return cache_trim_device(e, min_generation < 0 ? 0 : uint64_t(min_generation));
}

int64_t mtr_blob_cache_trim_to(mtr_engine* e, int64_t max_entries) {
    if (cache_engine(e, "mtr_blob_cache_trim_to")) return -1;
    if (max_entries < 0) {
        set_err("mtr_blob_cache_trim_to: max_entries is negative");
        return -1;
    }
    if (int64_t(e->cache.count) <= max_entries) return 0;  // (cutoff 0: everything stays)
    HIPCHK(hipSetDevice(e->device));
    // the smallest cutoff g of [0, generation + 1] that keeps at most max_entries: whole generations go, oldest first.
    // Ages below 1023 have a histogram bucket of their own; the cutoff is read from them when they cover it.
    const uint64_t gen = e->cache.gen, cap = uint64_t(max_entries);
    unsigned long long h[kCacheAgeBuckets];
    if (cache_ages_device(e, kCacheAgeBuckets, h)) return -1;
    uint64_t young = 0, cutoff = 0;
    bool found = false;
    for (uint64_t a = 0; a + 1 < uint64_t(kCacheAgeBuckets) && a <= gen && !found; a++) {
        young += h[a];
        if (young > cap) {  // keeping age a passes the cap: the cutoff lies just above its generation
            cutoff = gen - a + 1;
            found = true;
        }
    }
    if (!found) {
        // the generations 0 .. gen - 1023 share the last bucket: a search over the cutoff with the count kernel.  The
        // count does not grow with the cutoff, lo - 1 keeps too many (nothing at all does when lo = 0) and hi fits.
        uint64_t lo = 0, hi = gen - (kCacheAgeBuckets - 2);
        while (lo < hi) {  // at most 32 rounds
            const uint64_t mid = lo + (hi - lo) / 2;
            uint64_t c = 0;
            if (cache_count_device(e, mid, c)) return -1;
            if (c <= cap)
                hi = mid;
            else
                lo = mid + 1;
        }
        cutoff = lo;
    }
    return cache_trim_device(e, cutoff);
}

int64_t mtr_blob_cache_export(mtr_engine* e, uint8_t* ids, uint32_t* ages, int64_t cap) {
    if (cache_engine(e, "mtr_blob_cache_export")) return -1;
    const int64_t count = int64_t(e->cache.count);
    if (count == 0) return 0;
    if (cap < count) return -count;
    if (!ids || !ages) {
        set_err("mtr_blob_cache_export: ids or ages is null");
        return -1;
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(ids, e->cache.ids.p, size_t(count) * MTR_BLOB_ID_BYTES, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(ages, e->cache.stamp.p, size_t(count) * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int64_t i = 0; i < count; i++) ages[i] = e->cache.gen - ages[i];  // (the stamps came over)
    return count;
}

int mtr_blob_cache_import(mtr_engine* e, const uint8_t* ids, const uint32_t* ages, int64_t n) {
    static const char* fn = "mtr_blob_cache_import";
    if (cache_args(e, fn, ids, n)) return -1;
    if (n == 0) return MTR_OK;
    if (!ages) {
        set_err("mtr_blob_cache_import: ages is null");
        return -1;
    }
    HIPCHK(hipSetDevice(e->device));
    if (cache_upload(e, ids, uint64_t(n)) || e->cache.age.ensure(size_t(n))) return -1;
    HIPCHK(hipMemcpyAsync(e->cache.age.p, ages, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    // (so that generation - age is no less than 0)
    e->cache.gen = std::max(e->cache.gen, *std::max_element(ages, ages + n));
    if (cache_add_device(e, fn, e->cache.in.p, uint64_t(n), e->cache.age.p)) return -1;
    return MTR_OK;
}

// the novel result of every document against the cache: classify (probe the cache, insert the misses into the
// summary's own set), states and representatives, then the shared pass over the first occurrences (`changed` of a
// range counts them)
static int novel_build(mtr_engine* e) {
    if (blob_ids_build(e)) return -1;
    Novel& v = e->novel;
    Compacted& c = v.res;
    if (c.valid) return 0;
    if (e->ids.count > (int64_t(1) << 30)) {
        set_err("mtr_summary_novel: more than 2^30 blobs in one summary");
        return -1;
    }
    const uint32_t nb = uint32_t(e->ids.count);
    const uint64_t nslots = cache_slots_for(64, nb);
    if (v.ev.ensure(1) || v.slots.ensure(size_t(nslots)) || v.where.ensure(nb) || v.state.ensure(nb) ||
        v.rep.ensure(nb) || compacted_reserve(c, nb))
        return -1;
    const BlobCache& bc = e->cache;
    const bool cached = bc.count > 0;
    HIPCHK(hipEventRecord(v.ev[0], e->stream));
    HIPCHK(hipMemsetAsync(v.slots.p, 0, size_t(nslots) * sizeof(uint32_t), e->stream));
    HIPCHK(novel_classify_launch(e->ids.ids.p, nb, cached ? bc.ids.p : nullptr, cached ? bc.slots.p : nullptr,
                                 cached ? uint32_t(bc.nslots - 1) : 0, v.slots.p, uint32_t(nslots - 1), v.where.p,
                                 e->stream));
    HIPCHK(novel_state_launch(v.slots.p, v.where.p, e->ids.blen.p, nb, v.state.p, v.rep.p, c.flags.p, c.off.p,
                              e->stream));
    HIPCHK(hipEventRecord(c.ev[0], e->stream));  // (classified: the pass times its scan alone)
    if (compacted_finish(e, c, nb, "mtr_summary_novel: internal error: more first occurrences than blobs")) return -1;
    HIPCHK(hipEventElapsedTime(&v.t_classify, v.ev[0], c.ev[0]));
    c.valid = true;
    return 0;
}

int mtr_summary_novel_info(mtr_engine* e, uint32_t lo, uint32_t hi, int64_t* n_blobs, int64_t* n_first,
                           int64_t* first_bytes) {
    if (summary_range(e, "mtr_summary_novel_info", lo, hi)) return -1;
    DeltaRange r;
    if (lo < hi) {
        HIPCHK(hipSetDevice(e->device));
        if (novel_build(e) || compacted_range(e, e->novel.res, lo, hi, r)) return -1;
    }
    if (n_blobs) *n_blobs = r.count;
    if (n_first) *n_first = r.changed;
    if (first_bytes) *first_bytes = r.bytes;
    return MTR_OK;
}

int64_t mtr_summary_novel(mtr_engine* e, uint32_t lo, uint32_t hi, uint8_t* out, int64_t cap_bytes, uint8_t* state,
                          int64_t* rep, int64_t* blob_off, int64_t cap_blobs, int64_t* doc_first) {
    if (summary_range(e, "mtr_summary_novel", lo, hi)) return -1;
    if (lo == hi) {
        if (doc_first) doc_first[0] = 0;
        if (blob_off) blob_off[0] = 0;
        return 0;
    }
    HIPCHK(hipSetDevice(e->device));
    DeltaRange r;
    if (novel_build(e) || compacted_range(e, e->novel.res, lo, hi, r)) return -1;
    if (r.bytes > cap_bytes || r.count > cap_blobs || (r.bytes > 0 && !out) || (r.count > 0 && (!state || !rep)) ||
        !blob_off) {
        set_err("mtr_summary_novel: buffers smaller than mtr_summary_novel_info reports");
        return MTR_SUMMARY_TOO_SMALL;
    }
    std::vector<uint32_t> rep32(size_t(r.count));
    if (r.count)
        HIPCHK(hipMemcpy(rep32.data(), e->novel.rep.p + r.b0, size_t(r.count) * sizeof(uint32_t),
                         hipMemcpyDeviceToHost));
    if (compacted_copy_out(e->novel.res, r, out, e->novel.state.p, state, blob_off, doc_first)) return -1;
    for (int64_t k = 0; k < r.count; k++) rep[k] = rep32[size_t(k)] == kNoSlot ? -1 : int64_t(rep32[size_t(k)]);
    return r.bytes;
}

// ---- the hand-over passes of a pipelined run (mtr_replay_handover; the stage that issues them: apply_run.hip)
int mtr::handover_reserve(mtr_engine* e, uint32_t n, uint32_t parts, int64_t cap_blobs, int64_t cap_bytes,
                          hipStream_t s) {
    if (cap_blobs < 0 || cap_bytes < 0 || cap_blobs > (int64_t(1) << 30)) {
        set_err("mtr_replay_handover: cap_blobs or cap_bytes is negative, or cap_blobs is above 2^30");
        return -1;
    }
    e->drop_ids();  // (the buffers of the ids and of the novel result may be replaced below)
    const uint32_t cap = uint32_t(cap_blobs);
    const uint64_t nslots = cache_slots_for(64, cap);
    BlobIds& b = e->ids;
    Novel& v = e->novel;
    Compacted& c = v.res;
    mtr_engine::Handover& h = e->hand;
    if (b.first.ensure(size_t(n) + 2) || b.boff.ensure(cap) || b.blen.ensure(cap) || b.ids.ensure(size_t(cap) * 5) ||
        v.slots.ensure(size_t(nslots)) || v.where.ensure(cap) || v.state.ensure(cap) || v.rep.ensure(cap) ||
        compacted_reserve(c, cap) || c.compact.ensure(size_t(cap_bytes) + 16) ||
        h.words.ensure(size_t(parts) * 4) || h.ev.ensure(size_t(parts) * 5) || h.count_ev.ensure(parts) ||
        h.scan_ev.ensure(parts))
        return -1;
    // what the parts carry on the device starts from nothing: first[0] (the blobs before document 0) and the malformed
    // flag first[n + 1], the summary's own id set, the chosen count and bytes in res.tot
    HIPCHK(hipMemsetAsync(b.first.p, 0, sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(b.first.p + n + 1, 0, sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(v.slots.p, 0, size_t(nslots) * sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(c.tot.p, 0, 2 * sizeof(uint64_t), s));
    HIPCHK(hipMemsetAsync(c.off.p, 0, sizeof(uint64_t), s));  // (a summary without blobs: off[0], rank[0])
    HIPCHK(hipMemsetAsync(c.rank.p, 0, sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(c.chg_off.p, 0, sizeof(uint64_t), s));
    h.copied = h.t_ids = h.t_novel = 0;
    return 0;
}

int mtr::handover_count_pass(mtr_engine* e, uint32_t p, uint32_t lo, uint32_t hi, hipStream_t s) {
    HIPCHK(blob_table_count_range(e->out.p, e->out_off.p, e->out_size.p, lo, hi, e->ids.first.p,
                                  e->ids.first.p + e->n_docs + 1, e->hand.words.dev + 4 * size_t(p), s));
    HIPCHK(hipEventRecord(e->hand.count_ev[p], s));
    return 0;
}

int mtr::handover_ids_pass(mtr_engine* e, uint32_t p, uint32_t lo, uint32_t hi, uint32_t b0, uint32_t b1,
                           hipStream_t s) {
    BlobIds& b = e->ids;
    Novel& v = e->novel;
    Compacted& c = v.res;
    const BlobCache& bc = e->cache;
    const bool cached = bc.count > 0;
    const uint64_t nslots = cache_slots_for(64, uint64_t(e->pipe.hand_cap_blobs));
    const Events& ev = e->hand.ev;
    HIPCHK(hipEventRecord(ev[5 * size_t(p)], s));
    HIPCHK(blob_table_fill(e->out.p, e->out_off.p + lo, b.first.p + lo, hi - lo, b.boff.p, b.blen.p, s));
    HIPCHK(git_blob_ids_launch(e->out.p, b.boff.p + b0, b.blen.p + b0, b1 - b0, b.ids.p + size_t(b0) * 5, s));
    HIPCHK(hipEventRecord(ev[5 * size_t(p) + 1], s));
    HIPCHK(novel_range_launch(b.ids.p, b.blen.p, b0, b1, cached ? bc.ids.p : nullptr, cached ? bc.slots.p : nullptr,
                              cached ? uint32_t(bc.nslots - 1) : 0, v.slots.p, uint32_t(nslots - 1), v.where.p,
                              v.state.p, v.rep.p, c.flags.p, c.off.p, s));
    HIPCHK(delta_scan_range_launch(c.flags.p, b.boff.p, b0, b1 - b0, c.off.p, c.rank.p, c.chg_off.p, c.chg_src.p,
                                   c.tot.p, e->hand.words.dev + 4 * size_t(p) + 2, s));
    HIPCHK(hipEventRecord(ev[5 * size_t(p) + 2], s));
    HIPCHK(hipEventRecord(e->hand.scan_ev[p], s));
    return 0;
}

int mtr::handover_gather_pass(mtr_engine* e, uint32_t p, uint32_t j0, uint32_t j1, uint64_t o0, uint64_t o1,
                              hipStream_t s) {
    Compacted& c = e->novel.res;
    HIPCHK(hipEventRecord(e->hand.ev[5 * size_t(p) + 3], s));
    HIPCHK(delta_gather_range_launch(e->out.p, c.chg_off.p, c.chg_src.p, j0, j1, o0, o1, c.compact.p, s));
    HIPCHK(hipEventRecord(e->hand.ev[5 * size_t(p) + 4], s));
    return 0;
}

void mtr::handover_commit(mtr_engine* e, uint32_t nb) {
    e->ids.count = nb;
    e->summary_delta.valid = false;
    e->novel.res.valid = true;
}

// the per-blob tables of the whole summary after a hand-over run (the state-1 bytes went over part by part)
int mtr::handover_tables(mtr_engine* e, uint8_t* ids, uint8_t* state, int64_t* rep, int64_t* blob_off, int64_t* doc_first) {
    const uint32_t n = e->n_docs;
    DeltaRange r;
    if (compacted_range(e, e->novel.res, 0, n, r)) return -1;
    std::vector<uint32_t> rep32(size_t(r.count));
    if (r.count) {
        HIPCHK(hipMemcpy(rep32.data(), e->novel.rep.p, size_t(r.count) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ids, e->ids.ids.p, size_t(r.count) * MTR_BLOB_ID_BYTES, hipMemcpyDeviceToHost));
    }
    if (compacted_copy_out(e->novel.res, r, nullptr, e->novel.state.p, state, blob_off, doc_first)) return -1;
    for (int64_t k = 0; k < r.count; k++) rep[k] = rep32[size_t(k)] == kNoSlot ? -1 : int64_t(rep32[size_t(k)]);
    return 0;
}
