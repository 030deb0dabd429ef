// blob_cache.hip -- the device blob-id cache and the novel pass (mtr_blob_cache_* / mtr_summary_novel).
//
// Storage's upload decision is set membership of a blob's git id (SummaryTreeUploadManager.writeSummaryBlob against
// blobsShaCache), so the engine keeps such a set on the device, next to the ids it hashes there:
//   cache_insert_kernel   one lane per id: probe from a hash of the id, claim an empty slot with a 32-bit atomicCAS,
//                         compare all five words against the occupant of a used one, next slot when they differ
//   cache_rank_kernel     which source ids were new, scanned: new entries are appended in the order of their smallest
//                         source index, so two engines fed the same calls hold the same table
//   cache_commit_kernel   appends them and points their slots at the final entries
//   cache_has_kernel      probe only
//   novel_classify_kernel one lane per summary blob: probe the cache; a miss is inserted into the summary's own set
//   novel_state_kernel    after it: a slot holds the smallest blob index with its id, which gives state and rep
// The compaction and the gather of the state-1 blobs are summary_delta.hip's kernels on these flags and lengths.
// The life cycle (mtr_blob_cache_trim / _trim_to / _ages / _export / _import), further down:
//   cache_stamp_kernel    one lane per offered id, after the commit: probe, atomicMax on the entry's stamp
//   cache_age_hist_kernel grid-stride over the stamps, an LDS histogram a workgroup, 64-bit atomics for its buckets
//   cache_count_kernel    the entries a cutoff keeps (trim_to's search beyond the histogram's reach)
//   cache_keep_kernel, cache_keep_scan_kernel, cache_compact_kernel
//                         a trim: flags, their scan (one workgroup, as cache_rank_kernel), the survivors into a fresh
//                         table; cache_insert_kernel then fills a fresh slot array from that table
//
// No lane waits on another: a slot holds an index, never an id in the making, and every id a slot can name (the
// table's entries and the kernel's source ids) was written by an earlier operation on the stream.  A lane that loses a
// CAS reads the winner's index from the CAS itself and compares against memory that is already complete.  Equality is
// always all 160 bits: a SHA-1 prefix collision can be constructed, and a false "held" would lose a blob.
// Every probe loop is bounded by the slot count; at most half the slots are used, so it ends at an empty slot or at
// the id long before.
#include "blob_cache.hip.h"

#include <algorithm>

namespace mtr {

namespace {

__device__ __forceinline__ uint32_t id_hash(uint32_t a0, uint32_t a1) { return a0 ^ (a1 * 0x9E3779B1u); }

__device__ __forceinline__ bool same_id(const uint32_t* __restrict__ t, uint32_t a0, uint32_t a1, uint32_t a2,
                                        uint32_t a3, uint32_t a4) {
    return ((t[0] ^ a0) | (t[1] ^ a1) | (t[2] ^ a2) | (t[3] ^ a3) | (t[4] ^ a4)) == 0;
}

// does the set hold the id (nothing writes the set meanwhile)
__device__ __forceinline__ bool set_find(const uint32_t* __restrict__ table, const uint32_t* __restrict__ slots,
                                         uint32_t mask, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3,
                                         uint32_t a4) {
    uint32_t s = id_hash(a0, a1) & mask;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint32_t v = slots[s];
        if (v == 0) return false;
        if (same_id(table + 5 * size_t(v - 1), a0, a1, a2, a3, a4)) return true;
    }
    return false;
}

// offers the id as entry `mine - 1`; returns the slot that holds the id's entry (kNoSlot: no slot left, which a set
// kept at most half full never reaches).  Entry j is table[5 j ..] below `held`, src[5 (j - held) ..] from there on.
__device__ __forceinline__ uint32_t set_insert(const uint32_t* __restrict__ table, uint32_t held,
                                               const uint32_t* __restrict__ src, uint32_t* slots, uint32_t mask,
                                               uint32_t mine, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3,
                                               uint32_t a4) {
    uint32_t s = id_hash(a0, a1) & mask;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint32_t v = atomicCAS(&slots[s], 0u, mine);
        if (v == 0) return s;  // claimed
        const uint32_t j = v - 1;
        const uint32_t* t = j < held ? table + 5 * size_t(j) : src + 5 * size_t(j - held);
        if (same_id(t, a0, a1, a2, a3, a4)) {
            // a repeat: of an entry the set held before (left alone), or of another source id -- the slot keeps the
            // smaller index of the two, whichever lane won the CAS (the occupant's id stays what it is)
            if (j >= held && v > mine) atomicMin(&slots[s], mine);
            return s;
        }
    }
    return kNoSlot;
}

__global__ void __launch_bounds__(256)
cache_insert_kernel(const uint32_t* __restrict__ table, uint32_t held, const uint32_t* __restrict__ src, uint32_t n,
                    uint32_t* slots, uint32_t mask, uint32_t* __restrict__ where) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* x = src + 5 * size_t(i);
    const uint32_t w = set_insert(table, held, src, slots, mask, held + i + 1, x[0], x[1], x[2], x[3], x[4]);
    if (where) where[i] = w;
}

// delta_scan_kernel's scheme (one workgroup, a contiguous chunk per thread) over the "new" flags alone
constexpr int kRankThreads = 1024;
__global__ void __launch_bounds__(kRankThreads)
cache_rank_kernel(const uint32_t* __restrict__ slots, const uint32_t* __restrict__ where, uint32_t held, uint32_t n,
                  uint8_t* __restrict__ isnew, uint32_t* __restrict__ rank, uint32_t* __restrict__ tot) {
    __shared__ uint32_t part[kRankThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + kRankThreads - 1) / kRankThreads;
    const uint32_t lo = uint32_t(min(uint64_t(n), uint64_t(t) * chunk)), hi = uint32_t(min(uint64_t(n), uint64_t(lo) + chunk));
    uint32_t cnt = 0;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t w = where[i];
        const uint8_t f = w != kNoSlot && slots[w] == held + i + 1;
        isnew[i] = f;
        cnt += f;
    }
    part[t] = cnt;
    __syncthreads();
    for (uint32_t step = 1; step < kRankThreads; step <<= 1) {
        const uint32_t c = t >= step ? part[t - step] : 0;
        __syncthreads();
        part[t] += c;
        __syncthreads();
    }
    uint32_t j = part[t] - cnt;
    for (uint32_t i = lo; i < hi; i++) {
        rank[i] = j;
        j += isnew[i];
    }
    if (t == kRankThreads - 1) {
        rank[n] = part[t];
        tot[0] = part[t];
    }
}

__global__ void __launch_bounds__(256)
cache_commit_kernel(const uint32_t* __restrict__ src, const uint8_t* __restrict__ isnew,
                    const uint32_t* __restrict__ rank, const uint32_t* __restrict__ where, uint32_t held, uint32_t n,
                    uint32_t* __restrict__ table, uint32_t* __restrict__ slots) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !isnew[i]) return;
    const uint32_t fin = held + rank[i];
    const uint32_t* x = src + 5 * size_t(i);
    uint32_t* y = table + 5 * size_t(fin);
#pragma unroll
    for (int j = 0; j < 5; j++) y[j] = x[j];
    slots[where[i]] = fin + 1;  // (one new id, one slot, one lane)
}

__global__ void __launch_bounds__(256)
cache_has_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ slots, uint32_t mask,
                 const uint32_t* __restrict__ q, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* x = q + 5 * size_t(i);
    out[i] = set_find(table, slots, mask, x[0], x[1], x[2], x[3], x[4]) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
novel_classify_kernel(const uint32_t* __restrict__ ids, uint32_t n_blobs, const uint32_t* __restrict__ table,
                      const uint32_t* __restrict__ cslots, uint32_t cmask, uint32_t* slots, uint32_t mask,
                      uint32_t* __restrict__ where) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blobs) return;
    const uint32_t* x = ids + 5 * size_t(b);
    const uint32_t a0 = x[0], a1 = x[1], a2 = x[2], a3 = x[3], a4 = x[4];
    if (cslots && set_find(table, cslots, cmask, a0, a1, a2, a3, a4)) {
        where[b] = kNoSlot;
        return;
    }
    where[b] = set_insert(nullptr, 0, ids, slots, mask, b + 1, a0, a1, a2, a3, a4);
}

__global__ void __launch_bounds__(256)
novel_state_kernel(const uint32_t* __restrict__ slots, const uint32_t* __restrict__ where,
                   const uint32_t* __restrict__ blen, uint32_t n_blobs, uint8_t* __restrict__ state,
                   uint32_t* __restrict__ rep, uint8_t* __restrict__ flags, uint64_t* __restrict__ clen) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blobs) return;
    const uint32_t w = where[b];
    const uint32_t r = w == kNoSlot ? kNoSlot : slots[w] - 1;
    const bool first = r == b;
    state[b] = w == kNoSlot ? 0 : (first ? 1 : 2);
    rep[b] = r;
    flags[b] = first ? 1 : 0;
    clen[b] = first ? uint64_t(blen[b]) : 0;
}

// The two kernels over the blobs [b0, b1) of a summary whose blobs below b0 went through them before (the pipelined
// hand-over's ranges): indices stay summary-wide, the summary's own set is kept from range to range.  Every index a
// slot can hold from an earlier range is below b0, so the atomic-min never lets a blob of this range replace one: when
// the classify kernel of a range has ended, the slots its blobs sit in are final, and so are their states and reps.
// That needs the ranges' kernels in blob order, one after the other: the caller puts them all on one stream.
__global__ void __launch_bounds__(256)
novel_classify_range_kernel(const uint32_t* __restrict__ ids, uint32_t b0, uint32_t b1,
                            const uint32_t* __restrict__ table, const uint32_t* __restrict__ cslots, uint32_t cmask,
                            uint32_t* slots, uint32_t mask, uint32_t* __restrict__ where) {
    const uint32_t b = b0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= b1) return;
    const uint32_t* x = ids + 5 * size_t(b);
    const uint32_t a0 = x[0], a1 = x[1], a2 = x[2], a3 = x[3], a4 = x[4];
    if (cslots && set_find(table, cslots, cmask, a0, a1, a2, a3, a4)) {
        where[b] = kNoSlot;
        return;
    }
    where[b] = set_insert(nullptr, 0, ids, slots, mask, b + 1, a0, a1, a2, a3, a4);
}

__global__ void __launch_bounds__(256)
novel_state_range_kernel(const uint32_t* __restrict__ slots, const uint32_t* __restrict__ where,
                         const uint32_t* __restrict__ blen, uint32_t b0, uint32_t b1, uint8_t* __restrict__ state,
                         uint32_t* __restrict__ rep, uint8_t* __restrict__ flags, uint64_t* __restrict__ clen) {
    const uint32_t b = b0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= b1) return;
    const uint32_t w = where[b];
    const uint32_t r = w == kNoSlot ? kNoSlot : slots[w] - 1;
    const bool first = r == b;
    state[b] = w == kNoSlot ? 0 : (first ? 1 : 2);
    rep[b] = r;
    flags[b] = first ? 1 : 0;
    clen[b] = first ? uint64_t(blen[b]) : 0;
}

// ---- the cache's life cycle: a stamp per entry (the generation that last offered the id), the age histogram, and
// the trim.  An entry is never taken out of a probe chain: a chain with a hole loses every id that was pushed past the
// hole, a tombstone would need a lane to tell a dead entry from one in the making, and a slot only ever names a
// finished entry.  So a trim copies the survivors to a fresh table in table order and fills a fresh, zeroed slot
// array from it with cache_insert_kernel, the step a grow uses.

// the entry (index + 1) that holds the id, 0 = none (nothing writes the set meanwhile)
__device__ __forceinline__ uint32_t set_entry(const uint32_t* __restrict__ table, const uint32_t* __restrict__ slots,
                                              uint32_t mask, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3,
                                              uint32_t a4) {
    uint32_t s = id_hash(a0, a1) & mask;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint32_t v = slots[s];
        if (v == 0) return 0;
        if (same_id(table + 5 * size_t(v - 1), a0, a1, a2, a3, a4)) return v;
    }
    return 0;
}

// after an add's commit: every offered id is an entry now; equal ids of one call meet in the atomicMax
__global__ void __launch_bounds__(256)
cache_stamp_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ slots, uint32_t mask,
                   const uint32_t* __restrict__ q, const uint32_t* __restrict__ age, uint32_t gen, uint32_t n,
                   uint32_t* stamp) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* x = q + 5 * size_t(i);
    const uint32_t v = set_entry(table, slots, mask, x[0], x[1], x[2], x[3], x[4]);
    if (v) atomicMax(&stamp[v - 1], age ? gen - age[i] : gen);
}

constexpr uint32_t kAgeBuckets = 1024;
__global__ void __launch_bounds__(256)
cache_age_hist_kernel(const uint32_t* __restrict__ stamp, uint32_t count, uint32_t gen, uint32_t n,
                      unsigned long long* out) {
    __shared__ uint32_t h[kAgeBuckets];
    for (uint32_t b = threadIdx.x; b < n; b += blockDim.x) h[b] = 0;
    __syncthreads();
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride)
        atomicAdd(&h[min(gen - stamp[i], n - 1)], 1u);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < n; b += blockDim.x)
        if (h[b]) atomicAdd(&out[b], (unsigned long long)h[b]);
}

// out[0] += the entries with stamp >= cutoff
__global__ void __launch_bounds__(256)
cache_count_kernel(const uint32_t* __restrict__ stamp, uint32_t count, uint64_t cutoff, unsigned long long* out) {
    __shared__ uint32_t part;
    if (threadIdx.x == 0) part = 0;
    __syncthreads();
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    uint32_t c = 0;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) c += stamp[i] >= cutoff;
    if (c) atomicAdd(&part, c);
    __syncthreads();
    if (threadIdx.x == 0 && part) atomicAdd(out, (unsigned long long)part);
}

__global__ void __launch_bounds__(256)
cache_keep_kernel(const uint32_t* __restrict__ stamp, uint32_t count, uint64_t cutoff, uint8_t* __restrict__ keep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) keep[i] = stamp[i] >= cutoff;
}

// cache_rank_kernel's scheme over the keep flags: idx[i] = the survivors before entry i, idx[n] and tot[0] = all
__global__ void __launch_bounds__(kRankThreads)
cache_keep_scan_kernel(const uint8_t* __restrict__ keep, uint32_t n, uint32_t* __restrict__ idx,
                       uint32_t* __restrict__ tot) {
    __shared__ uint32_t part[kRankThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + kRankThreads - 1) / kRankThreads;
    const uint32_t lo = uint32_t(min(uint64_t(n), uint64_t(t) * chunk)), hi = uint32_t(min(uint64_t(n), uint64_t(lo) + chunk));
    uint32_t cnt = 0;
    for (uint32_t i = lo; i < hi; i++) cnt += keep[i];
    part[t] = cnt;
    __syncthreads();
    for (uint32_t step = 1; step < kRankThreads; step <<= 1) {
        const uint32_t c = t >= step ? part[t - step] : 0;
        __syncthreads();
        part[t] += c;
        __syncthreads();
    }
    uint32_t j = part[t] - cnt;
    for (uint32_t i = lo; i < hi; i++) {
        idx[i] = j;
        j += keep[i];
    }
    if (t == kRankThreads - 1) {
        idx[n] = part[t];
        tot[0] = part[t];
    }
}

__global__ void __launch_bounds__(256)
cache_compact_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ stamp,
                     const uint8_t* __restrict__ keep, const uint32_t* __restrict__ idx, uint32_t count,
                     uint32_t* __restrict__ ntable, uint32_t* __restrict__ nstamp) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count || !keep[i]) return;
    const uint32_t j = idx[i];
    const uint32_t* x = table + 5 * size_t(i);
    uint32_t* y = ntable + 5 * size_t(j);
#pragma unroll
    for (int k = 0; k < 5; k++) y[k] = x[k];
    nstamp[j] = stamp[i];
}

inline uint32_t groups_of(uint32_t n) { return (n + 255) / 256; }
inline uint32_t stride_groups(uint32_t n) { return std::min<uint32_t>(groups_of(n), 1024); }

}  // namespace

hipError_t cache_stamp_launch(const uint32_t* table, const uint32_t* slots, uint32_t mask, const uint32_t* q,
                              const uint32_t* age, uint32_t gen, uint32_t n, uint32_t* stamp, hipStream_t s) {
    if (n) cache_stamp_kernel<<<groups_of(n), 256, 0, s>>>(table, slots, mask, q, age, gen, n, stamp);
    return hipGetLastError();
}

hipError_t cache_age_hist_launch(const uint32_t* stamp, uint32_t count, uint32_t gen, uint32_t n,
                                 unsigned long long* out, hipStream_t s) {
    if (count) cache_age_hist_kernel<<<stride_groups(count), 256, 0, s>>>(stamp, count, gen, n, out);
    return hipGetLastError();
}

hipError_t cache_count_launch(const uint32_t* stamp, uint32_t count, uint64_t cutoff, unsigned long long* out,
                              hipStream_t s) {
    if (count) cache_count_kernel<<<stride_groups(count), 256, 0, s>>>(stamp, count, cutoff, out);
    return hipGetLastError();
}

hipError_t cache_keep_launch(const uint32_t* stamp, uint32_t count, uint64_t cutoff, uint8_t* keep, uint32_t* idx,
                             uint32_t* tot, hipStream_t s) {
    if (count) cache_keep_kernel<<<groups_of(count), 256, 0, s>>>(stamp, count, cutoff, keep);
    cache_keep_scan_kernel<<<1, kRankThreads, 0, s>>>(keep, count, idx, tot);
    return hipGetLastError();
}

hipError_t cache_compact_launch(const uint32_t* table, const uint32_t* stamp, const uint8_t* keep, const uint32_t* idx,
                                uint32_t count, uint32_t* ntable, uint32_t* nstamp, hipStream_t s) {
    if (count) cache_compact_kernel<<<groups_of(count), 256, 0, s>>>(table, stamp, keep, idx, count, ntable, nstamp);
    return hipGetLastError();
}

hipError_t cache_insert_launch(const uint32_t* table, uint32_t held, const uint32_t* src, uint32_t n, uint32_t* slots,
                               uint32_t mask, uint32_t* where, hipStream_t s) {
    if (n) cache_insert_kernel<<<groups_of(n), 256, 0, s>>>(table, held, src, n, slots, mask, where);
    return hipGetLastError();
}

hipError_t cache_rank_launch(const uint32_t* slots, const uint32_t* where, uint32_t held, uint32_t n, uint8_t* isnew,
                             uint32_t* rank, uint32_t* tot, hipStream_t s) {
    cache_rank_kernel<<<1, kRankThreads, 0, s>>>(slots, where, held, n, isnew, rank, tot);
    return hipGetLastError();
}

hipError_t cache_commit_launch(const uint32_t* src, const uint8_t* isnew, const uint32_t* rank, const uint32_t* where,
                               uint32_t held, uint32_t n, uint32_t* table, uint32_t* slots, hipStream_t s) {
    if (n) cache_commit_kernel<<<groups_of(n), 256, 0, s>>>(src, isnew, rank, where, held, n, table, slots);
    return hipGetLastError();
}

hipError_t cache_has_launch(const uint32_t* table, const uint32_t* slots, uint32_t mask, const uint32_t* q, uint32_t n,
                            uint8_t* out, hipStream_t s) {
    if (n) cache_has_kernel<<<groups_of(n), 256, 0, s>>>(table, slots, mask, q, n, out);
    return hipGetLastError();
}

hipError_t novel_classify_launch(const uint32_t* ids, uint32_t n_blobs, const uint32_t* table, const uint32_t* cslots,
                                 uint32_t cmask, uint32_t* slots, uint32_t mask, uint32_t* where, hipStream_t s) {
    if (n_blobs)
        novel_classify_kernel<<<groups_of(n_blobs), 256, 0, s>>>(ids, n_blobs, table, cslots, cmask, slots, mask, where);
    return hipGetLastError();
}

hipError_t novel_state_launch(const uint32_t* slots, const uint32_t* where, const uint32_t* blen, uint32_t n_blobs,
                              uint8_t* state, uint32_t* rep, uint8_t* flags, uint64_t* clen, hipStream_t s) {
    if (n_blobs) novel_state_kernel<<<groups_of(n_blobs), 256, 0, s>>>(slots, where, blen, n_blobs, state, rep, flags, clen);
    return hipGetLastError();
}

hipError_t novel_range_launch(const uint32_t* ids, const uint32_t* blen, uint32_t b0, uint32_t b1,
                              const uint32_t* table, const uint32_t* cslots, uint32_t cmask, uint32_t* slots,
                              uint32_t mask, uint32_t* where, uint8_t* state, uint32_t* rep, uint8_t* flags,
                              uint64_t* clen, hipStream_t s) {
    if (b1 <= b0) return hipSuccess;
    const uint32_t g = groups_of(b1 - b0);
    novel_classify_range_kernel<<<g, 256, 0, s>>>(ids, b0, b1, table, cslots, cmask, slots, mask, where);
    novel_state_range_kernel<<<g, 256, 0, s>>>(slots, where, blen, b0, b1, state, rep, flags, clen);
    return hipGetLastError();
}

}  // namespace mtr
