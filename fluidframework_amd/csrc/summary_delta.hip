// summary_delta.hip -- the incremental summary hand-over on the device (mtr_summary_delta).
//
// A host that keeps the git blob ids of the summary it uploaded last (the baseline) needs only the blobs whose id at
// the same (document, blob index) is new or different.  Three kernels on the engine stream:
//   delta_flag_kernel    one lane per blob: compare its id with the baseline's, emit a flag and a "changed length"
//   delta_scan_kernel    64-bit exclusive scan of the changed lengths (a summary can exceed 4 GiB) and the changed
//                        blobs compacted into (destination offset, source offset) pairs
//   delta_gather_kernel  the hot path: copies the changed blobs back to back into one compact buffer, partitioned by
//                        destination bytes, so one device-to-host copy brings them over
#include "summary_delta.hip.h"

namespace mtr {

namespace {

__global__ void __launch_bounds__(256)
delta_flag_kernel(const uint32_t* __restrict__ first, uint32_t n_docs, const uint32_t* __restrict__ blen,
                  const uint32_t* __restrict__ ids, uint32_t n_blobs, const uint32_t* __restrict__ base_first,
                  const uint32_t* __restrict__ base_ids, uint32_t base_docs, uint8_t* __restrict__ flags,
                  uint64_t* __restrict__ clen) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blobs) return;
    // the blob's document: the largest d in [0, n_docs) with first[d] <= b (documents without blobs repeat an entry)
    uint32_t lo = 0, hi = n_docs;
    while (hi - lo > 1) {
        const uint32_t m = lo + (hi - lo) / 2;
        if (first[m] <= b) lo = m;
        else hi = m;
    }
    const uint32_t k = b - first[lo];
    bool changed = true;
    if (lo < base_docs) {
        const uint32_t f = base_first[lo], cnt = base_first[lo + 1] - f;
        if (k < cnt) {
            const uint32_t* x = ids + 5 * size_t(b);
            const uint32_t* y = base_ids + 5 * (size_t(f) + k);
            uint32_t diff = 0;
#pragma unroll
            for (int j = 0; j < 5; j++) diff |= x[j] ^ y[j];
            changed = diff != 0;
        }
    }
    flags[b] = changed ? 1 : 0;
    clen[b] = changed ? uint64_t(blen[b]) : 0;
}

// blob_scan_kernel's scheme (one workgroup, a contiguous chunk per thread) over 64-bit lengths, carrying the count
// of changed blobs along: the second pass writes each blob's offset and appends the changed ones to the compact list
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads)
delta_scan_kernel(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ boff, uint32_t n,
                  uint64_t* __restrict__ clen, uint32_t* __restrict__ rank, uint64_t* __restrict__ chg_off,
                  uint64_t* __restrict__ chg_src, uint64_t* __restrict__ tot) {
    __shared__ uint64_t part[kScanThreads];
    __shared__ uint32_t cpart[kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = uint32_t(min(uint64_t(n), uint64_t(t) * chunk)), hi = uint32_t(min(uint64_t(n), uint64_t(lo) + chunk));
    uint64_t sum = 0;
    uint32_t cnt = 0;
    for (uint32_t i = lo; i < hi; i++) {
        sum += clen[i];
        cnt += flags[i];
    }
    part[t] = sum;
    cpart[t] = cnt;
    __syncthreads();
    for (uint32_t step = 1; step < kScanThreads; step <<= 1) {
        const uint64_t v = t >= step ? part[t - step] : 0;
        const uint32_t c = t >= step ? cpart[t - step] : 0;
        __syncthreads();
        part[t] += v;
        cpart[t] += c;
        __syncthreads();
    }
    uint64_t run = part[t] - sum;
    uint32_t j = cpart[t] - cnt;
    for (uint32_t i = lo; i < hi; i++) {
        const uint64_t c = clen[i];
        clen[i] = run;
        rank[i] = j;
        if (flags[i]) {
            chg_off[j] = run;
            chg_src[j] = boff[i];
            j++;
        }
        run += c;
    }
    if (t == kScanThreads - 1) {
        clen[n] = part[t];
        rank[n] = cpart[t];
        chg_off[cpart[t]] = part[t];
        tot[0] = cpart[t];
        tot[1] = part[t];
    }
}

// the largest j in [lo, n) with off[j] <= p, given off[lo] <= p < off[n]: a gallop from lo (the answer is usually lo
// or close to it: a lane's next 16 bytes, or a workgroup's next tile), then a bisection of the bracket
__device__ __forceinline__ uint32_t find_blob(const uint64_t* __restrict__ off, uint32_t lo, uint32_t n, uint64_t p) {
    uint32_t a = lo, step = 1;
    while (step < n - a && off[a + step] <= p) {
        a += step;
        step <<= 1;
    }
    uint32_t b = step < n - a ? a + step : n;  // off[b] > p
    while (b - a > 1) {
        const uint32_t m = a + (b - a) / 2;
        if (off[m] <= p) a = m;
        else b = m;
    }
    return a;
}

// delta_scan_kernel over the blobs [b0, b0 + n) of a summary that is scanned range by range (the pipelined hand-over):
// the chosen blobs and their bytes of the ranges before come in through tot (zeroed before the first range) and the new
// sums go out through it, so every offset, rank and compact-list entry is summary-wide and after the last range the
// arrays are what delta_scan_kernel over all blobs leaves.  Every thread reads tot before the first barrier, the last
// one writes it after the last.  host (mapped memory, 2 words) receives the two sums.
__global__ void __launch_bounds__(kScanThreads)
delta_scan_range_kernel(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ boff, uint32_t b0, uint32_t n,
                        uint64_t* __restrict__ clen, uint32_t* __restrict__ rank, uint64_t* __restrict__ chg_off,
                        uint64_t* __restrict__ chg_src, uint64_t* tot, int64_t* __restrict__ host) {
    __shared__ uint64_t part[kScanThreads];
    __shared__ uint32_t cpart[kScanThreads];
    const uint32_t j0 = uint32_t(tot[0]);
    const uint64_t o0 = tot[1];
    flags += b0;
    boff += b0;
    clen += b0;
    rank += b0;
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = uint32_t(min(uint64_t(n), uint64_t(t) * chunk)), hi = uint32_t(min(uint64_t(n), uint64_t(lo) + chunk));
    uint64_t sum = 0;
    uint32_t cnt = 0;
    for (uint32_t i = lo; i < hi; i++) {
        sum += clen[i];
        cnt += flags[i];
    }
    part[t] = sum;
    cpart[t] = cnt;
    __syncthreads();
    for (uint32_t step = 1; step < kScanThreads; step <<= 1) {
        const uint64_t v = t >= step ? part[t - step] : 0;
        const uint32_t c = t >= step ? cpart[t - step] : 0;
        __syncthreads();
        part[t] += v;
        cpart[t] += c;
        __syncthreads();
    }
    uint64_t run = o0 + part[t] - sum;
    uint32_t j = j0 + cpart[t] - cnt;
    for (uint32_t i = lo; i < hi; i++) {
        const uint64_t c = clen[i];
        clen[i] = run;
        rank[i] = j;
        if (flags[i]) {
            chg_off[j] = run;
            chg_src[j] = boff[i];
            j++;
        }
        run += c;
    }
    if (t == kScanThreads - 1) {
        const uint64_t bytes = o0 + part[t];
        const uint32_t chosen = j0 + cpart[t];
        clen[n] = bytes;
        rank[n] = chosen;
        chg_off[chosen] = bytes;
        tot[0] = chosen;
        tot[1] = bytes;
        host[0] = int64_t(chosen);
        host[1] = int64_t(bytes);
        __threadfence_system();
    }
}

// The 16 destination bytes [p, p + 16) of the compact buffer, as the gather kernels store them: j is the chosen blob
// that holds byte p (find_blob), `total` the end of the bytes being gathered (bytes from there on are zero).
__device__ __forceinline__ uint4 gather16(const uint8_t* __restrict__ src, const uint64_t* __restrict__ chg_off,
                                          const uint64_t* __restrict__ chg_src, uint32_t j, uint64_t p,
                                          uint64_t total) {
    const uint64_t end = chg_off[j + 1];
    uint64_t s = chg_src[j] + (p - chg_off[j]);  // source offset of destination byte p
    // (named scalars, not arrays: a private array here is promoted to LDS before the loops are unrolled)
    uint4 r;
    if (p + 16 <= end) {
        const uint4* a = reinterpret_cast<const uint4*>(src + (s & ~uint64_t(15)));
        const uint32_t sh = uint32_t(s) & 15u;
        const uint4 lo4 = a[0];
        const uint4 hi4 = sh ? a[1] : lo4;
        const bool s8 = sh & 8u, s4 = sh & 4u;
        // words [2, 8) of the pair when the shift has 8, then one word more when it has 4
        const uint32_t u0 = s8 ? lo4.z : lo4.x, u1 = s8 ? lo4.w : lo4.y, u2 = s8 ? hi4.x : lo4.z,
                       u3 = s8 ? hi4.y : lo4.w, u4 = s8 ? hi4.z : hi4.x, u5 = s8 ? hi4.w : hi4.y;
        const uint32_t v0 = s4 ? u1 : u0, v1 = s4 ? u2 : u1, v2 = s4 ? u3 : u2, v3 = s4 ? u4 : u3,
                       v4 = s4 ? u5 : u4;
        r.x = __builtin_amdgcn_alignbyte(v1, v0, sh & 3u);
        r.y = __builtin_amdgcn_alignbyte(v2, v1, sh & 3u);
        r.z = __builtin_amdgcn_alignbyte(v3, v2, sh & 3u);
        r.w = __builtin_amdgcn_alignbyte(v4, v3, sh & 3u);
    } else {
        uint32_t jj = j;
        uint64_t e = end;
        // the little-endian word of destination bytes [pq, pq + 4): blob bytes below `total`, zero from there on
        auto word = [&](uint64_t pq) {
            uint32_t v = 0;
#pragma unroll
            for (int q = 0; q < 4; q++, pq++) {
                if (pq < total) {
                    while (pq >= e) {  // (ends at the last blob at the latest: chg_off[changed] = total > pq)
                        jj++;
                        s = chg_src[jj];
                        e = chg_off[jj + 1];
                    }
                    v |= uint32_t(src[s]) << (8 * q);
                    s++;
                }
            }
            return v;
        };
        r.x = word(p);
        r.y = word(p + 4);
        r.z = word(p + 8);
        r.w = word(p + 12);
    }
    return r;
}

}  // namespace

// The compact buffer is cut into tiles of kTileBytes; a workgroup owns a run of consecutive tiles (one tile while the
// grid is small; more than one only when the tiles outnumber kMaxGroups workgroups, so that the search for the run's
// first blob is paid once per run).  Work is partitioned by destination bytes, never by blob: a 1 MB blob is spread
// over many workgroups, thousands of 200-byte blobs share one, and no wave waits on a longest blob.
//
// Each lane owns 16 destination bytes at a time (a 16-byte aligned 16-byte store; consecutive lanes, consecutive
// stores) and finds the changed blob that holds their first byte by a gallop from the blob of its previous 16 bytes.
//   - 16 bytes inside one blob: the source has any byte alignment, so the lane loads the 16-byte aligned words that
//     hold them (one when the source is aligned too, else two) and funnel-shifts the pair by (source address & 15):
//     a dword select by (address & 12), then v_alignbyte by (address & 3), as git_blob_id_kernel does.
//   - 16 bytes that span a blob boundary, or the end of the buffer: assembled bytewise, walking forward through the
//     blobs (empty ones included); bytes past the total stay zero.
// Reads: the bytewise path reads blob bytes only.  The aligned path reads [a, a + 16) with a = source & ~15, and
// [a + 16, a + 32) only when the source is misaligned; both hold at least one byte of the blob.  a is never below
// src because src is an allocation start (16-byte aligned); a + 32 can pass the last blob's end by up to 15 bytes,
// which relies on the 16 bytes of slack the engine allocates after the summary buffer (out.ensure(total + 16)).
// Writes: the last store may run up to 15 bytes past `total`; dst holds total + 16 bytes.
constexpr int kGatherThreads = 256;
constexpr uint32_t kTileBytes = 16384;
constexpr uint32_t kMaxGroups = 2048;  // 256 CUs x 8 workgroups of 4 waves
__global__ void __launch_bounds__(kGatherThreads)
delta_gather_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ chg_off,
                    const uint64_t* __restrict__ chg_src, uint32_t changed, uint64_t total, uint32_t tiles_per_group,
                    uint8_t* __restrict__ dst) {
    const uint64_t span = uint64_t(tiles_per_group) * kTileBytes;
    const uint64_t x0 = uint64_t(blockIdx.x) * span;
    if (x0 >= total) return;
    const uint64_t x1 = min(total, x0 + span);
    uint32_t j = find_blob(chg_off, 0, changed, x0);  // (the same in every lane)
    for (uint64_t p = x0 + 16 * threadIdx.x; p < x1; p += 16 * kGatherThreads) {
        j = find_blob(chg_off, j, changed, p);
        const uint4 r = gather16(src, chg_off, chg_src, j, p, total);
        *reinterpret_cast<uint4*>(dst + p) = r;
    }
}

// delta_gather_kernel over the destination bytes [o0, o1) alone: the chosen blobs [j0, j1) of one range of a summary
// that is gathered range by range (chg_off[j0] = o0, chg_off[j1] = o1; o0 < o1).  A range starts where the one before
// ended, at any byte, and the 16-byte stores need 16-byte aligned addresses: the tiles are cut from the 16-byte boundary
// at or below o0, and the lane whose 16 bytes begin below o0 stores its bytes from o0 on one by one -- the bytes
// below o0 in that block are the earlier range's gathered bytes, which this range's blob list does not describe: a
// 16-byte store there would overwrite them.  The last store writes zeros up to 15 bytes past o1, as
// delta_gather_kernel does past `total`; the next range's first bytes land there afterwards.  Both need the ranges'
// gathers, and the copies of their bytes, in range order on one stream.  dst holds 16 bytes past the last range's
// end.
__global__ void __launch_bounds__(kGatherThreads)
delta_gather_range_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ chg_off,
                          const uint64_t* __restrict__ chg_src, uint32_t j0, uint32_t j1, uint64_t o0, uint64_t o1,
                          uint32_t tiles_per_group, uint8_t* __restrict__ dst) {
    const uint64_t span = uint64_t(tiles_per_group) * kTileBytes;
    const uint64_t x0 = (o0 & ~uint64_t(15)) + uint64_t(blockIdx.x) * span;
    if (x0 >= o1) return;
    const uint64_t x1 = min(o1, x0 + span);
    const uint64_t* __restrict__ co = chg_off + j0;  // (offsets stay summary-wide; the indices are the range's)
    const uint64_t* __restrict__ cs = chg_src + j0;
    const uint32_t changed = j1 - j0;
    uint32_t j = find_blob(co, 0, changed, max(x0, o0));  // (the same in every lane)
    for (uint64_t p = x0 + 16 * threadIdx.x; p < x1; p += 16 * kGatherThreads) {
        if (p < o0) {  // (one lane of the range at most)
            uint32_t jj = 0;
            uint64_t s = cs[0], e = co[1];
            const uint64_t stop = min(p + 16, o1);
            for (uint64_t q = o0; q < stop; q++) {
                while (q >= e) {  // (ends at the range's last blob at the latest: co[changed] = o1 > q)
                    jj++;
                    s = cs[jj];
                    e = co[jj + 1];
                }
                dst[q] = src[s];
                s++;
            }
            continue;
        }
        j = find_blob(co, j, changed, p);
        const uint4 r = gather16(src, co, cs, j, p, o1);
        *reinterpret_cast<uint4*>(dst + p) = r;
    }
}

hipError_t delta_flag_launch(const uint32_t* first, uint32_t n_docs, const uint32_t* blen, const uint32_t* ids,
                             uint32_t n_blobs, const uint32_t* base_first, const uint32_t* base_ids,
                             uint32_t base_docs, uint8_t* flags, uint64_t* clen, hipStream_t s) {
    if (n_blobs)
        delta_flag_kernel<<<(n_blobs + 255) / 256, 256, 0, s>>>(first, n_docs, blen, ids, n_blobs, base_first, base_ids,
                                                                 base_docs, flags, clen);
    return hipGetLastError();
}

hipError_t delta_scan_launch(const uint8_t* flags, const uint64_t* boff, uint32_t n_blobs, uint64_t* clen,
                             uint32_t* rank, uint64_t* chg_off, uint64_t* chg_src, uint64_t* tot, hipStream_t s) {
    delta_scan_kernel<<<1, kScanThreads, 0, s>>>(flags, boff, n_blobs, clen, rank, chg_off, chg_src, tot);
    return hipGetLastError();
}

hipError_t delta_gather_launch(const uint8_t* src, const uint64_t* chg_off, const uint64_t* chg_src, uint32_t changed,
                               uint64_t total, uint8_t* dst, hipStream_t s) {
    if (changed == 0 || total == 0) return hipSuccess;
    const uint64_t tiles = (total + kTileBytes - 1) / kTileBytes;
    const uint64_t per = (tiles + kMaxGroups - 1) / kMaxGroups;
    const uint64_t groups = (tiles + per - 1) / per;
    delta_gather_kernel<<<uint32_t(groups), kGatherThreads, 0, s>>>(src, chg_off, chg_src, changed, total,
                                                                     uint32_t(per), dst);
    return hipGetLastError();
}

hipError_t delta_scan_range_launch(const uint8_t* flags, const uint64_t* boff, uint32_t b0, uint32_t n, uint64_t* clen,
                                   uint32_t* rank, uint64_t* chg_off, uint64_t* chg_src, uint64_t* tot, int64_t* host,
                                   hipStream_t s) {
    delta_scan_range_kernel<<<1, kScanThreads, 0, s>>>(flags, boff, b0, n, clen, rank, chg_off, chg_src, tot, host);
    return hipGetLastError();
}

hipError_t delta_gather_range_launch(const uint8_t* src, const uint64_t* chg_off, const uint64_t* chg_src, uint32_t j0,
                                     uint32_t j1, uint64_t o0, uint64_t o1, uint8_t* dst, hipStream_t s) {
    if (j1 <= j0 || o1 <= o0) return hipSuccess;
    const uint64_t tiles = (o1 - (o0 & ~uint64_t(15)) + kTileBytes - 1) / kTileBytes;
    const uint64_t per = (tiles + kMaxGroups - 1) / kMaxGroups;
    const uint64_t groups = (tiles + per - 1) / per;
    delta_gather_range_kernel<<<uint32_t(groups), kGatherThreads, 0, s>>>(src, chg_off, chg_src, j0, j1, o0, o1,
                                                                           uint32_t(per), dst);
    return hipGetLastError();
}

}  // namespace mtr
