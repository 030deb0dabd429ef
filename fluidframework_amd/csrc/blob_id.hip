// blob_id.hip -- git blob ids of the summary blobs on the device (mtr_summary_blob_ids / mtr_git_blob_ids).
//
// A blob's id is SHA-1("blob " + decimal byte length + NUL + the bytes): what `git hash-object` prints and what
// gitHashFile (@fluidframework/common-utils) returns, the name Fluid's git storage knows the blob by.
//
// SHA-1 is a serial chain within one blob, so the parallelism is across blobs: one lane per blob, each lane
// streaming its own 64-byte blocks.  Lanes of a wave run different numbers of blocks; the block loop holds no
// cross-lane operation and no barrier, so the divergent trip count is safe.  The 80 rounds are fully unrolled: the
// 16-word schedule window is indexed statically and stays in VGPRs (no scratch; fluidframework_amd/build.py
// refuses a build of this kernel with any).  The per-lane hashing is git_object_id (git_object_id.hip.h), shared with
// the tree ids of tree_id.hip.
#include "blob_id.hip.h"

#include "git_object_id.hip.h"

namespace mtr {

namespace {

// little-endian u32 at any byte alignment (the summary records are packed bytewise)
__device__ __forceinline__ uint32_t rd32(const uint8_t* p) {
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

// nb of a well-formed record (its nb lengths and blobs fill exactly `size` bytes), -1 otherwise
__device__ __forceinline__ int64_t record_blobs(const uint8_t* rec, int64_t size) {
    if (size < 4) return -1;
    const uint64_t nb = rd32(rec);
    uint64_t sum = 4 + 4 * nb;
    if (sum > uint64_t(size)) return -1;
    for (uint64_t k = 0; k < nb; k++) sum += rd32(rec + 4 + 4 * k);
    return sum == uint64_t(size) ? int64_t(nb) : -1;
}

__global__ void __launch_bounds__(256) blob_count_kernel(const uint8_t* out, const int64_t* off, const int64_t* size,
                                                         uint32_t n, uint32_t* first) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    const int64_t nb = record_blobs(out + off[d], size[d]);
    if (nb < 0) atomicOr(&first[n + 1], 1u);
    first[d] = nb < 0 ? 0u : uint32_t(nb);
}

// exclusive scan of first[0, n) in place, the sum to first[n]: one workgroup, a contiguous chunk per thread
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads) blob_scan_kernel(uint32_t* first, uint32_t n) {
    __shared__ uint32_t part[kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = min(n, t * chunk), hi = min(n, lo + chunk);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += first[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t step = 1; step < kScanThreads; step <<= 1) {
        const uint32_t v = t >= step ? part[t - step] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t c = first[i];
        first[i] = run;
        run += c;
    }
    if (t == kScanThreads - 1) first[n] = part[t];
}

__global__ void __launch_bounds__(256) blob_fill_kernel(const uint8_t* out, const int64_t* off, const uint32_t* first,
                                                        uint32_t n, uint64_t* boff, uint32_t* blen) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    const uint32_t b0 = first[d], nb = first[d + 1] - b0;  // (0 for a record blob_count_kernel refused)
    const uint8_t* rec = out + off[d];
    uint64_t pos = uint64_t(off[d]) + 4 + 4 * uint64_t(nb);
    for (uint32_t k = 0; k < nb; k++) {
        const uint32_t len = rd32(rec + 4 + 4 * k);
        boff[b0 + k] = pos;
        blen[b0 + k] = len;
        pos += len;
    }
}

// ---- the blob table of a document range that continues a summary (the pipelined hand-over): first[lo] already holds
// the blobs of the documents before lo (0 for lo = 0), so the counts go one word up and an inclusive scan finishes them

// first[d + 1] = the blobs of document d for d in [lo, hi); a malformed record counts none and raises *bad
__global__ void __launch_bounds__(256) blob_count_range_kernel(const uint8_t* out, const int64_t* off,
                                                               const int64_t* size, uint32_t lo, uint32_t hi,
                                                               uint32_t* first, uint32_t* bad) {
    const uint32_t d = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= hi) return;
    const int64_t nb = record_blobs(out + off[d], size[d]);
    if (nb < 0) atomicOr(bad, 1u);
    first[d + 1] = nb < 0 ? 0u : uint32_t(nb);
}

// first[d + 1] = first[lo] + the counts of [lo, d] for d in [lo, hi): blob_scan_kernel's scheme, inclusive and with
// the base the earlier ranges left.  host[0] = first[hi] (the summary's blobs so far), host[1] = *bad, for the host
// that waits on an event recorded after this kernel (mapped memory).
__global__ void __launch_bounds__(kScanThreads) blob_scan_range_kernel(uint32_t* first, uint32_t lo, uint32_t hi,
                                                                       const uint32_t* bad, int64_t* host) {
    __shared__ uint32_t part[kScanThreads];
    const uint32_t t = threadIdx.x, n = hi - lo;
    uint32_t* a = first + lo + 1;
    const uint32_t base = first[lo];
    const uint32_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t c0 = min(n, t * chunk), c1 = min(n, c0 + chunk);
    uint32_t sum = 0;
    for (uint32_t i = c0; i < c1; i++) sum += a[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t step = 1; step < kScanThreads; step <<= 1) {
        const uint32_t v = t >= step ? part[t - step] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = base + part[t] - sum;
    for (uint32_t i = c0; i < c1; i++) {
        run += a[i];
        a[i] = run;
    }
    if (t == kScanThreads - 1) {
        host[0] = int64_t(base + part[t]);
        host[1] = int64_t(*bad);
        __threadfence_system();
    }
}

}  // namespace

// One lane per blob; the message layout and the loads are git_object_id's (git_object_id.hip.h).
constexpr int kIdThreads = 64;  // one wave per workgroup: a workgroup ends with its longest blob
__global__ void __launch_bounds__(kIdThreads) __attribute__((amdgpu_waves_per_eu(8)))
git_blob_id_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ boff,
                   const uint32_t* __restrict__ blen, uint32_t n_blobs, uint32_t* __restrict__ ids) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_blobs) return;
    git_object_id(kGitTypeBlob, uintptr_t(bytes) + boff[i], blen[i], ids + 5 * size_t(i));
}

hipError_t blob_table_count(const uint8_t* out, const int64_t* off, const int64_t* size, uint32_t n, uint32_t* first,
                            hipStream_t s) {
    hipError_t rc = hipMemsetAsync(first + n, 0, 2 * sizeof(uint32_t), s);
    if (rc != hipSuccess) return rc;
    if (n) blob_count_kernel<<<(n + 255) / 256, 256, 0, s>>>(out, off, size, n, first);
    blob_scan_kernel<<<1, kScanThreads, 0, s>>>(first, n);
    return hipGetLastError();
}

hipError_t scan_u32_launch(uint32_t* a, uint32_t n, hipStream_t s) {
    blob_scan_kernel<<<1, kScanThreads, 0, s>>>(a, n);
    return hipGetLastError();
}

hipError_t blob_table_count_range(const uint8_t* out, const int64_t* off, const int64_t* size, uint32_t lo, uint32_t hi,
                                  uint32_t* first, uint32_t* bad, int64_t* host, hipStream_t s) {
    if (hi > lo) blob_count_range_kernel<<<(hi - lo + 255) / 256, 256, 0, s>>>(out, off, size, lo, hi, first, bad);
    blob_scan_range_kernel<<<1, kScanThreads, 0, s>>>(first, lo, hi, bad, host);
    return hipGetLastError();
}

hipError_t blob_table_fill(const uint8_t* out, const int64_t* off, const uint32_t* first, uint32_t n, uint64_t* boff,
                           uint32_t* blen, hipStream_t s) {
    if (n) blob_fill_kernel<<<(n + 255) / 256, 256, 0, s>>>(out, off, first, n, boff, blen);
    return hipGetLastError();
}

hipError_t git_blob_ids_launch(const uint8_t* bytes, const uint64_t* boff, const uint32_t* blen, uint32_t n_blobs,
                               uint32_t* ids, hipStream_t s) {
    if (n_blobs) git_blob_id_kernel<<<(n_blobs + kIdThreads - 1) / kIdThreads, kIdThreads, 0, s>>>(bytes, boff, blen, n_blobs, ids);
    return hipGetLastError();
}

}  // namespace mtr
