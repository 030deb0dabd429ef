// summary_delta.hip.h -- the incremental summary hand-over (mtr_summary_delta): which blobs of the current summary
// differ from a baseline of git blob ids, and their bytes gathered into one compact buffer.
// The kernels live in summary_delta.hip; handover.hip drives them through these launchers (all asynchronous on `s`).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mtr {

// Per blob b of the current summary (n_blobs blobs of n_docs documents; first / blen / ids as blob_id.hip.h makes
// them): flags[b] = 1 when the baseline holds no equal id at the same (document, index in the document), else 0;
// clen[b] = blen[b] for a changed blob, 0 otherwise.  The baseline is base_docs documents, document d's ids are
// base_ids[5 * base_first[d] .. 5 * base_first[d + 1]); base_docs = 0 (the pointers may then be null): every blob is
// changed.
hipError_t delta_flag_launch(const uint32_t* first, uint32_t n_docs, const uint32_t* blen, const uint32_t* ids,
                             uint32_t n_blobs, const uint32_t* base_first, const uint32_t* base_ids,
                             uint32_t base_docs, uint8_t* flags, uint64_t* clen, hipStream_t s);

// Exclusive 64-bit scan of clen[0, n_blobs) in place (clen[n_blobs] = the sum: clen becomes delta_off), and the
// changed blobs compacted in order: chg_off[j] = the j-th changed blob's offset in the compact buffer
// (chg_off[changed] = the sum), chg_src[j] = its offset in the summary buffer (boff).  rank[b] = the changed blobs
// before blob b (rank[n_blobs] = all of them).  tot[0] = the changed blobs, tot[1] = their bytes.  clen, rank and
// chg_off hold n_blobs + 1 entries, chg_src n_blobs.
hipError_t delta_scan_launch(const uint8_t* flags, const uint64_t* boff, uint32_t n_blobs, uint64_t* clen,
                             uint32_t* rank, uint64_t* chg_off, uint64_t* chg_src, uint64_t* tot, hipStream_t s);

// dst[chg_off[j], chg_off[j + 1]) = src[chg_src[j], ...) for j in [0, changed); total = chg_off[changed].
// src must be the start of an allocation that extends 16 bytes past the last source byte, dst one that holds
// total + 16 bytes (the last 16-byte store may run past total); both 16-byte aligned.
hipError_t delta_gather_launch(const uint8_t* src, const uint64_t* chg_off, const uint64_t* chg_src, uint32_t changed,
                               uint64_t total, uint8_t* dst, hipStream_t s);

// The two kernels for a summary that is compacted range by range, the ranges in blob order on one stream (the
// pipelined hand-over).  The scan over the blobs [b0, b0 + n): tot[0] / tot[1] carry the chosen blobs and their bytes
// from range to range (the caller zeroes them before the first), every position written is summary-wide, and after
// the last range clen, rank, chg_off, chg_src and tot are what delta_scan_launch over all blobs leaves.  host (mapped
// memory, 2 words) receives the new tot.
hipError_t delta_scan_range_launch(const uint8_t* flags, const uint64_t* boff, uint32_t b0, uint32_t n, uint64_t* clen,
                                   uint32_t* rank, uint64_t* chg_off, uint64_t* chg_src, uint64_t* tot, int64_t* host,
                                   hipStream_t s);

// dst[o0, o1) = the range's chosen blobs [j0, j1) (chg_off[j0] = o0, chg_off[j1] = o1).  o0 may be any byte: dst
// below o0 is not written.  Zeros may follow up to 15 bytes past o1, where the next range's bytes land; dst holds 16
// bytes more than the last range's end.  src as delta_gather_launch's.
hipError_t delta_gather_range_launch(const uint8_t* src, const uint64_t* chg_off, const uint64_t* chg_src, uint32_t j0,
                                     uint32_t j1, uint64_t o0, uint64_t o1, uint8_t* dst, hipStream_t s);

}  // namespace mtr
