// blob_id.hip.h -- git blob ids (SHA-1 of "blob <len>\0" + bytes) of the summary blobs, hashed on the device.
// The kernels live in blob_id.hip; handover.hip drives them through these launchers (all asynchronous on `s`).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mtr {

// The blob table of n summary records (mtr_get_summaries' layout: u32 nb, nb u32 lengths, the blobs back to back;
// record d = out[off[d], off[d] + size[d])).  first[d] receives the index of document d's first blob, first[n] the
// blob count, first[n + 1] a flag: non-zero when some record's blob lengths do not add up to its size (that
// document then counts no blobs).  first holds n + 2 words.
hipError_t blob_table_count(const uint8_t* out, const int64_t* off, const int64_t* size, uint32_t n, uint32_t* first,
                            hipStream_t s);
// The same table for the records of documents [lo, hi) of a summary whose earlier documents are in it already (the
// pipelined hand-over's ranges, in document order on one stream): first[lo] holds the blobs before document lo (the
// caller zeroes first[0]), first[lo + 1 .. hi] receive the first blobs of the documents after lo and the count so
// far.  *bad is raised by a record whose lengths do not add up (the caller zeroes it once; first[n_docs + 1] serves).
// host (mapped memory, 2 words) receives first[hi] and *bad.
hipError_t blob_table_count_range(const uint8_t* out, const int64_t* off, const int64_t* size, uint32_t lo, uint32_t hi,
                                  uint32_t* first, uint32_t* bad, int64_t* host, hipStream_t s);
// Exclusive scan of a[0, n) in place, the sum to a[n] (a holds n + 1 words): the single-workgroup scan of the blob table.
hipError_t scan_u32_launch(uint32_t* a, uint32_t n, hipStream_t s);
// Per blob its byte offset in `out` and its length, from the table blob_table_count made.
hipError_t blob_table_fill(const uint8_t* out, const int64_t* off, const uint32_t* first, uint32_t n, uint64_t* boff,
                           uint32_t* blen, hipStream_t s);
// ids[5 i .. 5 i + 5) = the 20 id bytes of blob i = bytes[boff[i], boff[i] + blen[i]).  Reads only the aligned
// 32-bit words of `bytes` that hold at least one byte of a blob; `bytes` must be 4-byte aligned.
hipError_t git_blob_ids_launch(const uint8_t* bytes, const uint64_t* boff, const uint32_t* blen, uint32_t n_blobs,
                               uint32_t* ids, hipStream_t s);

}  // namespace mtr
