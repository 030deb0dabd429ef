// blob_cache.hip.h -- the device blob-id cache (mtr_blob_cache_* / mtr_summary_novel): a set of 20-byte git blob ids
// that stands in for SummaryTreeUploadManager's blobsShaCache, and the pass that sorts the current summary's blobs
// into "storage holds it", "new: upload this copy" and "new, but an earlier blob of this summary is the same object".
// The kernels live in blob_cache.hip; handover.hip drives them through these launchers (all asynchronous on `s`).
//
// A set is an id table (5 u32 words an id, append-only until a trim compacts it into a fresh one) and an
// open-addressing slot array of u32 (linear probing, a power of two of slots, at most half of them used) that holds
// `entry index + 1`, 0 = empty.  A slot never holds an
// id, only the index of one that was complete in memory before the kernel started: a lane that meets an occupied slot
// compares all 160 bits against that entry and moves on or stops; no lane ever waits for another.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mtr {

constexpr uint32_t kCacheMinSlots = 1024;    // a cache's first slot array; it doubles from there
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;    // where[]: the id sits in no slot of the set being filled

// Inserts the n ids src[5 i ..] into the set (table, slots): entry j of the set is table[5 j ..] for j < held and
// src[5 (j - held) ..] from there on, so source id i is offered as entry held + i.  Ids the set holds are absorbed;
// of equal source ids the slot ends up holding the smallest (an atomicMin on the slot: equal ids only ever replace
// each other there).  where[i] (may be null) = the slot that holds id i's entry.  slots has mask + 1 entries, of which
// at least half stay empty.  Re-inserting a table into a fresh slot array is held = 0, src = the table.
hipError_t cache_insert_launch(const uint32_t* table, uint32_t held, const uint32_t* src, uint32_t n, uint32_t* slots,
                               uint32_t mask, uint32_t* where, hipStream_t s);

// After cache_insert_launch: isnew[i] = 1 when source id i is the one its slot kept (the smallest index of a new id),
// rank[i] = the new ids before i (rank[n] and tot[0] = all of them): the order new entries are appended in.
hipError_t cache_rank_launch(const uint32_t* slots, const uint32_t* where, uint32_t held, uint32_t n, uint8_t* isnew,
                             uint32_t* rank, uint32_t* tot, hipStream_t s);

// Appends the new ids: table[5 (held + rank[i]) ..] = src[5 i ..] and the id's slot now names that entry.  table
// holds held + tot[0] entries.
hipError_t cache_commit_launch(const uint32_t* src, const uint8_t* isnew, const uint32_t* rank, const uint32_t* where,
                               uint32_t held, uint32_t n, uint32_t* table, uint32_t* slots, hipStream_t s);

// out[i] = 1 when the set holds q[5 i ..], else 0.
hipError_t cache_has_launch(const uint32_t* table, const uint32_t* slots, uint32_t mask, const uint32_t* q, uint32_t n,
                            uint8_t* out, hipStream_t s);

// The life cycle.  stamp[j] = the generation that last offered entry j's id (one word per entry of the table).
// After an add's commit: stamp[entry of q[5 i ..]] = max(itself, age ? gen - age[i] : gen) for the n offered ids; equal
// ids of one call end with the largest value.  (An id the set does not hold is passed over.)
hipError_t cache_stamp_launch(const uint32_t* table, const uint32_t* slots, uint32_t mask, const uint32_t* q,
                              const uint32_t* age, uint32_t gen, uint32_t n, uint32_t* stamp, hipStream_t s);

// out[min(gen - stamp[j], n - 1)] += 1 for every entry j < count; out has n <= 1024 buckets, zeroed by the caller.
hipError_t cache_age_hist_launch(const uint32_t* stamp, uint32_t count, uint32_t gen, uint32_t n,
                                 unsigned long long* out, hipStream_t s);

// out[0] += the entries j < count with stamp[j] >= cutoff.
hipError_t cache_count_launch(const uint32_t* stamp, uint32_t count, uint64_t cutoff, unsigned long long* out,
                              hipStream_t s);

// A trim's first half: keep[j] = stamp[j] >= cutoff, idx[j] = the survivors before entry j (idx[count] and tot[0] =
// all of them; one workgroup scans, as cache_rank_launch).
hipError_t cache_keep_launch(const uint32_t* stamp, uint32_t count, uint64_t cutoff, uint8_t* keep, uint32_t* idx,
                             uint32_t* tot, hipStream_t s);

// Its second half: survivor j's five id words and stamp to entry idx[j] of (ntable, nstamp), which hold tot[0]
// entries; table order is kept.  The caller then fills a zeroed slot array with cache_insert_launch(held = 0,
// src = ntable).
hipError_t cache_compact_launch(const uint32_t* table, const uint32_t* stamp, const uint8_t* keep, const uint32_t* idx,
                                uint32_t count, uint32_t* ntable, uint32_t* nstamp, hipStream_t s);

// One lane per blob b of the current summary (ids as blob_id.hip.h makes them): a blob the cache (table, cslots,
// cmask; cslots null = no cache) holds gets where[b] = kNoSlot; any other is inserted as entry b into the summary's
// own set `slots` (zeroed, mask + 1 >= 2 n_blobs entries), where[b] = its slot.  When the kernel has ended, a slot
// holds the smallest blob index with that id.
hipError_t novel_classify_launch(const uint32_t* ids, uint32_t n_blobs, const uint32_t* table, const uint32_t* cslots,
                                 uint32_t cmask, uint32_t* slots, uint32_t mask, uint32_t* where, hipStream_t s);

// state[b] = 0 (the cache holds it), 1 (new, and b is the smallest index with the id) or 2 (new, an earlier blob is
// the same); rep[b] = that smallest index (0xFFFFFFFF for state 0); flags[b] = 1 for state 1, clen[b] = blen[b] for
// state 1 and 0 otherwise: what delta_scan_launch and delta_gather_launch compact and gather.
hipError_t novel_state_launch(const uint32_t* slots, const uint32_t* where, const uint32_t* blen, uint32_t n_blobs,
                              uint8_t* state, uint32_t* rep, uint8_t* flags, uint64_t* clen, hipStream_t s);

// Both passes over the blobs [b0, b1) of a summary that is classified range by range (the pipelined hand-over):
// indices, where / state / rep / flags / clen positions and the summary's own set are summary-wide; the set is zeroed
// once, before the first range, and sized for every blob of the summary.  The ranges must be launched in blob order
// on one stream: a range's states and reps are final when its kernels end because every later index is larger.
hipError_t novel_range_launch(const uint32_t* ids, const uint32_t* blen, uint32_t b0, uint32_t b1,
                              const uint32_t* table, const uint32_t* cslots, uint32_t cmask, uint32_t* slots,
                              uint32_t mask, uint32_t* where, uint8_t* state, uint32_t* rep, uint8_t* flags,
                              uint64_t* clen, hipStream_t s);

}  // namespace mtr
