/*
 * mtr.h -- C ABI of the MI355X batched merge-tree replay engine (libmtr.so).
 *
 * The engine is a drop-in for the *observer* (all-ops-remote) path of
 * @fluidframework/merge-tree's Client (packages/dds/merge-tree/src/client.ts:98):
 * a scribe-like summarizer or a replay tool hands it ISequencedDocumentMessage
 * batches for many documents at once and asks for each document's summary.
 * Paths below are relative to the reference's packages/dds/merge-tree/src/.
 *
 *   reference                                      | engine
 *   -----------------------------------------------+------------------------------------------
 *   new Client(specToSegment, logger, options)      | mtr_engine_create   (client.ts:107-131)
 *     IMergeTreeOptions (mergeTree.ts:400-438)      |   mtr_options
 *   Client.startOrUpdateCollaboration(id, min, cur) | MTR_OP_START_COLLAB record (client.ts:1133)
 *   Client.applyMsg(msg) for every message          | mtr_submit + mtr_run (client.ts:858-887)
 *   Client.updateSeqNumbers(min, seq)               | MTR_F_LAST / MTR_OP_SEQ records (client.ts:877)
 *   Client.summarize(runtime, handle, ser, [])      | mtr_summarize + mtr_get_summary (client.ts:966)
 *   createTextHelper().getText()                    | mtr_get_text (MergeTreeTextHelper.ts:20)
 *   ...getText(refSeq, clientId, ph, start, end),   | mtr_get_range_segments (MergeTreeTextHelper.ts:20-81,
 *     Client.walkSegments(handler, start, end)      |   client.ts walkSegments), many ranges at once
 *   Client.resolveRemoteClientPosition(pos, refSeq, | mtr_transform_positions (MTR_POS_FROM_VIEW / _FROM_LEAF),
 *     clientId), Client.getPosition(segment)        |   many (document, view) pairs at once
 *   IntervalCollection.findOverlappingIntervals,    | mtr_query_intervals (MTR_IVQ_OVERLAP / _PREVIOUS / _NEXT),
 *     previousInterval, nextInterval                |   many collections of many documents at once
 *   assert(cond, 0xNNN) / UsageError                | mtr_doc_status (per-document status word)
 *
 * No exceptions cross the ABI; every call returns MTR_OK (0) or an error code.
 * All pointers are host pointers; device memory is owned by the engine.
 */
#ifndef MTR_H
#define MTR_H

#include <stddef.h>
#include <stdint.h>

#include "mtr_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mtr_engine mtr_engine;

/* Per-document device arena capacities (0 = engine default). */
typedef struct mtr_caps {
    uint32_t max_segments;   /* leaf records per document */
    uint32_t heap_entries;   /* zamboni LRU heap entries per document (heap.ts:11) */
    uint32_t text_units;     /* UTF-16 text arena per document */
    uint32_t prop_words;     /* property-set arena per document (u32 words) */
    uint32_t remover_cells;  /* overlapping-remove list cells per document */
    uint32_t ops_per_launch; /* ops applied per document per kernel launch (0 = all) */
    uint32_t ref_slots;      /* local references per document (allocated with the first batch that creates one) */
} mtr_caps;

/* Create an engine for up to max_docs documents on HIP device `device`. */
mtr_engine* mtr_engine_create(const mtr_options* opt, int device, uint32_t max_docs, const mtr_caps* caps);
int mtr_engine_destroy(mtr_engine* e);

/* Forget every document (all state back to a fresh Client); keeps allocations. */
int mtr_reset(mtr_engine* e);

/* Copy a batch to the device (async on the engine stream).  Document i of the batch is
 * engine document i.  The batch's host arrays may be reused after mtr_sync. */
int mtr_submit(mtr_engine* e, const mtr_batch* b);

/* mtr_submit with the hand-over pipelined (SURVEY 8d's end-to-end path: a summarizer handing over sequenced
 * remote messages).  The batch's document descriptors and tables are copied at once; its op records and text
 * go over in `parts` document ranges on a copy stream, and the next mtr_run starts each range's documents as
 * soon as their records have landed, so the upload overlaps the apply of the ranges before it.  Same results as
 * mtr_submit + mtr_run.  The batch's host arrays must stay valid (and, for an overlapped copy, page-locked:
 * mtr_host_alloc) until mtr_run returns.  Only the remote-op path is pipelined: a range holding MTR_F_DELTA,
 * local-op, local-reference or rare records (op_scan) is not started, and mtr_run then returns
 * MTR_ERR_UNSUPPORTED -- mtr_reset and submit that batch with mtr_submit.  Documents must be laid out in order
 * (each document's op records and text after the previous one's); parts <= 1 is mtr_submit. */
int mtr_submit_pipelined(mtr_engine* e, const mtr_batch* b, uint32_t parts);

/* The whole end-to-end hand-over in one call: mtr_submit_pipelined + mtr_run + mtr_summarize + mtr_get_summaries
 * over every document, pipelined at both ends -- a range whose documents have no ops left is summarized and its
 * records downloaded into `out` (cap bytes; page-locked for the copies to overlap) while the later ranges still
 * upload and apply.  Writes doc_off[0..n_docs] (as mtr_get_summaries) and returns the byte count, or -1
 * (mtr_last_error).  When cap is too small the error text starts "mtr_replay_pipelined: the output buffer holds":
 * the batch is then applied in full and mtr_summarize + mtr_get_summaries give its records.  The summaries stay
 * readable afterwards
 * (mtr_get_summary, mtr_get_summaries, mtr_hashes).  A batch the pipelined path does not take (see
 * mtr_submit_pipelined), or whose ranges would hold fewer than 3,000 documents each (MTR_PIPE_MIN_PART_DOCS), runs
 * the serial calls.  Replaces, for a summarizer, the applyMsg loop followed by
 * summarizeCore (SURVEY 8d's end-to-end row). */
int64_t mtr_replay_pipelined(mtr_engine* e, const mtr_batch* b, uint32_t parts, uint8_t* out, int64_t cap,
                             int64_t* doc_off);

/* Apply the submitted ops (Client.applyMsg for each message, in order, per document). Async. */
int mtr_run(mtr_engine* e);

/* Declare documents rows_doc and cols_doc to be the rows and cols PermutationVectors of one
 * SharedMatrix (replaces `new PermutationVector(...)` x2 in the SharedMatrix constructor,
 * matrix.ts:106-121).  The rows document's op list drives both (see MTR_OP_SETCELL / MTR_F_COLS in
 * mtr_types.h); each vector's summary is its SnapshotV1 blobs followed by its handleTable blob
 * (PermutationVector.summarize, permutationvector.ts:310-325).  Persistent across mtr_reset. */
int mtr_set_matrix(mtr_engine* e, uint32_t rows_doc, uint32_t cols_doc);

/* The delta records (mtr_delta) of the MTR_F_DELTA ops of the last submitted batch for one document,
 * in op order: for a SharedString the SequenceDeltaEvent ranges SharedSegmentSequence turns into
 * catch-up ops (sequence.ts:697-736); for a SharedMatrix vector document the MTR_DELTA_CELL /
 * MTR_DELTA_RECYCLE records of its cell tracking (include/mtr_types.h).  Returns the count, or
 * -(count) if cap is too small.  mtr_submit sizes each document's buffer by an exact bound (see
 * mtr_submit in mtr_engine.hip). */
int64_t mtr_get_deltas(mtr_engine* e, uint32_t doc, mtr_delta* out, int64_t cap);

/* The properties an MTR_DELTA_REGEN_X record references (its len field): [n, key id, value id, ...] in JS
 * own-key order, the ids of the batch tables' keys and values -- the segment's `properties` that
 * createInsertSegmentOp serializes (client.ts:763-768 -> TextSegment / Marker.toJSONObject).  Returns the
 * word count 2n + 1, -(that) when cap is too small, -1 on a bad reference (pass cap >= 1: an empty set's one
 * word then always fits, so -1 is never a size).  Replaces reading
 * segment.properties in resetPendingDeltaToOps (client.ts:708-800). */
int64_t mtr_get_props(mtr_engine* e, uint32_t doc, uint32_t ref, uint32_t* out, int64_t cap);

/* mtr_get_deltas for n documents at once, with the property sets mtr_get_props returns for their regenerate records:
 * the SequenceDeltaEvent ranges of a fleet's catch-up ops (sequence.ts:697-736) and the members of its reconnect ops
 * (resetPendingDeltaToOps, client.ts:708-800) in two launches, at most one upload and four downloads, whatever n is.
 *   docs       [n] documents in any order, repeats allowed; NULL = documents 0 .. n - 1.
 *   doc_first  [n + 1], required when n > 0: the exclusive scan of the documents' record counts, the total last.
 *   out        out[doc_first[i] + k] = record k of docs[i], field for field what mtr_get_deltas(e, docs[i], ...)
 *              writes for the last submitted batch.
 *   props_off  [total + 1] offsets into props per record.  A MTR_DELTA_REGEN_X record of a SharedString document with
 *              len >= 0 has the words mtr_get_props(e, doc, rec.len, ...) returns, [n, key id, value id, ...]; every
 *              other record has none: another kind, len == -1, and every record of a matrix vector document
 *              (mtr_set_matrix), whose REGEN_X fields are handles.  NULL skips the part: it is neither measured nor
 *              checked.  props == NULL with props_off given is a size query for the words (props_off is filled).
 * A document's count is its DocHdr.dused when the last submitted batch held it, and 0 otherwise: for doc >= that
 * batch's n_docs, for every document while that batch had no MTR_F_DELTA op, and after the pipelined submits, which
 * take no delta ops.  (For doc >= n_docs mtr_get_deltas returns a count left over from an earlier batch and writes
 * nothing; the batched call reports 0 there.)
 * Returns the total record count.  out == NULL is a size query: doc_first is filled; props_off must be NULL then (-1).
 * cap < total, or a non-NULL props with props_cap below the word total: MTR_SUMMARY_TOO_SMALL, doc_first written,
 * props_off written in full when cap >= total, no records or words written.  -1 (mtr_last_error) with nothing written:
 * a missing doc_first, a docs[i] >= max_docs (named by its index i), a header whose dused is negative or exceeds the
 * document's slice of the record buffer, or -- in the props part -- a reference whose set does not lie inside the
 * document's property arena (mtr_get_props' check, made on the device).  n = 0 returns 0 with doc_first[0] = 0 (and
 * props_off[0] = 0) when given and no device work.  The call only reads state: the records and their counts, the
 * cached summary, id, delta and novel results stay, and the call may be repeated. */
int64_t mtr_get_deltas_batch(mtr_engine* e, const uint32_t* docs, uint32_t n, mtr_delta* out, int64_t cap,
                             int64_t* doc_first, uint32_t* props, int64_t props_cap, int64_t* props_off);

/* Build every document's summary blobs on the device (Client.summarize). Async except for
 * one small size read-back between the sizing and writing passes. */
int mtr_summarize(mtr_engine* e);

/* Wait for all queued work on the engine stream. */
int mtr_sync(mtr_engine* e);

/* Size of one document's summary after mtr_summarize (SnapshotV1/Legacy emit, snapshotV1.ts:122-178,
 * snapshotlegacy.ts:122-182): *n_blobs = number of blobs, *n_bytes = their total payload bytes.
 * Callers size the buffers of mtr_get_summary from it.  Returns MTR_OK or -1 (mtr_last_error). */
int mtr_summary_info(mtr_engine* e, uint32_t doc, int64_t* n_blobs, int64_t* n_bytes);

/* Blobs of one document after mtr_summarize: writes them back-to-back to out (cap bytes),
 * blob_len[k] = bytes of blob k (order: header, body / body_0, body_1, ...).
 * Returns the number of blobs (>= 1); MTR_SUMMARY_TOO_SMALL when cap or max_blobs is smaller than
 * mtr_summary_info reports (nothing written); -1 on any other error (mtr_last_error). */
#define MTR_SUMMARY_TOO_SMALL (-3)
int64_t mtr_get_summary(mtr_engine* e, uint32_t doc, uint8_t* out, int64_t cap, int64_t* blob_len,
                        int32_t max_blobs);

/* Bulk download of the summaries of documents [lo, hi) in ONE device-to-host copy (a scribe hands
 * every blob of a batch to storage at once).  Layout: per document, in order, a little-endian u32
 * blob count nb, nb u32 blob lengths, then the blob bytes.  doc_off[i] (hi - lo + 1 entries) = offset
 * of document lo + i in out; doc_off[hi - lo] = total bytes.  Returns the total bytes, or -(bytes
 * needed) when cap is too small (nothing written; a non-empty range always needs >= 8 bytes), or -1
 * on error.  `out` may be pinned memory from mtr_host_alloc for full PCIe bandwidth. */
int64_t mtr_get_summaries(mtr_engine* e, uint32_t lo, uint32_t hi, uint8_t* out, int64_t cap, int64_t* doc_off);

/* Page-locked host memory (hipHostMalloc) for op batches and summary downloads; NULL on failure. */
void* mtr_host_alloc(uint64_t bytes);
int mtr_host_free(void* p);

/* 64-bit FNV-1a of every document's summary (blob lengths + bytes), n_docs entries. */
int mtr_summary_hashes(mtr_engine* e, uint64_t* out, uint32_t n_docs);

/* Total summary bytes of all documents (after mtr_summarize). */
int64_t mtr_summary_bytes(mtr_engine* e);

/* Git blob ids: SHA-1 of "blob <byte length in decimal>\0" followed by the blob's bytes -- what `git hash-object`
 * prints and gitHashFile (@fluidframework/common-utils) returns, the name Fluid's git storage (gitrest / historian)
 * knows a blob by.  Hashed on the device, one lane per blob. */
#define MTR_BLOB_ID_BYTES 20

/* Ids of the summary blobs of documents [lo, hi) after mtr_summarize or mtr_replay_pipelined
 * (valid exactly where mtr_get_summaries is).  out receives 20 bytes per blob in record order
 * (header, body / body_0, ...; for a matrix vector its V1 blobs then handleTable);
 * doc_first[i] (hi - lo + 1 entries) = index in out of document lo + i's first blob,
 * doc_first[hi - lo] = the count.
 * Returns the count, -(count needed) when cap_blobs is too small (nothing written),
 * -1 on error (mtr_last_error); pass cap_blobs >= 1 and -1 is never a size.  The ids of every document are
 * computed on the first call after a summary and kept on the device; later calls only download.
 * Replaces gitHashFile over every blob in SummaryTreeUploadManager (routerlicious-driver). */
int64_t mtr_summary_blob_ids(mtr_engine* e, uint32_t lo, uint32_t hi, uint8_t* out, int64_t cap_blobs,
                             int64_t* doc_first);

/* Ids of n blobs in caller memory: blob i is bytes[off[i], off[i + 1]).
 * Uploads, hashes on the device, downloads n * 20 bytes.
 * For the blobs the host makes itself (catch-up ops, interval header) and for tests. */
int mtr_git_blob_ids(mtr_engine* e, const uint8_t* bytes, const int64_t* off, uint32_t n, uint8_t* out);

/* Incremental hand-over.  A baseline is a set of blob ids keyed by (document, blob index in record order): the ids of
 * the summary storage already holds.  A blob of the current summary is "changed" when its document or its index is
 * not in the baseline or the id there differs; the name of blob k of a document is fixed by k, so the same index is
 * the same path in the summary tree.  With no baseline every blob is changed.  The baseline is content-addressed
 * data: it survives mtr_submit, mtr_run, mtr_summarize, the pipelined calls and mtr_reset; only the three calls below
 * and mtr_engine_destroy drop it.
 *
 * mtr_summary_set_baseline: the current summary's ids become the baseline (valid exactly where mtr_summary_blob_ids
 * is; computes the ids if no call has yet; a device-to-device copy, the current ids stay valid). */
int mtr_summary_set_baseline(mtr_engine* e);
/* A baseline from the host, in the layout mtr_summary_blob_ids returns: 20 bytes per blob, doc_first[n_docs + 1]
 * non-decreasing from 0 (-1 otherwise).  For a summarizer that starts from a stored tree or restarts.  n_docs may be
 * smaller or larger than the engine's document count; 0 documents is no baseline. */
int mtr_summary_set_baseline_ids(mtr_engine* e, const uint8_t* ids, const int64_t* doc_first, uint32_t n_docs);
/* Drops the baseline. */
int mtr_summary_clear_baseline(mtr_engine* e);

/* Sizes of the delta of documents [lo, hi): blobs in the range, how many changed, their total bytes.  Valid exactly
 * where mtr_summary_blob_ids is (-1 otherwise).  The delta of every document is built on the first call after a
 * summary or a baseline call (a flag kernel, a 64-bit scan, a gather of the changed blobs into one compact device
 * buffer) and kept on the device; later calls only download. */
int mtr_summary_delta_info(mtr_engine* e, uint32_t lo, uint32_t hi, int64_t* n_blobs, int64_t* n_changed,
                           int64_t* changed_bytes);

/* flags[k] (n_blobs bytes): 1 = blob k of the range is new or differs from the baseline, 0 = the baseline holds
 * the same id at the same (document, index).  blob_off[n_blobs + 1]: blob k's bytes are
 * out[blob_off[k], blob_off[k + 1]) -- empty for an unchanged blob.  doc_first[hi - lo + 1] as in
 * mtr_summary_blob_ids.  out receives the changed blobs back to back in ONE device-to-host copy (may be pinned).
 * Returns changed_bytes; MTR_SUMMARY_TOO_SMALL when cap_bytes or cap_blobs is below what _info reports (nothing
 * written); -1 on error.  An empty range returns 0 and writes doc_first[0] = blob_off[0] = 0.
 * Blobs the baseline has but the current summary lacks (a document that shrank to fewer chunks) are not reported: the
 * host sees that from doc_first against its own record of the baseline.
 * The host uploads the changed blobs, refers to the others by id (mtr_summary_blob_ids), and calls
 * mtr_summary_set_baseline once storage has acknowledged. */
int64_t mtr_summary_delta(mtr_engine* e, uint32_t lo, uint32_t hi, uint8_t* out, int64_t cap_bytes, uint8_t* flags,
                          int64_t* blob_off, int64_t cap_blobs, int64_t* doc_first);

/* The blob-id cache: a set of 20-byte blob ids kept on the device, the ids storage holds under any path of any
 * document.  It stands in for SummaryTreeUploadManager's blobsShaCache (writeSummaryBlob skips the upload of a blob
 * whose sha the cache holds: git storage is content-addressed).  Content-addressed data like the baseline and
 * independent of it: it survives mtr_submit, mtr_run, mtr_summarize, the pipelined calls and mtr_reset; only the
 * mtr_blob_cache_* calls and mtr_engine_destroy change it, and the baseline and delta calls behave the same with or
 * without one.  At most 2^31 - 1 ids.  Every call returns MTR_OK or -1 (mtr_last_error) unless stated.
 *
 * mtr_blob_cache_add: n ids from the host (20 bytes each); ids the cache holds and repeats within the call are
 * absorbed; n = 0 is a no-op. */
int mtr_blob_cache_add(mtr_engine* e, const uint8_t* ids, int64_t n);
/* Adds the id of every blob of the current summary, device to device: the "storage acknowledged" step.  Valid exactly
 * where mtr_summary_blob_ids is; computes the ids if no call has yet. */
int mtr_blob_cache_add_summary(mtr_engine* e);
int mtr_blob_cache_clear(mtr_engine* e);
/* The number of distinct ids held (-1: no engine). */
int64_t mtr_blob_cache_size(mtr_engine* e);
/* out[i] = 1 when the cache holds ids[20 i ..], else 0: for the blobs the host makes itself. */
int mtr_blob_cache_has(mtr_engine* e, const uint8_t* ids, int64_t n, uint8_t* out);

/* The cache's life cycle: generations, trim, export and import (fluidframework_amd/gitid.py's BlobCacheModel is the
 * host definition).  The cache has a generation, a u32 that starts at 0, and every entry a stamp: the generation at
 * which its id was last offered.  mtr_blob_cache_add stamps every id it is given, held or new, with the current
 * generation; mtr_blob_cache_add_summary first moves to the next generation (one acknowledged summary is one
 * generation; at generation 2^32 - 1 it is refused), so a blob the summary refers to counts as used whether or not it
 * was uploaded.  A stamp only ever grows.  An entry's age is generation - stamp.  Stamps and generation survive what
 * the cache survives; mtr_blob_cache_clear releases the stamps with the ids, every buffer the cache calls work in,
 * and returns to generation 0.  Stamping changes no membership and drops nothing that was built from the set.
 * Every call returns -1 (mtr_last_error) on a bad argument or without an engine.
 *
 * mtr_blob_cache_generation: the current generation. */
int64_t mtr_blob_cache_generation(mtr_engine* e);
/* out[a] = the entries of age a for a < n - 1, out[n - 1] = all older ones; the sum is mtr_blob_cache_size.
 * 1 <= n <= 1024.  A histogram kernel over the stamps; n words come back. */
int mtr_blob_cache_ages(mtr_engine* e, int64_t* out, int32_t n);
/* Drops the entries with stamp < min_generation and returns how many (0: the cache, the generation and the cached
 * mtr_summary_novel result stay as they are; otherwise that result is dropped).  The survivors keep their order.
 * The generation does not change.  On the device: keep flags, their scan, one 4-byte read-back of the kept count,
 * the survivors copied into a fresh table, and a fresh slot array -- the smallest power of two >= max(1024, 2 x
 * kept) -- filled from that table; no entry is ever taken out of a probe chain.  The old table, stamps and slots are
 * released.  Dropping every entry leaves the cache as mtr_blob_cache_clear does, except for the generation. */
int64_t mtr_blob_cache_trim(mtr_engine* e, int64_t min_generation);
/* Trims to at most max_entries (>= 0) entries by whole generations, oldest first: mtr_blob_cache_trim at the smallest
 * cutoff of [0, generation + 1] that keeps no more than max_entries, found from the device's age histogram (and a
 * counting kernel where more than 1,023 generations are in play); no id is downloaded.  An entry is never dropped
 * while one of an older generation stays; a cap that falls inside a generation drops that whole generation;
 * max_entries = 0 empties the cache.  Returns the entries removed. */
int64_t mtr_blob_cache_trim_to(mtr_engine* e, int64_t max_entries);
/* The entries in table order: ids[20 i ..] and ages[i].  Returns the count; -(count) when cap is below it (nothing
 * written); pass cap >= 1.  Two device-to-host copies; drops nothing. */
int64_t mtr_blob_cache_export(mtr_engine* e, uint8_t* ids, uint32_t* ages, int64_t cap);
/* Offers n ids with their ages: the generation becomes max(generation, the largest age given), then every id is added
 * as by mtr_blob_cache_add with stamp = max(stamp, generation - ages[i]) -- of equal ids in one call the youngest age
 * wins.  Importing an export into an engine without a cache reproduces ids, order, ages and generation.  n = 0 is a
 * no-op. */
int mtr_blob_cache_import(mtr_engine* e, const uint8_t* ids, const uint32_t* ages, int64_t n);

/* The current summary against the cache.  Per blob k of documents [lo, hi), in record order:
 *   state[k] = 0  the cache holds its id; no bytes;
 *   state[k] = 1  it does not, and k is the smallest blob index, in record order over ALL documents of the summary,
 *                 with that id: this is the copy to upload, its bytes are out[blob_off[k], blob_off[k + 1]);
 *   state[k] = 2  it does not, and an earlier blob of this summary has the same id; no bytes.
 * rep[k] = the summary-wide index (mtr_summary_blob_ids' order over documents [0, n_docs)) of that smallest-index
 * blob: the blob's own index for state 1, -1 for state 0; it may lie outside the range, and the host then gets those
 * bytes with that range.  Without a cache, or with an empty one, nothing is held: distinct blobs come over once each.
 * Validity, MTR_SUMMARY_TOO_SMALL / -1, the empty range, blob_off, doc_first and the one device-to-host copy of the
 * bytes are mtr_summary_delta's.  The result is built on the device for every document on the first call after the
 * summary or the cache's contents changed (probe the cache, insert the misses into a set of the summary's own, the
 * delta's scan and gather over the first occurrences) and kept there; later calls only download.
 * mtr_summary_novel_info: blobs in the range, how many have state 1, their total bytes.
 * The host uploads the state-1 blobs, refers to all others by id, and calls mtr_blob_cache_add_summary once storage
 * has acknowledged. */
int mtr_summary_novel_info(mtr_engine* e, uint32_t lo, uint32_t hi, int64_t* n_blobs, int64_t* n_first,
                           int64_t* first_bytes);
int64_t mtr_summary_novel(mtr_engine* e, uint32_t lo, uint32_t hi, uint8_t* out, int64_t cap_bytes, uint8_t* state,
                          int64_t* rep, int64_t* blob_off, int64_t cap_blobs, int64_t* doc_first);

/* mtr_replay_pipelined that downloads only the blobs storage lacks.  The call writes, byte for byte and word for
 * word, what mtr_submit + mtr_run + mtr_summarize, then mtr_summary_novel(0, n_docs, out, cap_bytes, state, rep,
 * blob_off, cap_blobs, doc_first), then mtr_summary_blob_ids(0, n_docs, ids, cap_blobs, NULL) write, and returns
 * first_bytes -- but as part of the pipelined run: a range whose documents have no ops left is summarized, its blobs are
 * hashed, classified against the cache and against the blobs of the ranges before it, its first occurrences gathered
 * and those bytes alone downloaded into `out` (page-locked for the copies to overlap), while the later ranges still
 * upload and apply.  The records never cross to the host; the per-blob tables follow when the run has ended.
 * Afterwards the engine is as after a summary whose ids and novel result are built: mtr_get_summary[ies],
 * mtr_summary_hashes, mtr_summary_blob_ids, _tree_ids, _set_baseline, mtr_blob_cache_add_summary and
 * mtr_summary_novel of any range serve without hashing or classifying again.  The cache and the baseline are read,
 * not changed: call mtr_blob_cache_add_summary once storage has acknowledged.
 * cap_blobs and cap_bytes bound everything the run writes: its device buffers are sized from them before the first
 * range starts, and nothing grows while ranges are in flight.  A summary with more blobs than cap_blobs, or more
 * first-occurrence bytes than cap_bytes, is an error (-1) whose text starts "mtr_replay_handover: the output buffers
 * hold": the batch is then applied in full, and mtr_summarize + the serial calls give the result.  (The device's record
 * buffer holds cap_bytes + 4 (n_docs + cap_blobs) bytes, or what an earlier summary left if that is more; when the
 * cache holds so much that the records outgrow it although the new bytes fit, the call finishes with the serial calls
 * itself, and the next call's buffer holds a quarter more than those records; mtr_last_timing out[16] says which way
 * a call went.)
 * Fallback and refusals are mtr_replay_pipelined's: parts <= 1, ranges under MTR_PIPE_MIN_PART_DOCS documents and
 * batches mtr_submit_pipelined does not take run the serial calls inside, with the same result; a range with records
 * beyond remote ops gives MTR_ERR_UNSUPPORTED's error text (mtr_reset, then the serial calls).
 * mtr_last_timing out[13..16] describe the last call. */
int64_t mtr_replay_handover(mtr_engine* e, const mtr_batch* b, uint32_t parts, uint8_t* out, int64_t cap_bytes,
                            uint8_t* ids, uint8_t* state, int64_t* rep, int64_t* blob_off, int64_t cap_blobs,
                            int64_t* doc_first);

/* Git tree ids of the summary trees, hashed on the device (fluidframework_amd/csrc/tree_id.hip).  A tree's id is
 * SHA-1("tree <body length>\0" + body), the body being the entries sorted bytewise by name (a subtree comparing as its
 * name followed by '/') and concatenated, each "<mode in octal, no leading zero> <name>\0" + its 20 id bytes: what
 * `git mktree` prints and what storage answers createGitTree with (SummaryTreeUploadManager.writeSummaryTreeCore,
 * summaryTreeUploadManager.ts: one createGitTree round trip per tree to learn this sha; an unchanged subtree is
 * referred to by it).  The object holds a subtree's mode as "40000". */
#define MTR_TREE_NAME_MAX 39
typedef struct mtr_tree_entry {   /* 64 bytes */
    uint8_t  id[20];
    uint32_t mode;                /* 0100644 blob, 040000 subtree */
    uint8_t  name_len;            /* 1..MTR_TREE_NAME_MAX */
    char     name[MTR_TREE_NAME_MAX];
} mtr_tree_entry;

/* The id of the tree Client.summarize returns for every document of [lo, hi): its blobs under the names `header`,
 * `body_0`, `body_1`, ... (SnapshotV1; `header`, `body` in the legacy format) by their ids (mtr_summary_blob_ids),
 * merged with the host-made entries of that tree (the legacy catch-up blob, an interval collection's header, ...).
 * A SharedMatrix vector document (mtr_set_matrix) gives PermutationVector.summarize's tree
 * (permutationvector.ts:310-325): the subtree `segments` over all its blobs but the last, whose id is computed first,
 * and the blob `handleTable`, its last blob; the host-made entries join this outer tree.  A document without blobs
 * gives the tree of its host-made entries alone.
 * out: 20 bytes per document of [lo, hi).  extra (may be NULL) / extra_first[hi-lo+1]: host-made entries of document
 * lo+i's top tree, extra[extra_first[i], extra_first[i+1]) in any order.  Valid exactly where mtr_summary_blob_ids
 * is; computes the blob ids if no call has yet, and leaves the blob-id and delta caches as they are.  Returns hi-lo
 * (0 for an empty range), or -1 (mtr_last_error): bad range, no summary, a bad or duplicate name, one that repeats an
 * entry the engine makes (the message names the document and the entry); out is then untouched. */
int64_t mtr_summary_tree_ids(mtr_engine* e, uint32_t lo, uint32_t hi, const mtr_tree_entry* extra,
                             const int64_t* extra_first, uint8_t* out);
/* n host trees: tree i's entries are entries[first[i], first[i+1]) in any order; a tree without entries is the empty
 * tree (4b825dc6...).  For the levels above the document (channel, data store: writeSummaryTreeCore's recursion) and
 * for tests.  Returns MTR_OK, or -1 (mtr_last_error; the message names the tree and the entry). */
int mtr_git_tree_ids(mtr_engine* e, const mtr_tree_entry* entries, const int64_t* first, uint32_t n, uint8_t* out);

/* Local-view text of one document (UTF-16 units), gathered on the device
 * (MergeTreeTextHelper.getText, MergeTreeTextHelper.ts:20-81); returns the length (writes the text only
 * when it fits in cap units), -1 on error. */
int64_t mtr_get_text(mtr_engine* e, uint32_t doc, uint16_t* out, int64_t cap);

/* Local-view texts of documents [lo, hi) in one device gather and one download: doc_off[i] = first unit
 * of document lo + i in out, doc_off[hi - lo] = total.  Returns the total units (out NULL: a size query,
 * nothing written; doc_off filled either way), -1 when cap is too small or on error. */
int64_t mtr_get_texts(mtr_engine* e, uint32_t lo, uint32_t hi, uint16_t* out, int64_t cap, int64_t* doc_off);

/* Client.getContainingSegment(pos, {referenceSequenceNumber, clientId}) (client.ts:1065-1078 ->
 * mergeTree.ts:787-813): the segment holding position pos in the (ref_seq, client) view, found on the
 * device (one wave scans the document's visibility in that view).  client: a short id, -1
 * (LocalClientId) or -2 (NonCollabClient).  text (cap units, may be NULL) receives a text segment's
 * units.  Returns MTR_OK with info->leaf = -1 when no segment covers pos; then info->start is the view's length
 * (nodeLength(root) at that view: pos = INT32_MAX is a getLength query, SharedString.getLength for this client's own
 * view). */
typedef struct mtr_segment_info {
    int32_t leaf;        /* index of the leaf in tree order, -1 = none */
    int32_t offset;      /* pos - the segment's start in the view (getContainingSegment's offset) */
    int32_t length;      /* cachedLength */
    int32_t seq;         /* segment.seq */
    int32_t client;      /* segment.clientId: short id, -1 LocalClientId, -2 NonCollabClient */
    int32_t removed_seq; /* removedSeq; -1 = UnassignedSequenceNumber (a pending local remove) when removed,
                            else not removed (undefined) */
    int32_t marker;      /* 1 = Marker (text holds nothing; ref_type holds its refType) */
    int32_t ref_type;    /* marker refType / PermutationSegment start handle / text arena offset */
    int32_t props;       /* property-set index in the document's arena, -1 = none */
    int32_t start;       /* the segment's position in the view */
    int32_t removed;     /* 1 = the segment carries removal info (acked or pending) */
    int32_t local_seq;   /* localSeq of a pending local insert (then seq = -1), else -1 */
    int32_t local_removed_seq; /* localSeq of a pending local remove (then removed_seq = -1), else -1 */
    int32_t groups;      /* segmentGroups.size: the pending local ops the segment belongs to */
} mtr_segment_info;
int mtr_get_containing_segment(mtr_engine* e, uint32_t doc, int32_t pos, int32_t ref_seq, int32_t client,
                               mtr_segment_info* info, uint16_t* text, int64_t text_cap);

/* mtr_get_containing_segment for n views at once, with the segments' text and properties: one launch (a workgroup per
 * query), one upload of the queries and at most four downloads, whatever n is.  The same query may repeat and the
 * queries may name documents in any order.
 *   info[i]      what mtr_get_containing_segment(e, q[i].doc, q[i].pos, q[i].ref_seq, q[i].client, &info[i], ...)
 *                writes (leaf = -1 with start = the view's length included).
 *   text_off     [n + 1] offsets into text: text[text_off[i] .. text_off[i + 1]) are the units the single call writes
 *                into a large enough buffer (none for no segment, a marker, a matrix vector document).
 *   props_off    [n + 1] offsets into props: props[props_off[i] .. props_off[i + 1]) are the words
 *                mtr_get_props(e, q[i].doc, info[i].props, ...) returns, [n, key id, value id, ...] (none when
 *                info[i].props == -1 or there is no segment).
 * A document that is a matrix vector (mtr_set_matrix) has neither: its segments hold no text, and info[i].props is
 * there a tracking id and no property-set reference, so both of its ranges are empty.
 * text == NULL or props == NULL makes that half a size query (its offsets are filled, no units or words written); a NULL
 * text_off or props_off skips that half entirely.  Returns n; MTR_SUMMARY_TOO_SMALL when a non-NULL text or props has a
 * cap below its offsets' total (info and both offset arrays are written in full, no units or words); -1
 * (mtr_last_error) on a bad argument: a query whose doc >= max_docs is named by its index, and nothing is written.
 * -1 with nothing written as well when, in a half that was asked for, a segment's text or its property set does not
 * lie inside the document's arena (mtr_get_props' check; a corrupted document: the batch gathers on the device, where
 * such a reference must not be followed).  A half that is skipped is not checked.
 * n = 0 returns 0 with text_off[0] = props_off[0] = 0 and no device work.  The call only reads document state. */
typedef struct mtr_view_query {
    uint32_t doc;
    int32_t pos;     /* INT32_MAX: a getLength query (info[i].start = the view's length) */
    int32_t ref_seq;
    int32_t client;  /* a short id, -1 (LocalClientId) or -2 (NonCollabClient) */
} mtr_view_query;
int64_t mtr_get_containing_segments(mtr_engine* e, const mtr_view_query* q, uint32_t n, mtr_segment_info* info,
                                    uint16_t* text, int64_t text_cap, int64_t* text_off, uint32_t* props,
                                    int64_t props_cap, int64_t* props_off);

/* The segments, the text and the properties of n ranges [start, end), each at its own (ref_seq, client) view, in one
 * call: Client.walkSegments(handler, start, end) and MergeTreeTextHelper.getText(refSeq, clientId, placeholder, start,
 * end) (MergeTreeTextHelper.ts:20-81) for many documents and views at once.  Two launches of one wave per query, one
 * upload of the queries and at most six downloads, whatever n and the ranges' lengths are.
 * The segments of query i are the steps k = 0, 1, ... of a walk by mtr_get_containing_segment over positions p_k:
 * p_0 = start; r_k = what mtr_get_containing_segment(e, doc, p_k, ref_seq, client, ...) writes; p_{k+1} = r_k.start +
 * r_k.length; the walk stops when r_k.leaf == -1 or p_k >= end.  K_i, the steps taken, is 0 for start == end, for a
 * start at or past the view's length and for a document that holds nothing.
 *   seg_first   [n + 1], required when n > 0: the exclusive scan of K_i, the total last.
 *   info        info[seg_first[i] + k] = r_k, field for field (offset is the clip at the range's start; leaf is the
 *               tree-order ordinal).  info_cap: the rows info holds.  NULL: no rows are written or downloaded.
 *   text_first  [n + 1] offsets into text: text[text_first[i] .. text_first[i + 1]) is getText(refSeq, clientId,
 *               placeholder, start, end) of query i.
 *   text_off    [total + 1] offsets into text per segment: a text segment's units inside [start, end), clipped at both
 *               ends; for a marker one `placeholder` unit when placeholder != 0, else none; none in a matrix vector.
 *   props_off   [total + 1] offsets into props per segment: the words mtr_get_props(e, doc, info.props, ...) returns
 *               (none for props == -1 and in a matrix vector, as in mtr_get_containing_segments).
 * Each part can be skipped: info == NULL; text_first and text_off both NULL (either alone may be NULL: the other is
 * still filled); props_off NULL.  A part that is skipped is neither measured nor checked.  text == NULL or props ==
 * NULL with the part's offsets given is a size query.  total is the call's return value, so a first call with
 * seg_first (and text_first) alone sizes info, text_off, props_off and text.
 * Returns the total segment count.  MTR_SUMMARY_TOO_SMALL when a non-NULL info, text or props has a cap below its
 * total: every offset array given is written in full, no rows, units or words.  -1 (mtr_last_error) with nothing
 * written: a missing q or seg_first; a query with doc >= max_docs, start < 0 or end < start (named by its index); in a
 * part that was asked for, a segment whose text or property set does not lie inside the document's arena (checked on
 * the device, as mtr_get_containing_segments checks).  n = 0 returns 0, writes the [0] entry of every offset array
 * given and does no device work.  The call only reads document state: the cached summary, id, delta and novel results
 * stay. */
typedef struct mtr_range_query {
    uint32_t doc;
    int32_t start;    /* >= 0 */
    int32_t end;      /* >= start; INT32_MAX = the view's end */
    int32_t ref_seq;
    int32_t client;   /* a short id, -1 (LocalClientId) or -2 (NonCollabClient) */
} mtr_range_query;
int64_t mtr_get_range_segments(mtr_engine* e, const mtr_range_query* q, uint32_t n, uint16_t placeholder,
                               int64_t* seg_first, mtr_segment_info* info, int64_t info_cap,
                               uint16_t* text, int64_t text_cap, int64_t* text_first, int64_t* text_off,
                               uint32_t* props, int64_t props_cap, int64_t* props_off);

/* Positions mapped from one view of a document into another, n at once: Client.resolveRemoteClientPosition(remotePos,
 * remoteRefSeq, remoteClientId) (getContainingSegment at the remote view, then getPosition(segment) + offset at the
 * target view) and Client.getPosition(segment) for many (document, view) pairs.  One launch of one wave per query, one
 * upload of the queries, one download of the rows and one synchronisation, whatever n is.
 * With C(doc, p, rs, cl) what mtr_get_containing_segment writes, R(doc, rs, cl) the info rows of
 * mtr_get_range_segments for [0, INT32_MAX) at that view and len(doc, rs, cl) = C(doc, INT32_MAX, rs, cl).start:
 * P(L), the position of leaf ordinal L in the target view, is R[k].start for the smallest k with R[k].leaf >= L, and
 * the target view's len when there is no such row; the leaf is visible iff some row has leaf == L.
 *   MTR_POS_FROM_VIEW   r = C(doc, pos, ref_seq, client).  r.leaf >= 0: out = {P(r.leaf) + r.offset, r.leaf, r.offset,
 *                       FOUND | VISIBLE when the target view shows it} -- the offset is added even on a segment the
 *                       target view hides, as the reference adds it.  r.leaf == -1 and pos == r.start (pos is the
 *                       source view's length): {len(target), -1, 0, AT_END}.  Otherwise (a negative pos included):
 *                       {-1, -1, 0, 0}.
 *   MTR_POS_FROM_LEAF   L = pos, the source view is ignored.  0 <= L < the document's leaf count (mtr_export's):
 *                       {P(L) + offset, L, offset, FOUND | VISIBLE?}; otherwise {-1, -1, 0, 0}.
 * Queries may repeat and may name documents in any order; a matrix vector document is answered like any other.
 * Returns n.  -1 (mtr_last_error) with nothing written, the query named by its index: a missing q or out when n > 0, a
 * doc >= max_docs, a bad mode, a negative offset, a nonzero offset in FROM_VIEW mode.  n = 0 returns 0 with no device
 * work.  The call only reads document state: the cached summary, id, delta and novel results stay. */
#define MTR_POS_FROM_VIEW 0   /* pos is a position in the (ref_seq, client) view */
#define MTR_POS_FROM_LEAF 1   /* pos is a leaf's tree-order ordinal (mtr_segment_info.leaf); the source view is ignored */
typedef struct mtr_position_query {   /* 32 bytes */
    uint32_t doc;
    int32_t pos;
    int32_t ref_seq, client;          /* source view (client: short id, -1 LocalClientId, -2 NonCollabClient) */
    int32_t to_ref_seq, to_client;    /* target view, same spelling */
    int32_t mode;                     /* MTR_POS_FROM_VIEW / MTR_POS_FROM_LEAF */
    int32_t offset;                   /* FROM_LEAF: units into the segment, >= 0; FROM_VIEW: must be 0 */
} mtr_position_query;
#define MTR_POS_FOUND   1   /* a segment was found */
#define MTR_POS_VISIBLE 2   /* ... and the target view shows it */
#define MTR_POS_AT_END  4   /* no segment, and pos was the source view's length: pos = the target view's length */
typedef struct mtr_position {         /* 16 bytes */
    int32_t pos;      /* position in the target view, -1 = undefined */
    int32_t leaf;     /* the segment's ordinal, -1 = none */
    int32_t offset;   /* units into it */
    int32_t flags;
} mtr_position;
int64_t mtr_transform_positions(mtr_engine* e, const mtr_position_query* q, uint32_t n, mtr_position* out);

/* Local references (MTR_OP_REF_CREATE / MTR_OP_REF_REMOVE records, localReference.ts): out[r] =
 * Client.localReferencePositionToPosition of reference r (client.ts:398-403 -> mergeTree.ts:1046-1062),
 * MTR_DETACHED_POSITION (-1) when it has no position.  Returns the document's reference count (out written
 * only when it fits in cap), -1 on error. */
int64_t mtr_get_ref_positions(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap);
/* Every local reference of document doc as out[2r] = its position (as mtr_get_ref_positions) and out[2r+1] = state
 * bits: MTR_REF_ST_SEGMENT (LocalReference.getSegment() is defined, localReference.ts:106), MTR_REF_ST_HELD (that
 * segment's LocalReferenceCollection holds it, :357-384), MTR_REF_ST_REMOVED (that segment is in the tree and
 * removed).  An interval collection's compare (compareReferencePositions, referencePositions.ts:113-121) agrees
 * with the position order exactly when every endpoint is held by a live segment or has no segment at all
 * (DESIGN.md section 9).  Returns the reference count (out written only when 2*count fits in cap), -1 on error. */
int64_t mtr_get_ref_states(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap);
/* Every local reference of document doc as four int32: its position and state bits (as mtr_get_ref_states), then
 * compareReferencePositions' key (referencePositions.ts:113-121): a leaf key increasing in tree order (the segment's
 * ordinal order; -1 = no segment, -2 = a segment zamboni took out of the tree, whose ordinal the engine no longer
 * knows) and LocalReference.getOffset (localReference.ts:110).  A live interval collection orders its intervals by it
 * (SequenceInterval.compare, sequence/src/intervalCollection.ts:505-539), including endpoints left on removed
 * segments.  Returns the reference count (out written only when 4*count fits in cap), -1 on error. */
int64_t mtr_get_ref_keys(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap);
/* The three calls above for n documents at once: one launch (a wave per 64 references of a document; a document
 * without references costs none), one upload of the list and at most two downloads, whatever n is.  mode is the
 * words per reference and selects the call: MTR_REFS_POSITIONS (localReferencePositionToPosition, client.ts:398-403 ->
 * mergeTree.ts:1046-1062), MTR_REFS_STATES (with the state bits, localReference.ts:106, :357-384), MTR_REFS_KEYS (with
 * compareReferencePositions' key and getOffset, referencePositions.ts:113-121, localReference.ts:110).
 *   docs       [n] documents in any order, repeats allowed; NULL = documents 0 .. n - 1.
 *   doc_first  [n + 1], required when n > 0: doc_first[i] = the index, counted in references, of listed document i's
 *              first reference; doc_first[n] = the total.
 *   out        out[mode * (doc_first[i] + r) ..] = the mode words of reference r of docs[i]: exactly what the single
 *              call of that mode writes for that document (none for a document that never created a reference, and
 *              none at all while the engine has no reference table).
 * Returns the total reference count.  out == NULL is a size query: doc_first is filled, nothing else written.
 * cap_words < mode * total: MTR_SUMMARY_TOO_SMALL, doc_first filled, no words written.  -1 (mtr_last_error) with
 * nothing written: a bad mode, a missing doc_first, a docs[i] >= max_docs (named by its index i), or a document whose
 * header claims more references than caps.ref_slots (a corrupted document: the device does not follow it).
 * n = 0 returns 0 with doc_first[0] = 0 (when given) and no device work.  The call only reads document state: the
 * cached summary, id, delta and novel results stay. */
#define MTR_REFS_POSITIONS 1   /* words per reference: what mtr_get_ref_positions writes */
#define MTR_REFS_STATES    2   /* ... mtr_get_ref_states */
#define MTR_REFS_KEYS      4   /* ... mtr_get_ref_keys */
int64_t mtr_get_refs(mtr_engine* e, const uint32_t* docs, uint32_t n, int32_t mode, int32_t* out, int64_t cap_words,
                     int64_t* doc_first);
/* IntervalCollection.findOverlappingIntervals, previousInterval and nextInterval (sequence/src/intervalCollection.ts:
 * 950-992) for n queries over many interval collections of many documents: a fixed number of launches and copies (one
 * upload, two downloads, two synchronisations), whatever n and the collections' sizes are.  The call creates no
 * reference and writes no record: it only reads document state, and the cached summary, id, delta and novel results stay.
 * Stated over the calls above.  K(r), the key of reference r of the set's document, from its MTR_REFS_KEYS words: (0, 0,
 * 0) when word 2 is -1 (no segment), else (1, word 2, word 3).  T(p), the key of position p of the document's local view
 * (the view MTR_REF_LOCALVIEW names): the key a MTR_REFTYPE_TRANSIENT reference created at p with MTR_REF_LOCALVIEW
 * would have -- (1, the slot of the leaf holding p, the units of that leaf ahead of p), and (0, 0, 0) when no segment
 * holds p (p < 0, p at or past the view's length).  Keys compare as tuples.
 *   MTR_IVQ_OVERLAP    the intervals k of the set with K(start ref) <= T(end) and K(end ref) >= T(start)
 *                      (SequenceInterval.overlaps), in ascending k; none when end < start or the set is empty.  The
 *                      host puts them into compare order from the returned keys (ties by id).
 *   MTR_IVQ_PREVIOUS   at most one hit: the interval with the greatest K(end ref) <= T(start) (the end tree's floor)
 *   MTR_IVQ_NEXT       at most one hit: the interval with the least K(end ref) >= T(start) (the end tree's ceil)
 *                      Among equal end keys the smallest k is returned, with MTR_IVQ_TIE set when more than one
 *                      interval of the set has that end key (the end tree keeps one node for them: the host decides).
 *   hit_first  [n + 1], required when n > 0: query i's hits are hits[hit_first[i] .. hit_first[i + 1]); hit_first[n] =
 *              the total.
 *   status     [n], required when n > 0: 0, or MTR_IVQ_UNLINKED when an endpoint of the query's set sits on a segment
 *              zamboni took out of the tree (word 2 is -2: it has no place in the order); the query then has no hits.
 * Returns the total number of hits.  hits == NULL is a size query: hit_first and status are filled.  hit_cap < total:
 * MTR_SUMMARY_TOO_SMALL, hit_first and status filled, no rows written.  -1 (mtr_last_error) with nothing written: a
 * missing array when n > 0; a set whose doc >= max_docs or whose intervals run past n_intervals (named "set i"); a
 * query whose set >= n_sets or whose mode is none of the three (named "query i"); a reference id the set's document
 * does not have (found on the device, named "set i, interval k"); a document whose header claims more references than
 * caps.ref_slots.  Sets and queries are checked in that order, also when n = 0; n = 0 then returns 0 with
 * hit_first[0] = 0 (when given) and no device work. */
#define MTR_IVQ_OVERLAP  0
#define MTR_IVQ_PREVIOUS 1
#define MTR_IVQ_NEXT     2
#define MTR_IVQ_TIE      1   /* mtr_interval_hit.flags */
#define MTR_IVQ_UNLINKED 1   /* status */
typedef struct mtr_interval_set {    /* one collection of one document */
    uint32_t doc;
    uint32_t first, count;           /* its intervals: refs[2*(first+k)], refs[2*(first+k)+1] = the start and end
                                        reference ids of interval k, k < count */
} mtr_interval_set;
typedef struct mtr_interval_query {  /* 16 bytes */
    uint32_t set;                    /* index into sets */
    int32_t start, end;              /* positions in the document's local view; PREVIOUS / NEXT use start only */
    int32_t mode;                    /* MTR_IVQ_OVERLAP / _PREVIOUS / _NEXT */
} mtr_interval_query;
typedef struct mtr_interval_hit {    /* 32 bytes */
    int32_t interval;                /* k, its index in its set */
    int32_t start_pos, end_pos;      /* localReferencePositionToPosition of its endpoints (word 0 of MTR_REFS_KEYS) */
    int32_t start_key, start_off, end_key, end_off;  /* words 2, 3 of MTR_REFS_KEYS of each endpoint */
    int32_t flags;                   /* MTR_IVQ_TIE for PREVIOUS / NEXT, else 0 */
} mtr_interval_hit;
int64_t mtr_query_intervals(mtr_engine* e, const mtr_interval_set* sets, uint32_t n_sets, const uint32_t* refs,
                            uint32_t n_intervals, const mtr_interval_query* q, uint32_t n, int64_t* hit_first,
                            int32_t* status, mtr_interval_hit* hits, int64_t hit_cap);

/* Marker search, n queries at once: SharedString.findTile(pos, label, preceding) (MergeTree.findTile(startPos, clientId,
 * tileLabel, preceding), mergeTree.ts:1091, which searches at the client's view for a marker whose referenceTileLabels
 * hold the label -- here the caller passes the view, the call hard-codes none) and SharedString.getMarkerFromId followed
 * by getPosition (MergeTree.idToSegment, mergeTree.ts:549,668).  One launch of one wave per query, one upload of the
 * labels, the values and the queries together, one download of the rows and one synchronisation, whatever n is.
 * Stated over the calls above.  R(doc, rs, cl) = the info rows of mtr_get_range_segments for [0, INT32_MAX) at that view,
 * W(doc, ref) = the words mtr_get_props returns ([n, k0, v0, ...]), len = C(doc, INT32_MAX, rs, cl).start.  A row matches
 * label l when row.marker == 1 and either labels[l].key == MTR_LABEL_ANY, or row.props != -1 and W(doc, row.props) holds
 * a pair (k, v) with k == labels[l].key and v one of vals[labels[l].first .. first + count) -- the ids of the values
 * that carry the label, which the host works out from its value table (any label-carrying key works the same way:
 * "referenceTileLabels", "referenceRangeLabels", ...).  MTR_PROPS_NEVER (bit 31 of a leaf's set index) is masked off as
 * mtr_get_props masks it.
 *   MTR_MK_PRECEDING   the matching row of R(doc, ref_seq, client) with the greatest start <= pos; pos == INT32_MAX: the
 *                      last matching marker of the view.
 *   MTR_MK_FOLLOWING   the matching row with the least start >= pos.
 *                      Both: a hit is {row.start, row.leaf, row.ref_type, row.props, row.seq, FOUND | VISIBLE} (a
 *                      marker is one unit long, so starts differ and the hit is unique); no such row -- a negative pos
 *                      for PRECEDING, a pos past len for FOLLOWING, an empty document, a matrix vector document --
 *                      gives {-1, -1, 0, -1, 0, 0}.
 *   MTR_MK_BY_ID       pos is a marker ordinal (payload2 - 1 of the marker's insert / load record), label is unused.
 *                      An ordinal never mapped, and one whose segment zamboni took out of the tree, give {-1, -1, 0, -1,
 *                      0, 0}.  Otherwise, with L the marker's leaf ordinal: {P(L), L, ref_type, props, seq, FOUND |
 *                      VISIBLE?}, P(L) and "visible" as mtr_transform_positions defines them for MTR_POS_FROM_LEAF
 *                      into the (ref_seq, client) view; ref_type, props and seq as mtr_segment_info reports them.
 * Queries may repeat and may name documents in any order.
 * Returns n.  -1 (mtr_last_error) with nothing written, the offender named by its index ("label j", "query i"): a label
 * whose first + count > n_vals or whose values do not ascend strictly; a missing q or out when n > 0, missing labels
 * or vals when their counts are not 0; a doc >= max_docs; a bad mode; a label >= n_labels in a query that is not
 * BY_ID; a marker whose property reference lies outside the document's property arena (a corrupted document, found on
 * the device).  Labels are checked first, also when n = 0; n = 0 then returns 0 with no device work.  The call only
 * reads document state: the cached summary, id, delta and novel results stay. */
#define MTR_MK_PRECEDING 0   /* the last matching marker that starts at or before pos in the view  */
#define MTR_MK_FOLLOWING 1   /* the first matching marker that starts at or after pos in the view  */
#define MTR_MK_BY_ID     2   /* the marker mapped to ordinal `pos` (MergeTree.idToSegment); label unused */
#define MTR_MK_FOUND   1
#define MTR_MK_VISIBLE 2     /* BY_ID only: the view shows the marker (always set on a PRECEDING/FOLLOWING hit) */
#define MTR_LABEL_ANY  0xffffffffu   /* mtr_marker_label.key: every marker matches */
typedef struct mtr_marker_label {    /* 12 bytes */
    uint32_t key;                    /* property key id (e.g. the interned "referenceTileLabels"), or MTR_LABEL_ANY */
    uint32_t first, count;           /* vals[first .. first+count): value ids, ascending, that carry the label */
} mtr_marker_label;
typedef struct mtr_marker_query {    /* 24 bytes */
    uint32_t doc;
    int32_t pos;                     /* view position; BY_ID: the marker ordinal (payload2 - 1 of its insert/load record) */
    int32_t ref_seq, client;         /* the view; client: short id, -1 LocalClientId, -2 NonCollabClient */
    int32_t mode;
    uint32_t label;                  /* index into labels (ignored by BY_ID) */
} mtr_marker_query;
typedef struct mtr_marker_hit {      /* 24 bytes */
    int32_t pos;                     /* the marker's position in the view, -1 = none */
    int32_t leaf;                    /* its tree-order ordinal (mtr_segment_info.leaf), -1 = none */
    int32_t ref_type;                /* mtr_segment_info.ref_type */
    int32_t props;                   /* mtr_segment_info.props */
    int32_t seq;                     /* mtr_segment_info.seq */
    int32_t flags;
} mtr_marker_hit;
int64_t mtr_find_markers(mtr_engine* e, const mtr_marker_label* labels, uint32_t n_labels, const uint32_t* vals,
                         uint32_t n_vals, const mtr_marker_query* q, uint32_t n, mtr_marker_hit* out);
/* The segments of a SharedMatrix vector document in tree order (walkAllSegments, mergeTreeNodeWalk.ts:170), five
 * int32 each: cachedLength, 1 when removed (the local view does not show it, localNetLength, mergeTree.ts:613-634),
 * PermutationSegment.start (permutationvector.ts:53-72; MTR_HANDLE_UNALLOCATED), tracking id (-1: none) and its
 * group bits (include/mtr_types.h "Tracking groups").  The SharedMatrix undo host reads getPosition,
 * handleToPosition and the column handles from it (undoprovider.ts:138-170, matrix.ts:371-430).  Returns the
 * segment count (out written only when it fits in cap segments), -1 on error. */
int64_t mtr_get_leaves(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap);
/* Reference `id` of document doc: out[0] = index (tree order) of the leaf of its segment (LocalReference.
 * getSegment, localReference.ts:106; -1 = none, or the segment is no longer in the tree), out[1] = getOffset,
 * out[2] = refType, out[3] = 1 when the segment's LocalReferenceCollection holds it (has(), :357-384).
 * Returns out[0], or -2 on error. */
int32_t mtr_get_ref_info(mtr_engine* e, uint32_t doc, uint32_t id, int32_t* out);

/* MergeTree.pendingSegments.length (mergeTree.ts:1324-1357, asserted by client.applyMsg.spec.ts): the
 * SegmentGroups of this client's local ops that no sequenced message has acked yet; -1 = bad document. */
int32_t mtr_pending_groups(mtr_engine* e, uint32_t doc);

/* Per-document status: MTR_OK or an MTR_ERR_* code; *op_index = op that failed (or -1). */
int mtr_doc_status(mtr_engine* e, uint32_t doc, int32_t* op_index);

/* Leaf records of one document in the oracle's export format (8 int32 per leaf:
 * len, seq, client, removed_seq|INT32_MIN, n_removers, bnd, is_marker, props_hash).
 * Returns #leaves or -(needed); *height = tree height. */
int64_t mtr_export(mtr_engine* e, uint32_t doc, int32_t* out, int64_t cap_leaves, int32_t* height);

/* Engine-wide counters: out[0]=ops applied, out[1]=docs, out[2]=max leaves in any doc,
 * out[3]=sum of leaves, out[4]=docs with non-OK status, out[5]=kernel launches of the last run,
 * out[6]=max heap entries, out[7]=max text units used, out[8]=sum over applied ops of the leaf count
 * before the op, out[9]=UTF-16 units inserted.  Counters accumulate from mtr_reset. */
int mtr_stats(mtr_engine* e, int64_t* out, int32_t n);

/* Device time (ms) of the last mtr_run / mtr_summarize measured with HIP events: out[0]=apply
 * (wall, engine stream), out[1]=summarize, out[2]=apply kernel launches, out[3]=sum of the apply
 * launches' own durations (a round's size-class launches overlap on up to 4 streams), out[4]=the last blob-id
 * computation (mtr_summary_blob_ids: table kernels + id kernel), out[5]=the last delta build (mtr_summary_delta:
 * flag + scan + gather kernels), out[6]=the gather kernel's part of out[5], out[7]=the last tree-id computation
 * (mtr_summary_tree_ids / mtr_git_tree_ids: size, scan, write and id kernels, both levels), out[8]=the last novel
 * build (mtr_summary_novel: classify + state, scan and gather kernels), out[9]=the gather kernel's part of out[8],
 * out[10]=the classify and state kernels' part of out[8], out[11]=the last mtr_blob_cache_trim / _trim_to of a cache
 * with entries (keep flags, scan, compaction and slot rebuild; the read-back of the kept count lies outside the events),
 * out[12]=the last age histogram (mtr_blob_cache_ages, or the one mtr_blob_cache_trim_to takes), out[13]=the bytes
 * of blob content the last mtr_replay_handover copied to the host (a count, exact), out[14]=the summed device time of
 * its per-range id passes (blob offsets + id kernel), out[15]=the summed device time of its per-range classify + state,
 * scan and gather passes (0 for both when the call took the serial calls: out[4] and out[8] then hold their times),
 * out[16]=1 when the last mtr_replay_handover ran its ranges, 0 when it took the serial calls inside. */
int mtr_last_timing(mtr_engine* e, double* out, int32_t n);

/* Record mode (synthetic workloads, include/mtr_synth.h): draw cfg->n_docs documents' op logs
 * with the engine's own exact view lengths, apply them, and keep the recorded batch on the device
 * (mtr_reset + mtr_run then replays it).  `tables` supplies prop-op/key/value/client tables. */
struct mtr_synth_cfg;
int mtr_generate(mtr_engine* e, const struct mtr_synth_cfg* cfg, const mtr_batch* tables);

/* Record mode with pre-grown documents (config C5): every document first loads `grow`
 * two-unit snapshot header segments (MTR_OP_LOAD records, reloadFromSegments) and starts
 * collaboration, then draws cfg->ops_per_doc messages as mtr_generate does; per document
 * grow + 1 + ops_per_doc records and cfg->text_cap >= 2 * grow + the messages' text.  Draws the same
 * logs as the oracle's oracle_generate_grown from the same seeds. */
int mtr_generate_grown(mtr_engine* e, const struct mtr_synth_cfg* cfg, const mtr_batch* tables, uint32_t grow);

/* Record mode for SharedMatrix workloads: cfg->n_docs matrices drawn from the
 * matrix recipe (mtr_synth_matrix_finish) with the engine's exact view lengths of both vectors.
 * Matrix m is the pair (rows = engine document 2m, cols = 2m + 1; paired as by mtr_set_matrix) and
 * its op list is the rows document's; the engine needs max_docs >= 2 * n_docs.  Draws the same logs
 * as the oracle's oracle_generate_matrix from the same seeds. */
int mtr_generate_matrix(mtr_engine* e, const struct mtr_synth_cfg* cfg, const mtr_batch* tables);

/* Copy the recorded batch of documents [lo, hi) to the host (compacted: op_begin/text_base are
 * rewritten relative to the copied arrays; text_cap = capacity of `text` in UTF-16 units). */
int mtr_download_batch(mtr_engine* e, uint32_t lo, uint32_t hi, mtr_doc_desc* docs, mtr_op* ops, uint16_t* text,
                       uint64_t text_cap);

/* Apply-kernel phase timers (thread-0 clock cycles summed over documents; see apply.hip.h P_*).
 * Only a -DMTR_PROF build collects them; otherwise returns MTR_ERR_UNSUPPORTED and zeros. */
int mtr_profile(mtr_engine* e, uint64_t* out, int32_t n, int32_t reset);

/* Debug: copy the scan arrays (E = inclusive visible-length prefix, V = visible length per leaf) that
 * the last op of HBM-resident document `doc` computed: out[0..n) = E, out[n..2n) = V.  Returns n or -1. */
int64_t mtr_debug_scan(mtr_engine* e, uint32_t doc, int32_t* out, int64_t n);

/* Debug: the bytes of device and page-locked host memory that the engines of this process hold now (every
 * engine-owned buffer; mtr_host_alloc blocks are the caller's and are not counted).  Back to its earlier value once
 * an engine is destroyed, or a create has failed: what a test of the engine's ownership watches. */
int64_t mtr_debug_live_bytes(void);

/* Debug: the launch census -- which apply kernels mtr_run (and record mode) launched on this engine since
 * mtr_engine_create or the last mtr_reset; host counters, no device work.  Writes the first n of 21 words and returns
 * 21 (-1: no engine or no buffer):
 *   out[0..16)  launches per runtime-layout instantiation: LDS_X, HBM_X, LDS_LEAN, HBM_LEAN, LDS_DL, HBM_DL, LDS_GN,
 *               HBM_GN, PAIR_LDS, PAIR_HBM, PAIR_LDS_DL, PAIR_HBM_DL, PAIR_LDS_GN, PAIR_HBM_GN, PAIR2_LDS, PAIR2_HBM
 *               (X: rare records compiled in, LEAN: without them, DL: delta reporting, GN: record mode, PAIR: matrix
 *               pairs; LDS / HBM: where the documents' leaves live during the launch)
 *   out[16]     launches of the fixed-capacity kernels (compile-time LDS layout, 64 to 1,536 leaves)
 *   out[17..19) the smallest and the largest leaf capacity launched (0: nothing launched yet)
 *   out[19]     HBM-resident launches (all of the HBM_* above)
 *   out[20]     the largest leaf capacity of an LDS-resident launch
 * What a test reads to know that it reached the kernel it was written for. */
int mtr_debug_launch_counts(mtr_engine* e, int64_t* out, int n);

/* Human-readable description of the last engine-level error (static storage). */
const char* mtr_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MTR_H */
