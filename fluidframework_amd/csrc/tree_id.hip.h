// tree_id.hip.h -- git tree ids (SHA-1 of "tree <len>\0" + the sorted entries) of summary trees, hashed on the device.
// The kernels live in tree_id.hip; handover.hip drives them through tree_ids_launch (asynchronous on `s`).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mtr.h"

namespace mtr {

// One batch of n trees.  Tree t's entries are the engine-made ones of document t (named on the device) merged with
// the host-made ones x[x_first[t], x_first[t + 1]), which arrive sorted by git's rule and validated.
//   level 0: a document's own tree.  A SharedString document (kind 0): `header` and `body_k` (v1) or `body` (legacy)
//            over all its blobs, plus its extras.  A matrix vector document (kind != 0): the `segments` subtree over
//            all blobs but the last, no extras.  Every tree's id goes to out.
//   level 1: the outer tree of a matrix vector document: `handleTable` (its last blob), `segments` (out[t], level
//            0's result) and its extras; out[t] is replaced.  Other documents are left alone.
// first == nullptr: host trees, which hold nothing but their x entries.
struct TreeJob {
    uint32_t n;
    uint32_t level;
    uint32_t v1;
    const uint32_t* first;     // [n + 1] each document's first blob in blob_ids (the blob table's BlobIds::first + lo)
    const uint32_t* kind;      // [n] 0 SharedString, else a matrix vector; nullptr = all 0
    const uint32_t* blob_ids;  // five words per blob
    const uint32_t* x_first;   // [n + 1]; nullptr = no host-made entries
    const mtr_tree_entry* x;
    uint32_t* off;             // [n + 1] work: tree body sizes, then their offsets in body and the total
    uint8_t* body;             // the tree bodies back to back; 4-byte aligned, at least the total rounded up to 4
    uint32_t* out;             // [n] five words per tree
};

// An upper bound of a tree body's size from its entry counts (for sizing TreeJob::body before the device knows):
// an engine-made entry is at most "100644 body_4294967295\0" + 20 bytes.
constexpr uint64_t kTreeEngineEntryMax = 6 + 1 + 15 + 1 + 20;

// size pass, scan, write pass, hash: out holds the ids when `s` reaches the end of them
hipError_t tree_ids_launch(const TreeJob& job, hipStream_t s);

}  // namespace mtr
