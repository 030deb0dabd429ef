"""The git blob id: the name Fluid's git storage (gitrest / historian) knows a blob by.

``git_blob_id(data)`` is SHA-1 over ``b"blob <len>\\0"`` followed by the bytes -- what ``git hash-object`` prints and
what gitHashFile (@fluidframework/common-utils) returns.  This is the host definition; the engine computes the same
ids on the device (Engine.blob_ids / Engine.git_blob_ids, fluidframework_amd/csrc/blob_id.hip).
"""
from __future__ import annotations

import hashlib

BLOB_ID_BYTES = 20  # include/mtr.h: MTR_BLOB_ID_BYTES


def git_blob_id(data: bytes) -> str:
    """40 lowercase hex digits."""
    view = memoryview(data)
    h = hashlib.sha1(b"blob %d\0" % view.nbytes)
    h.update(view)
    return h.hexdigest()


def summary_delta(baseline, blobs):
    """The host definition of the incremental hand-over (Engine.summary_delta computes it on the device).

    ``baseline``: per document a list of hex ids, or None for no baseline; ``blobs``: per document a list of bytes.
    Returns per document a list of ``(id, bytes_or_None)``: None where the baseline holds the same id at the same
    (document, index), the blob's bytes where the document or the index is new or the id differs.  Ids the baseline
    holds beyond a document's blobs, or for documents beyond ``blobs``, are not reported."""
    out = []
    for d, doc in enumerate(blobs):
        base = baseline[d] if baseline is not None and d < len(baseline) else []
        row = []
        for k, b in enumerate(doc):
            i = git_blob_id(b)
            row.append((i, None if k < len(base) and base[k] == i else bytes(b)))
        out.append(row)
    return out


NOVEL_HELD, NOVEL_FIRST, NOVEL_REPEAT = 0, 1, 2  # include/mtr.h: mtr_summary_novel's state[k]


def summary_novel(cache, blobs):
    """The host definition of the hand-over against the blob-id cache (Engine.summary_novel computes it on the device).

    ``cache``: a set (any container) of hex ids storage holds, or None; ``blobs``: per document a list of bytes.
    Returns per document a list of ``(id, state, rep, bytes_or_None)``.  ``state`` is NOVEL_HELD (0) when the cache
    holds the id, NOVEL_FIRST (1) when it does not and this is the first blob of the summary, in record order over all
    documents, with that id -- the copy to upload, the only state with bytes -- and NOVEL_REPEAT (2) when an earlier
    blob of the summary has the same id.  ``rep`` is the summary-wide index of that first blob (the blob's own index
    for state 1, -1 for state 0).  This is SummaryTreeUploadManager.writeSummaryBlob's rule: upload a blob unless
    blobsShaCache holds its sha, under any path of any document."""
    held = frozenset(cache) if cache is not None else frozenset()
    first, out, index = {}, [], 0
    for doc in blobs:
        row = []
        for b in doc:
            i = git_blob_id(b)
            if i in held:
                row.append((i, NOVEL_HELD, -1, None))
            elif i in first:
                row.append((i, NOVEL_REPEAT, first[i], None))
            else:
                first[i] = index
                row.append((i, NOVEL_FIRST, index, bytes(b)))
            index += 1
        out.append(row)
    return out


CACHE_AGE_BUCKETS = 1024  # include/mtr.h: mtr_blob_cache_ages' largest n
CACHE_GENERATION_MAX = 2**32 - 1


class BlobCacheModel:
    """The host definition of the blob-id cache's life cycle (the engine's mtr_blob_cache_* calls are tested against
    it): an insertion-ordered map from hex id to stamp, the generation at which the id was last offered, and a
    ``generation`` that starts at 0 and counts the acknowledged summaries."""

    def __init__(self):
        self.stamps = {}  # hex id -> stamp, in table order
        self.generation = 0

    def _offer(self, i, stamp):
        self.stamps[i] = max(self.stamps.get(i, 0), stamp)  # (an unknown id is appended)

    def add(self, ids):
        """mtr_blob_cache_add: unknown ids are appended in the order of their first occurrence; every offered id,
        held or new, is stamped with the generation."""
        for i in ids:
            self._offer(i, self.generation)

    def add_summary(self, ids_in_record_order):
        """mtr_blob_cache_add_summary: the next generation, then ``add`` -- a blob the summary refers to counts as
        used whether or not it was uploaded."""
        if self.generation >= CACHE_GENERATION_MAX:
            raise ValueError("the cache is at generation 2^32 - 1")
        self.generation += 1
        self.add(ids_in_record_order)

    def ages(self, n):
        """out[a] = the entries with generation - stamp == a for a < n - 1; out[n - 1] = all older ones."""
        if not 1 <= n <= CACHE_AGE_BUCKETS:
            raise ValueError(f"n = {n} is outside 1..{CACHE_AGE_BUCKETS}")
        out = [0] * n
        for s in self.stamps.values():
            out[min(self.generation - s, n - 1)] += 1
        return out

    def trim(self, min_generation):
        """Removes the entries with stamp < min_generation; the survivors keep their order.  Returns the number
        removed."""
        before = len(self.stamps)
        self.stamps = {i: s for i, s in self.stamps.items() if s >= min_generation}
        return before - len(self.stamps)

    def trim_to(self, max_entries):
        """``trim`` at the smallest g of [0, generation + 1] that keeps at most max_entries entries: whole
        generations go, oldest first."""
        if max_entries < 0:
            raise ValueError("max_entries is negative")
        by_stamp = {}
        for s in self.stamps.values():
            by_stamp[s] = by_stamp.get(s, 0) + 1
        g, kept = 0, 0
        for s in sorted(by_stamp, reverse=True):  # youngest first
            if kept + by_stamp[s] > max_entries:
                g = s + 1  # (generation s does not fit, so it and everything older goes)
                break
            kept += by_stamp[s]
        return self.trim(g)

    def export(self):
        """(ids in table order, their ages)."""
        return list(self.stamps), [self.generation - s for s in self.stamps.values()]

    def import_(self, ids, ages):
        """mtr_blob_cache_import: the generation rises to the largest age, then each id is offered with stamp
        generation - age; of equal ids the youngest age wins."""
        ids, ages = list(ids), [int(a) for a in ages]
        if len(ids) != len(ages):
            raise ValueError(f"{len(ids)} ids but {len(ages)} ages")
        self.generation = max(self.generation, max(ages, default=0))
        for i, a in zip(ids, ages):
            self._offer(i, self.generation - a)

    def clear(self):
        self.stamps = {}
        self.generation = 0

    def has(self, ids):
        return [i in self.stamps for i in ids]

    def size(self):
        return len(self.stamps)

    def ids(self):
        return list(self.stamps)


MODE_BLOB = 0o100644
MODE_TREE = 0o40000
TREE_NAME_MAX = 39  # include/mtr.h: MTR_TREE_NAME_MAX (the device interface's limit, not git's)


def git_tree_id(entries) -> str:
    """The id of the git tree with these ``(mode, name, id_hex)`` entries, given in any order.

    The body is the entries sorted bytewise by name, a subtree comparing as its name followed by ``/``, each
    ``b"<mode in octal, no leading zero> <name>\\0"`` + the 20 raw id bytes; the id is SHA-1 over
    ``b"tree <body length>\\0"`` + body -- what ``git mktree`` prints and what storage answers createGitTree with
    (SummaryTreeUploadManager.writeSummaryTreeCore).  ``mode`` is MODE_BLOB (0o100644) or MODE_TREE (0o40000: the
    object holds ``40000``, although FileMode.Directory and ``git mktree``'s input write ``040000``).  Names are str
    (encoded as UTF-8) or bytes.  Raises ValueError on an empty name, a name holding NUL or ``/``, a name given twice
    and an unknown mode.  The engine computes the same ids on the device (Engine.tree_ids / Engine.git_tree_ids,
    fluidframework_amd/csrc/tree_id.hip)."""
    rows, seen = [], set()
    for mode, name, id_hex in entries:
        raw = name.encode() if isinstance(name, str) else bytes(name)
        if mode not in (MODE_BLOB, MODE_TREE):
            raise ValueError(f"tree entry {raw!r}: mode {mode:o} is neither 100644 nor 40000")
        if not raw:
            raise ValueError("tree entry with an empty name")
        if b"\0" in raw or b"/" in raw:
            raise ValueError(f"tree entry {raw!r}: the name holds a NUL or a '/'")
        if raw in seen:
            raise ValueError(f"tree entry {raw!r}: the name appears twice")
        seen.add(raw)
        oid = bytes.fromhex(id_hex)
        if len(oid) != BLOB_ID_BYTES:
            raise ValueError(f"tree entry {raw!r}: the id is not 40 hex digits")
        rows.append((raw + b"/" if mode == MODE_TREE else raw, b"%o %s\0" % (mode, raw) + oid))
    body = b"".join(r[1] for r in sorted(rows))
    return hashlib.sha1(b"tree %d\0" % len(body) + body).hexdigest()


def summary_tree_id(blobs, v1, extras=(), matrix=False) -> str:
    """The id of the tree Client.summarize returns for a document whose engine blobs are ``blobs`` (bytes, in record
    order): ``header``, ``body_0``, ``body_1``, ... (SnapshotV1) or ``header``, ``body`` (legacy), merged with
    ``extras``, the host-made ``(mode, name, id_hex)`` entries of that tree (``catchupOps``, an interval collection's
    header, ...).  ``matrix``: PermutationVector.summarize's tree of a SharedMatrix vector document
    (permutationvector.ts:310-325): the subtree ``segments`` over all blobs but the last and the blob ``handleTable``,
    the last; the extras join this outer tree.  A document without blobs gives the tree of its extras alone.
    Raises ValueError as git_tree_id does; an extra that repeats an engine name is a name given twice."""
    blobs = list(blobs)
    segs = blobs[:-1] if matrix else blobs
    if not v1 and len(segs) > 2:
        raise ValueError(f"{len(segs)} blobs, but the legacy format names two (header, body)")
    names = ["header"] + ([f"body_{k}" for k in range(len(segs) - 1)] if v1 else ["body"])
    inner = [(MODE_BLOB, n, git_blob_id(b)) for n, b in zip(names, segs)]
    if not matrix:
        return git_tree_id(inner + list(extras))
    if not blobs:
        return git_tree_id(list(extras))
    return git_tree_id([(MODE_TREE, "segments", git_tree_id(inner)), (MODE_BLOB, "handleTable", git_blob_id(blobs[-1]))]
                       + list(extras))
