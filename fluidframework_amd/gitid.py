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
