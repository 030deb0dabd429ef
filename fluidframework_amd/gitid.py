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
