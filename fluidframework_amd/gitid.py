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
