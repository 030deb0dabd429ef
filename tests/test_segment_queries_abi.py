"""The batched position query's C ABI against its Python binding (no GPU calls): mtr_view_query is 16 bytes with the
header's field order, and the ctypes signature engine.lib() declares for mtr_get_containing_segments is the header's."""
import ctypes as C
import os
import re

import numpy as np

from fluidframework_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C parameter type -> what the binding passes it as (every pointer travels as an address)
CTYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int}
NUMPY = {"uint32_t": "<u4", "int32_t": "<i4"}


def _header():
    src = open(os.path.join(ROOT, "include", "mtr.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _ctype(decl):
    decl = decl.replace("const", "").strip()
    if "*" in decl:
        return C.c_void_p
    return CTYPES[decl.split()[0]]


def test_view_query_is_16_bytes_in_header_order():
    m = re.search(r"typedef struct mtr_view_query \{(.*?)\} mtr_view_query;", _header(), re.S)
    assert m, "include/mtr.h declares no mtr_view_query"
    fields = [f.split() for f in m.group(1).split(";") if f.strip()]
    want = np.dtype([(name, NUMPY[ty]) for ty, name in fields])
    assert want.itemsize == 16
    assert abi.VIEW_QUERY_DTYPE == want
    assert [abi.VIEW_QUERY_DTYPE.fields[n][1] for n in ("doc", "pos", "ref_seq", "client")] == [0, 4, 8, 12]


def test_ctypes_signature_matches_the_header():
    m = re.search(r"(\w+)\s+mtr_get_containing_segments\s*\((.*?)\);", _header(), re.S)
    assert m, "include/mtr.h declares no mtr_get_containing_segments"
    res, args = abi.SEGMENT_QUERY_SIGNATURES["mtr_get_containing_segments"]
    assert res is CTYPES[m.group(1)]
    assert args == [_ctype(p) for p in m.group(2).split(",")]
    assert len(args) == 10


def test_library_exports_the_call_with_that_signature():
    from fluidframework_amd.engine import lib

    fn = lib().mtr_get_containing_segments
    res, args = abi.SEGMENT_QUERY_SIGNATURES["mtr_get_containing_segments"]
    assert fn.restype is res and list(fn.argtypes) == args
