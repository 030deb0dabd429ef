"""mtr_get_range_segments on every layer that names it, without a GPU: include/mtr.h, the ctypes table (abi.py), the
library's export, the Python hosts and the Node host and declaration agree."""
import ctypes as C
import os
import re

from fluidframework_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE_OF = {"mtr_engine*": C.c_void_p, "const mtr_range_query*": C.c_void_p, "uint32_t": C.c_uint32,
            "uint16_t": C.c_uint16, "int64_t": C.c_int64, "int64_t*": C.c_void_p, "mtr_segment_info*": C.c_void_p,
            "uint16_t*": C.c_void_p, "uint32_t*": C.c_void_p}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtr.h")).read(), flags=re.S)


def test_header_and_ctypes_table_agree():
    m = re.search(r"(\w+)\s+mtr_get_range_segments\s*\(([^)]*)\)\s*;", _header())
    assert m, "include/mtr.h does not declare mtr_get_range_segments"
    params = [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
    res, args = abi.RANGE_QUERY_SIGNATURES["mtr_get_range_segments"]
    assert CTYPE_OF[m.group(1)] is res
    assert [CTYPE_OF[p] for p in params] == args
    assert len(args) == 14


def test_query_struct_is_20_bytes_and_matches_the_dtype():
    m = re.search(r"typedef\s+struct\s+mtr_range_query\s*\{([^}]*)\}\s*mtr_range_query\s*;", _header())
    assert m, "include/mtr.h does not define mtr_range_query"
    fields = [tuple(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == [("uint32_t", "doc"), ("int32_t", "start"), ("int32_t", "end"), ("int32_t", "ref_seq"),
                      ("int32_t", "client")]
    kinds = {"uint32_t": "<u4", "int32_t": "<i4"}
    assert [(n, abi.RANGE_QUERY_DTYPE.fields[n][0].str, abi.RANGE_QUERY_DTYPE.fields[n][1]) for _, n in fields] == \
        [(n, kinds[t], 4 * k) for k, (t, n) in enumerate(fields)]
    assert abi.RANGE_QUERY_DTYPE.itemsize == 20  # sizeof(mtr_range_query): five 4-byte words, no padding


def test_library_exports_it_and_the_hosts_name_it():
    path = os.path.join(ROOT, "fluidframework_amd", "libmtr.so")
    if not os.path.exists(path):
        from fluidframework_amd import build
        build.build_engine()
    assert hasattr(C.CDLL(path), "mtr_get_range_segments")
    from fluidframework_amd import live
    from fluidframework_amd.engine import Engine
    for name in ("range_segments", "range_texts", "properties_at"):
        assert callable(getattr(Engine, name))
    assert callable(live.EngineExecutor.text_range) and callable(live.LiveSession.text_range)
    node = os.path.join(ROOT, "fluidframework_amd", "node")
    assert "mtr_get_range_segments(" in open(os.path.join(node, "mtr_napi.cc")).read()
    dts = open(os.path.join(node, "index.d.ts")).read()
    for name in ("getRangeSegments(", "getTextRanges(", "getText(start?: number, end?: number)"):
        assert name in dts, name
    js = open(os.path.join(node, "index.js")).read()
    assert "getRangeSegments(" in js and "getTextRanges(" in js
