"""mtr_get_refs on every layer that names it, without a GPU: include/mtr.h, the ctypes table (abi.py), the library's
export, the Python hosts and the Node declaration agree."""
import ctypes as C
import os
import re

from fluidframework_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE_OF = {"mtr_engine*": C.c_void_p, "const uint32_t*": C.c_void_p, "uint32_t": C.c_uint32, "int32_t": C.c_int32,
            "int32_t*": C.c_void_p, "int64_t": C.c_int64, "int64_t*": C.c_void_p}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtr.h")).read(), flags=re.S)


def test_header_and_ctypes_table_agree():
    m = re.search(r"(\w+)\s+mtr_get_refs\s*\(([^)]*)\)\s*;", _header())
    assert m, "include/mtr.h does not declare mtr_get_refs"
    params = [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
    res, args = abi.REF_QUERY_SIGNATURES["mtr_get_refs"]
    assert CTYPE_OF[m.group(1)] is res
    assert [CTYPE_OF[p] for p in params] == args


def test_mode_constants_agree():
    defs = dict(re.findall(r"#define\s+(MTR_REFS_\w+)\s+(\d+)", _header()))
    assert {k: int(v) for k, v in defs.items()} == {"MTR_REFS_POSITIONS": abi.REFS_POSITIONS,
                                                    "MTR_REFS_STATES": abi.REFS_STATES, "MTR_REFS_KEYS": abi.REFS_KEYS}
    assert (abi.REFS_POSITIONS, abi.REFS_STATES, abi.REFS_KEYS) == (1, 2, 4)  # the words per reference


def test_library_exports_it_and_the_hosts_name_it():
    path = os.path.join(ROOT, "fluidframework_amd", "libmtr.so")
    if not os.path.exists(path):
        from fluidframework_amd import build
        build.build_engine()
    assert hasattr(C.CDLL(path), "mtr_get_refs")
    from fluidframework_amd import live, sequence
    from fluidframework_amd.engine import Engine
    for name in ("refs_batch", "ref_positions_many", "ref_states_many", "ref_keys_many"):
        assert callable(getattr(Engine, name))
    assert callable(sequence.interval_headers) and callable(live.EngineExecutor.ref_keys_many)
    node = os.path.join(ROOT, "fluidframework_amd", "node")
    assert "mtr_get_refs(e, docs, n, mode" in open(os.path.join(node, "mtr_napi.cc")).read()
    assert "getRefsBatch(clients: BatchReplayClient[], mode: 1 | 2 | 4)" in open(os.path.join(node, "index.d.ts")).read()
