"""ctypes binding of libmtr.so (include/mtr.h) and the observer-Client mirror.

The product path: a batch packed by :mod:`fluidframework_amd.batch` goes to the HIP engine through
the C ABI.  There is no CPU fallback -- if libmtr.so (gfx950 code object) cannot be loaded or no
HIP device is present, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi, gitid

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class EngineError(RuntimeError):
    pass


class MtrCaps(C.Structure):
    _fields_ = [
        ("max_segments", C.c_uint32),
        ("heap_entries", C.c_uint32),
        ("text_units", C.c_uint32),
        ("prop_words", C.c_uint32),
        ("remover_cells", C.c_uint32),
        ("ops_per_launch", C.c_uint32),
        ("ref_slots", C.c_uint32),
    ]


class SegmentInfo(C.Structure):
    """include/mtr.h: mtr_segment_info"""
    _fields_ = [(n, C.c_int32) for n in ("leaf", "offset", "length", "seq", "client", "removed_seq", "marker",
                                         "ref_type", "props", "start", "removed", "local_seq",
                                         "local_removed_seq", "groups")]


def lib():
    """Load libmtr.so (never falls back to anything else)."""
    global _LIB
    if _LIB is None:
        # MTR_LIB=libmtr_prof.so selects the phase-timer build (python -m fluidframework_amd.build --prof)
        path = os.path.join(_HERE, os.environ.get("MTR_LIB", "libmtr.so"))
        if not os.path.exists(path):
            raise EngineError(f"{path} missing: build it with `python -m fluidframework_amd.build`")
        L = C.CDLL(path)
        L.mtr_engine_create.restype = C.c_void_p
        L.mtr_engine_create.argtypes = [C.POINTER(abi.MtrOptions), C.c_int, C.c_uint32, C.POINTER(MtrCaps)]
        L.mtr_engine_destroy.argtypes = [C.c_void_p]
        for name in ("mtr_reset", "mtr_run", "mtr_summarize", "mtr_sync"):
            getattr(L, name).argtypes = [C.c_void_p]
            getattr(L, name).restype = C.c_int
        L.mtr_submit.argtypes = [C.c_void_p, C.c_void_p]
        L.mtr_submit.restype = C.c_int
        L.mtr_submit_pipelined.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.mtr_submit_pipelined.restype = C.c_int
        L.mtr_replay_pipelined.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p]
        L.mtr_replay_pipelined.restype = C.c_int64
        L.mtr_replay_handover.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.mtr_replay_handover.restype = C.c_int64
        L.mtr_get_summary.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]
        L.mtr_get_summary.restype = C.c_int64
        L.mtr_summary_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.mtr_summary_info.restype = C.c_int
        L.mtr_get_summaries.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p]
        L.mtr_get_summaries.restype = C.c_int64
        L.mtr_host_alloc.argtypes = [C.c_uint64]
        L.mtr_host_alloc.restype = C.c_void_p
        L.mtr_host_free.argtypes = [C.c_void_p]
        L.mtr_host_free.restype = C.c_int
        L.mtr_summary_hashes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.mtr_summary_hashes.restype = C.c_int
        L.mtr_summary_blob_ids.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p]
        L.mtr_summary_blob_ids.restype = C.c_int64
        L.mtr_git_blob_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.mtr_git_blob_ids.restype = C.c_int
        L.mtr_summary_tree_ids.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtr_summary_tree_ids.restype = C.c_int64
        L.mtr_git_tree_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.mtr_git_tree_ids.restype = C.c_int
        L.mtr_summary_set_baseline.argtypes = [C.c_void_p]
        L.mtr_summary_set_baseline.restype = C.c_int
        L.mtr_summary_set_baseline_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.mtr_summary_set_baseline_ids.restype = C.c_int
        L.mtr_summary_clear_baseline.argtypes = [C.c_void_p]
        L.mtr_summary_clear_baseline.restype = C.c_int
        L.mtr_summary_delta_info.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.mtr_summary_delta_info.restype = C.c_int
        L.mtr_summary_delta.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_void_p]
        L.mtr_summary_delta.restype = C.c_int64
        for name, (res, args) in abi.BLOB_CACHE_SIGNATURES.items():
            getattr(L, name).restype = res
            getattr(L, name).argtypes = args
        for name, (res, args) in (list(abi.SEGMENT_QUERY_SIGNATURES.items()) + list(abi.REF_QUERY_SIGNATURES.items()) +
                                  list(abi.RANGE_QUERY_SIGNATURES.items()) + list(abi.DELTA_QUERY_SIGNATURES.items()) +
                                  list(abi.POSITION_QUERY_SIGNATURES.items()) +
                                  list(abi.INTERVAL_QUERY_SIGNATURES.items()) +
                                  list(abi.MARKER_QUERY_SIGNATURES.items())):
            getattr(L, name).restype = res
            getattr(L, name).argtypes = args
        L.mtr_summary_bytes.argtypes = [C.c_void_p]
        L.mtr_summary_bytes.restype = C.c_int64
        L.mtr_get_text.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64]
        L.mtr_get_text.restype = C.c_int64
        L.mtr_get_texts.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p]
        L.mtr_get_texts.restype = C.c_int64
        L.mtr_get_containing_segment.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_int32,
                                                 C.POINTER(SegmentInfo), C.c_void_p, C.c_int64]
        L.mtr_get_containing_segment.restype = C.c_int
        L.mtr_doc_status.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)]
        L.mtr_pending_groups.argtypes = [C.c_void_p, C.c_uint32]
        L.mtr_pending_groups.restype = C.c_int32
        L.mtr_doc_status.restype = C.c_int
        L.mtr_export.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        L.mtr_export.restype = C.c_int64
        L.mtr_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.mtr_stats.restype = C.c_int
        L.mtr_set_matrix.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.mtr_set_matrix.restype = C.c_int
        L.mtr_get_deltas.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64]
        L.mtr_get_deltas.restype = C.c_int64
        L.mtr_get_props.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int64]
        L.mtr_get_props.restype = C.c_int64
        L.mtr_last_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.mtr_last_timing.restype = C.c_int
        L.mtr_last_error.restype = C.c_char_p
        L.mtr_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.mtr_profile.restype = C.c_int
        L.mtr_generate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtr_generate.restype = C.c_int
        L.mtr_generate_grown.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.mtr_generate_grown.restype = C.c_int
        L.mtr_generate_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mtr_generate_matrix.restype = C.c_int
        L.mtr_download_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_uint64]
        L.mtr_download_batch.restype = C.c_int
        L.mtr_get_ref_positions.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64]
        L.mtr_get_ref_positions.restype = C.c_int64
        L.mtr_get_ref_states.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64]
        L.mtr_get_ref_states.restype = C.c_int64
        L.mtr_get_ref_keys.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64]
        L.mtr_get_ref_keys.restype = C.c_int64
        L.mtr_get_leaves.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64]
        L.mtr_get_leaves.restype = C.c_int64
        L.mtr_get_ref_info.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.mtr_get_ref_info.restype = C.c_int32
        L.mtr_debug_live_bytes.argtypes = []
        L.mtr_debug_live_bytes.restype = C.c_int64
        L.mtr_debug_launch_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.mtr_debug_launch_counts.restype = C.c_int
        _LIB = L
    return _LIB


# include/mtr.h: mtr_tree_entry (64 bytes)
TREE_ENTRY = np.dtype([("id", "u1", 20), ("mode", "<u4"), ("name_len", "u1"), ("name", "S39")])
assert TREE_ENTRY.itemsize == 64


def pack_tree_entries(trees):
    """``trees``: per tree a list of ``(mode, name, id_hex)``.  Returns (entries, first): an mtr_tree_entry array and
    the i8 offsets of each tree's entries in it.  Raises ValueError on what the record cannot hold: a name longer
    than gitid.TREE_NAME_MAX bytes or empty, an id that is not 20 bytes.  (The engine checks the rest: modes, NUL and
    '/' in names, duplicates.)"""
    first = np.zeros(len(trees) + 1, dtype="<i8")
    np.cumsum([len(t) for t in trees], out=first[1:])
    x = np.zeros(max(int(first[-1]), 1), dtype=TREE_ENTRY)
    k = 0
    for t in trees:
        for mode, name, id_hex in t:
            raw = name.encode() if isinstance(name, str) else bytes(name)
            if not 1 <= len(raw) <= gitid.TREE_NAME_MAX:
                raise ValueError(f"tree entry {raw!r}: the name has {len(raw)} bytes, outside 1..{gitid.TREE_NAME_MAX}")
            oid = bytes.fromhex(id_hex)
            if len(oid) != gitid.BLOB_ID_BYTES:
                raise ValueError(f"tree entry {raw!r}: the id is not 40 hex digits")
            x[k] = (np.frombuffer(oid, dtype="u1"), mode, len(raw), raw)
            k += 1
    return x, first


def live_bytes() -> int:
    """mtr_debug_live_bytes: device and page-locked bytes the engines of this process hold now."""
    return int(lib().mtr_debug_live_bytes())


def _err() -> str:
    return (lib().mtr_last_error() or b"").decode(errors="replace")


class _Pinned:
    """Owner of one mtr_host_alloc block (freed when the last array view goes away)."""

    def __init__(self, nbytes):
        self.p = lib().mtr_host_alloc(max(int(nbytes), 1))
        if not self.p:
            raise EngineError(f"mtr_host_alloc failed: {_err()}")
        self.nbytes = max(int(nbytes), 1)

    def __del__(self):
        if getattr(self, "p", None):
            lib().mtr_host_free(self.p)
            self.p = None


def pinned(shape, dtype) -> np.ndarray:
    """A numpy array in page-locked host memory (mtr_host_alloc): op uploads and summary downloads
    from it run at full PCIe rate."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) if np.ndim(shape) else int(shape)
    owner = _Pinned(n * dt.itemsize)
    buf = (C.c_uint8 * owner.nbytes).from_address(owner.p)
    buf._owner = owner  # the array holds `buf`, `buf` holds the owner
    return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)


class Engine:
    """One engine = the observer Clients of up to ``max_docs`` documents on one GPU."""

    def __init__(self, max_docs, *, device=0, new_length_calc=False, snapshot_v1=True, chunk_size=10000,
                 max_segments=0, heap_entries=0, text_units=0, prop_words=0, remover_cells=0, ops_per_launch=0,
                 ref_slots=0):
        self.opts = abi.MtrOptions(int(new_length_calc), int(snapshot_v1), int(chunk_size), 0)
        self.caps = MtrCaps(max_segments, heap_entries, text_units, prop_words, remover_cells, ops_per_launch,
                            ref_slots)
        self.max_docs = int(max_docs)
        h = lib().mtr_engine_create(C.byref(self.opts), int(device), self.max_docs, C.byref(self.caps))
        if not h:
            raise EngineError(f"mtr_engine_create failed: {_err()}")
        self.h = h
        self._batch = None

    def close(self):
        if getattr(self, "h", None):
            lib().mtr_engine_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError(f"{what} failed ({rc}): {_err()}")

    def reset(self):
        self._check(lib().mtr_reset(self.h), "mtr_reset")

    def submit(self, batch):
        self._batch = batch  # keep host arrays alive until the copies completed
        self._check(lib().mtr_submit(self.h, C.addressof(batch.c)), "mtr_submit")

    def submit_pipelined(self, batch, parts=16):
        """mtr_submit_pipelined: the op records and text go over in `parts` document ranges on a copy stream and the
        next run() starts each range as soon as it has landed (remote-op batches; see include/mtr.h).  The batch's
        arrays should be page-locked (Engine.download(..., pinned_memory=True)) for the copies to overlap."""
        self._batch = batch
        self._check(lib().mtr_submit_pipelined(self.h, C.addressof(batch.c), int(parts)), "mtr_submit_pipelined")

    def replay_pipelined(self, batch, out, parts=16):
        """mtr_replay_pipelined: upload, apply, summarize and download every document's summary records into
        `out` (a u1 array, page-locked for the copies to overlap), pipelined over `parts` document ranges.
        Returns (out, doc_off) like summaries()."""
        self._batch = batch
        n = int(batch.c.n_docs)
        doc_off = np.zeros(n + 1, dtype="<i8")
        r = lib().mtr_replay_pipelined(self.h, C.addressof(batch.c), int(parts), out.ctypes.data, out.size,
                                       doc_off.ctypes.data)
        if r < 0:
            raise EngineError(f"mtr_replay_pipelined failed: {_err()}")
        return out, doc_off

    def replay_handover(self, batch, out, parts=16, cap_blobs=None):
        """mtr_replay_handover: replay_pipelined that downloads only the blobs storage lacks.  Upload, apply and
        summarize pipelined over `parts` document ranges; each range's blobs are hashed and sorted against the blob-id
        cache and the ranges before it on the device, and its first occurrences alone come over into `out` (a u1
        array, page-locked for the copies to overlap; its size bounds the new bytes).  `cap_blobs` bounds the
        summary's blobs (default: 16 a document).  Returns (out, state, rep, blob_off, doc_first, ids): the first
        five as summary_novel_raw() over all documents, ids [blobs, 20] u1 as blob_ids_raw().  The summary, its ids
        and its novel result stay on the device for the other hand-over calls."""
        self._batch = batch
        n = int(batch.c.n_docs)
        cap = max(1, 16 * n if cap_blobs is None else int(cap_blobs))
        ids = np.zeros((cap, gitid.BLOB_ID_BYTES), dtype="u1")
        state = np.zeros(cap, dtype="u1")
        rep = np.zeros(cap, dtype="<i8")
        blob_off = np.zeros(cap + 1, dtype="<i8")
        doc_first = np.zeros(n + 1, dtype="<i8")
        r = lib().mtr_replay_handover(self.h, C.addressof(batch.c), int(parts), out.ctypes.data, out.size,
                                      ids.ctypes.data, state.ctypes.data, rep.ctypes.data, blob_off.ctypes.data, cap,
                                      doc_first.ctypes.data)
        if r < 0:
            raise EngineError(f"mtr_replay_handover failed: {_err()}")
        nb = int(doc_first[n])
        return out, state[:nb], rep[:nb], blob_off[:nb + 1], doc_first, ids[:nb]

    def run(self):
        self._check(lib().mtr_run(self.h), "mtr_run")

    def set_matrix(self, rows_doc, cols_doc):
        """Documents rows_doc / cols_doc are the rows / cols PermutationVectors of one SharedMatrix
        (the rows document's op list drives both; see include/mtr.h mtr_set_matrix)."""
        self._check(lib().mtr_set_matrix(self.h, int(rows_doc), int(cols_doc)), "mtr_set_matrix")

    def summarize(self):
        self._check(lib().mtr_summarize(self.h), "mtr_summarize")

    def sync(self):
        self._check(lib().mtr_sync(self.h), "mtr_sync")

    def apply(self, batch):
        self.submit(batch)
        self.run()
        self.sync()

    def generate(self, cfg, tabs, grow=0):
        """Record mode: synthesize cfg.n_docs op logs (include/mtr_synth.h) with this engine's exact
        view lengths and apply them; the recorded batch stays on the device for replays.  grow > 0:
        every document first loads `grow` two-unit snapshot segments (config C5; mtr_generate_grown)."""
        self._tabs = tabs
        self._cfg = cfg
        self._grow = grow
        self._check(lib().mtr_generate_grown(self.h, C.byref(cfg), C.addressof(tabs.c), grow), "mtr_generate")

    def generate_matrix(self, cfg, tabs):
        """Record mode for SharedMatrix logs (mtr_synth_matrix_finish): cfg.n_docs matrices, matrix m
        = engine documents (2m rows, 2m+1 cols); the recorded logs stay on the device for replays."""
        self._tabs = tabs
        self._cfg = cfg
        self._grow = 0
        self._check(lib().mtr_generate_matrix(self.h, C.byref(cfg), C.addressof(tabs.c)), "mtr_generate_matrix")

    def download_matrix(self, lo, hi):
        """The recorded op lists of matrices [lo, hi) as a host Batch with one document per matrix (the
        layout of oracle.generate_matrix)."""
        from .synth import with_docs
        n = hi - lo
        per = self._cfg.ops_per_doc + 1
        docs = np.zeros(2 * n, dtype=abi.DOC_DTYPE)
        ops = np.zeros(max(n * per, 1), dtype=abi.OP_DTYPE)
        text = np.zeros(1, dtype="<u2")
        self._check(lib().mtr_download_batch(self.h, 2 * lo, 2 * hi, docs.ctypes.data, ops.ctypes.data,
                                             text.ctypes.data, 0), "mtr_download_batch")
        return with_docs(self._tabs, docs[0::2].copy(), ops[:n * per], text)

    def download(self, lo, hi, pinned_memory=False):
        """The recorded batch of documents [lo, hi) as a host Batch (sharing the recipe tables); with
        pinned_memory the op and text arrays live in page-locked memory (full-rate uploads)."""
        from .synth import with_docs
        n = hi - lo
        per = getattr(self, "_grow", 0) + self._cfg.ops_per_doc + 1
        alloc = (lambda k, dt: pinned(k, dt)) if pinned_memory else (lambda k, dt: np.zeros(k, dtype=dt))
        docs = np.zeros(n, dtype=abi.DOC_DTYPE)
        ops = alloc(n * per, abi.OP_DTYPE)
        cap = n * int(self._cfg.text_cap)
        text = alloc(max(cap, 1), "<u2")
        self._check(lib().mtr_download_batch(self.h, lo, hi, docs.ctypes.data, ops.ctypes.data, text.ctypes.data, cap),
                    "mtr_download_batch")
        used = int(docs["text_base"][-1] + docs["text_count"][-1]) if n else 0
        text = text[:max(used, 1)] if pinned_memory else text[:max(used, 1)].copy()
        return with_docs(self._tabs, docs, ops, text)

    def summary(self, doc) -> list[bytes]:
        nb, nbytes = C.c_int64(0), C.c_int64(0)
        self._check(lib().mtr_summary_info(self.h, doc, C.byref(nb), C.byref(nbytes)), "mtr_summary_info")
        out = np.zeros(max(nbytes.value, 1), dtype="u1")
        lens = np.zeros(max(nb.value, 1), dtype="<i8")
        r = lib().mtr_get_summary(self.h, doc, out.ctypes.data, out.size, lens.ctypes.data, nb.value)
        if r < 0:
            raise EngineError(f"mtr_get_summary failed ({r}): {_err()}")
        res, off = [], 0
        for k in range(r):
            res.append(out[off:off + lens[k]].tobytes())
            off += int(lens[k])
        return res

    def summaries(self, lo=0, hi=None, out=None):
        """Every blob of documents [lo, hi) in one device-to-host copy (mtr_get_summaries).  Returns
        (buffer, doc_off): document lo + i's record is buffer[doc_off[i]:doc_off[i + 1]] = u32 blob
        count nb, nb u32 lengths, the blob bytes.  `out` (a u1 array, e.g. pinned) is reused when big
        enough."""
        hi = self._n_docs() if hi is None else hi
        doc_off = np.zeros(hi - lo + 1, dtype="<i8")
        need = lib().mtr_get_summaries(self.h, lo, hi, None, 0, doc_off.ctypes.data)
        if need == -1:
            raise EngineError(_err())
        need = -need if need < 0 else need
        if out is None or out.size < need:
            out = np.zeros(max(need, 1), dtype="u1")
        r = lib().mtr_get_summaries(self.h, lo, hi, out.ctypes.data, out.size, doc_off.ctypes.data)
        if r < 0:
            raise EngineError(f"mtr_get_summaries failed ({r}): {_err()}")
        return out, doc_off

    @staticmethod
    def split_record(buf, a, b) -> list[bytes]:
        """The blobs of one document record of :meth:`summaries`."""
        nb = int(np.frombuffer(buf[a:a + 4].tobytes(), "<u4")[0])
        lens = np.frombuffer(buf[a + 4:a + 4 + 4 * nb].tobytes(), "<u4")
        res, off = [], a + 4 + 4 * nb
        for n in lens:
            res.append(buf[off:off + int(n)].tobytes())
            off += int(n)
        assert off == b, "malformed summary record"
        return res

    def _n_docs(self):
        return int(self.stats()["docs"])

    def hashes(self, n=None) -> np.ndarray:
        n = self.max_docs if n is None else n
        out = np.zeros(n, dtype="<u8")
        self._check(lib().mtr_summary_hashes(self.h, out.ctypes.data, n), "mtr_summary_hashes")
        return out

    def blob_ids_raw(self, lo=0, hi=None, cap=None):
        """mtr_summary_blob_ids over documents [lo, hi): (ids [count, 20] u1, doc_first [hi - lo + 1] i8) -- document
        lo + i's ids are ids[doc_first[i]:doc_first[i + 1]], in the order of its record's blobs.  `cap` (blobs): the
        first buffer's size (default: four a document, grown when the engine asks for more)."""
        hi = self._n_docs() if hi is None else hi
        doc_first = np.zeros(max(hi - lo, 0) + 1, dtype="<i8")
        cap = max(1, 4 * (hi - lo) if cap is None else int(cap))  # (cap >= 1: -1 then only means an error)
        while True:
            out = np.zeros((cap, gitid.BLOB_ID_BYTES), dtype="u1")
            r = lib().mtr_summary_blob_ids(self.h, lo, hi, out.ctypes.data, cap, doc_first.ctypes.data)
            if r == -1:
                raise EngineError(f"mtr_summary_blob_ids failed: {_err()}")
            if r >= 0:
                return out[:r], doc_first
            cap = -r

    def blob_ids(self, lo=0, hi=None) -> list[list[str]]:
        """Per document of [lo, hi): the git blob ids (40 hex digits, gitid.git_blob_id) of its summary blobs, in
        summary()'s order, hashed on the device."""
        ids, first = self.blob_ids_raw(lo, hi)
        hexes = [row.tobytes().hex() for row in ids]
        return [hexes[first[i]:first[i + 1]] for i in range(len(first) - 1)]

    def git_blob_ids(self, blobs) -> list[str]:
        """The git blob ids of host blobs (those a host builds itself: catch-up ops, an interval header), hashed on
        the device (mtr_git_blob_ids)."""
        blobs = [bytes(b) for b in blobs]
        off = np.zeros(len(blobs) + 1, dtype="<i8")
        np.cumsum([len(b) for b in blobs], out=off[1:])
        data = np.frombuffer(b"".join(blobs) or b"\0", dtype="u1")
        return self.git_blob_ids_packed(data, off)

    def git_blob_ids_packed(self, data, off) -> list[str]:
        """git_blob_ids for blobs already packed: blob i is data[off[i]:off[i + 1]] (a u1 array, i8 offsets)."""
        data = np.ascontiguousarray(data, dtype="u1")
        off = np.ascontiguousarray(off, dtype="<i8")
        n = len(off) - 1
        if n < 0 or (n > 0 and (off[0] < 0 or off[-1] > data.size or np.any(np.diff(off) < 0))):
            raise EngineError("git_blob_ids_packed: offsets outside the data or decreasing")
        out = np.zeros((max(n, 1), gitid.BLOB_ID_BYTES), dtype="u1")
        self._check(lib().mtr_git_blob_ids(self.h, data.ctypes.data, off.ctypes.data, n, out.ctypes.data),
                    "mtr_git_blob_ids")
        return [row.tobytes().hex() for row in out[:n]]

    def tree_ids_raw(self, lo=0, hi=None, extras=None) -> np.ndarray:
        """mtr_summary_tree_ids over documents [lo, hi): [hi - lo, 20] u1, the git tree id of each document's summary
        tree (gitid.summary_tree_id), hashed on the device.  ``extras``: per document of the range a list of host-made
        ``(mode, name, id_hex)`` entries of its top tree (None or shorter than the range: none for the rest)."""
        hi = self._n_docs() if hi is None else hi
        n = max(hi - lo, 0)
        out = np.zeros((max(n, 1), gitid.BLOB_ID_BYTES), dtype="u1")
        x = first = None
        if extras is not None:
            extras = list(extras)
            if len(extras) > n:
                raise EngineError(f"tree_ids: extras for {len(extras)} documents, the range has {n}")
            x, first = pack_tree_entries(extras + [()] * (n - len(extras)))
        r = lib().mtr_summary_tree_ids(self.h, lo, hi, None if x is None else x.ctypes.data,
                                       None if first is None else first.ctypes.data, out.ctypes.data)
        if r < 0:
            raise EngineError(f"mtr_summary_tree_ids failed: {_err()}")
        return out[:n]

    def tree_ids(self, lo=0, hi=None, extras=None) -> list[str]:
        """Per document of [lo, hi): the git tree id (40 hex digits) of its summary tree; see tree_ids_raw."""
        return [row.tobytes().hex() for row in self.tree_ids_raw(lo, hi, extras)]

    def git_tree_ids(self, trees) -> list[str]:
        """The git tree ids of host trees (the levels above the document: channel, data store), each a list of
        ``(mode, name, id_hex)`` in any order, hashed on the device (mtr_git_tree_ids)."""
        trees = list(trees)
        x, first = pack_tree_entries(trees)
        out = np.zeros((max(len(trees), 1), gitid.BLOB_ID_BYTES), dtype="u1")
        self._check(lib().mtr_git_tree_ids(self.h, x.ctypes.data, first.ctypes.data, len(trees), out.ctypes.data),
                    "mtr_git_tree_ids")
        return [row.tobytes().hex() for row in out[:len(trees)]]

    def set_baseline(self, ids=None):
        """The baseline of the incremental hand-over: the blob ids storage already holds, keyed by (document, blob
        index).  ``None`` marks the current summary (mtr_summary_set_baseline, a device-to-device copy); otherwise a
        list per document of hex ids (blob_ids()' result) or an ``(ids [count, 20] u1, doc_first)`` pair
        (blob_ids_raw()'s).  It stays until the next set_baseline / clear_baseline, across batches and reset()."""
        if ids is None:
            self._check(lib().mtr_summary_set_baseline(self.h), "mtr_summary_set_baseline")
            return
        if isinstance(ids, tuple):
            raw, first = ids
            raw = np.ascontiguousarray(raw, dtype="u1").reshape(-1, gitid.BLOB_ID_BYTES)
            first = np.ascontiguousarray(first, dtype="<i8")
        else:
            first = np.zeros(len(ids) + 1, dtype="<i8")
            np.cumsum([len(doc) for doc in ids], out=first[1:])
            raw = np.frombuffer(bytes.fromhex("".join(x for doc in ids for x in doc)), dtype="u1")
            raw = raw.reshape(-1, gitid.BLOB_ID_BYTES)
        if len(first) < 1 or first[-1] != len(raw):
            raise EngineError("set_baseline: doc_first does not end at the id count")
        self._check(lib().mtr_summary_set_baseline_ids(self.h, raw.ctypes.data if len(raw) else None,
                                                       first.ctypes.data, len(first) - 1),
                    "mtr_summary_set_baseline_ids")

    def clear_baseline(self):
        self._check(lib().mtr_summary_clear_baseline(self.h), "mtr_summary_clear_baseline")

    def summary_delta_info(self, lo=0, hi=None):
        """(blobs, changed blobs, changed bytes) of documents [lo, hi) (mtr_summary_delta_info)."""
        hi = self._n_docs() if hi is None else hi
        nb, nc, by = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(lib().mtr_summary_delta_info(self.h, lo, hi, C.byref(nb), C.byref(nc), C.byref(by)),
                    "mtr_summary_delta_info")
        return nb.value, nc.value, by.value

    def summary_delta_raw(self, lo=0, hi=None, out=None):
        """The blobs of documents [lo, hi) that are new or differ from the baseline, in one device-to-host copy
        (mtr_summary_delta).  Returns (buffer, flags, blob_off, doc_first): blob k of the range (blob_ids_raw()'s
        order) is changed when flags[k] is 1 and its bytes are buffer[blob_off[k]:blob_off[k + 1]] (empty for an
        unchanged blob); document lo + i's blobs are doc_first[i]:doc_first[i + 1].  `out` (a u1 array, e.g. pinned)
        is reused when big enough."""
        hi = self._n_docs() if hi is None else hi
        nb, _, nbytes = self.summary_delta_info(lo, hi)
        if out is None or out.size < nbytes:
            out = np.zeros(max(nbytes, 1), dtype="u1")
        flags = np.zeros(nb, dtype="u1")
        blob_off = np.zeros(nb + 1, dtype="<i8")
        doc_first = np.zeros(max(hi - lo, 0) + 1, dtype="<i8")
        r = lib().mtr_summary_delta(self.h, lo, hi, out.ctypes.data, out.size, flags.ctypes.data,
                                    blob_off.ctypes.data, nb, doc_first.ctypes.data)
        if r < 0:
            raise EngineError(f"mtr_summary_delta failed ({r}): {_err()}")
        return out, flags, blob_off, doc_first

    def summary_delta(self, lo=0, hi=None):
        """Per document of [lo, hi): a list of (id_hex, bytes | None) in summary()'s order -- None where the baseline
        holds the same id at the same index, the blob otherwise (gitid.summary_delta is the host definition)."""
        hi = self._n_docs() if hi is None else hi
        buf, flags, off, first = self.summary_delta_raw(lo, hi)
        ids = self.blob_ids(lo, hi)
        res = []
        for i, doc in enumerate(ids):
            b0 = int(first[i])
            res.append([(x, buf[off[b0 + k]:off[b0 + k + 1]].tobytes() if flags[b0 + k] else None)
                        for k, x in enumerate(doc)])
        return res

    @staticmethod
    def _raw_ids(ids) -> np.ndarray:
        """Hex strings, or an (n, 20) u1 array, as a contiguous (n, 20) u1 array."""
        if isinstance(ids, np.ndarray):
            raw = np.ascontiguousarray(ids, dtype="u1")
        else:
            raw = np.frombuffer(bytes.fromhex("".join(ids)), dtype="u1")
        if raw.size % gitid.BLOB_ID_BYTES:
            raise EngineError("blob ids: not 20 bytes (40 hex digits) each")
        return raw.reshape(-1, gitid.BLOB_ID_BYTES)

    def blob_cache_add(self, ids):
        """Adds ids storage holds to the device blob-id cache (mtr_blob_cache_add): hex strings or an (n, 20) u1 array.
        The cache is a set -- the stand-in for SummaryTreeUploadManager's blobsShaCache -- that stays across batches,
        summaries and reset() until blob_cache_clear()."""
        raw = self._raw_ids(ids)
        self._check(lib().mtr_blob_cache_add(self.h, raw.ctypes.data if len(raw) else None, len(raw)),
                    "mtr_blob_cache_add")

    def blob_cache_add_summary(self):
        """Adds the id of every blob of the current summary, device to device (mtr_blob_cache_add_summary): call it
        once storage has acknowledged the upload."""
        self._check(lib().mtr_blob_cache_add_summary(self.h), "mtr_blob_cache_add_summary")

    def blob_cache_clear(self):
        self._check(lib().mtr_blob_cache_clear(self.h), "mtr_blob_cache_clear")

    def blob_cache_size(self) -> int:
        """The number of distinct ids the cache holds."""
        return int(lib().mtr_blob_cache_size(self.h))

    def blob_cache_has(self, ids) -> np.ndarray:
        """Per id (hex strings or an (n, 20) u1 array): 1 when the cache holds it, else 0 (mtr_blob_cache_has) -- for
        the blobs the host makes itself."""
        raw = self._raw_ids(ids)
        out = np.zeros(len(raw), dtype="u1")
        self._check(lib().mtr_blob_cache_has(self.h, raw.ctypes.data if len(raw) else None, len(raw),
                                             out.ctypes.data), "mtr_blob_cache_has")
        return out

    def blob_cache_generation(self) -> int:
        """The cache's generation (mtr_blob_cache_generation): the acknowledged summaries so far, or what an import
        brought; gitid.BlobCacheModel is the host definition of this and the calls below."""
        r = int(lib().mtr_blob_cache_generation(self.h))
        if r < 0:
            raise EngineError(f"mtr_blob_cache_generation failed ({r}): {_err()}")
        return r

    def blob_cache_ages(self, n) -> np.ndarray:
        """out[a] = the entries last referenced a generations ago, out[n - 1] = all older ones (mtr_blob_cache_ages);
        1 <= n <= 1024."""
        out = np.zeros(max(int(n), 1), dtype="<i8")
        self._check(lib().mtr_blob_cache_ages(self.h, out.ctypes.data, int(n)), "mtr_blob_cache_ages")
        return out

    def blob_cache_trim(self, min_generation) -> int:
        """Drops the entries not referenced since `min_generation` (stamp < min_generation) on the device and returns
        how many (mtr_blob_cache_trim); the survivors keep their order and the freed memory goes back."""
        r = int(lib().mtr_blob_cache_trim(self.h, int(min_generation)))
        if r < 0:
            raise EngineError(f"mtr_blob_cache_trim failed ({r}): {_err()}")
        return r

    def blob_cache_trim_to(self, max_entries) -> int:
        """Trims to at most `max_entries` entries by whole generations, oldest first (mtr_blob_cache_trim_to); returns
        the entries removed."""
        r = int(lib().mtr_blob_cache_trim_to(self.h, int(max_entries)))
        if r < 0:
            raise EngineError(f"mtr_blob_cache_trim_to failed ({r}): {_err()}")
        return r

    def blob_cache_export(self):
        """(ids[n, 20] u1, ages[n] u4) of the entries in table order (mtr_blob_cache_export): what blob_cache_import
        of a restarted summarizer takes."""
        n = self.blob_cache_size()
        ids = np.zeros((n, gitid.BLOB_ID_BYTES), dtype="u1")
        ages = np.zeros(n, dtype="<u4")
        if n:
            r = int(lib().mtr_blob_cache_export(self.h, ids.ctypes.data, ages.ctypes.data, n))
            if r != n:
                raise EngineError(f"mtr_blob_cache_export failed ({r}): {_err()}")
        return ids, ages

    def blob_cache_import(self, ids, ages):
        """Offers ids (hex strings or an (n, 20) u1 array) with their ages (mtr_blob_cache_import): the generation
        becomes at least the largest age, and of equal ids the youngest age wins."""
        raw = self._raw_ids(ids)
        age = np.ascontiguousarray(ages, dtype="<u4").reshape(-1)
        if len(age) != len(raw):
            raise EngineError(f"blob_cache_import: {len(raw)} ids but {len(age)} ages")
        self._check(lib().mtr_blob_cache_import(self.h, raw.ctypes.data if len(raw) else None,
                                                age.ctypes.data if len(age) else None, len(raw)),
                    "mtr_blob_cache_import")

    def summary_novel_info(self, lo=0, hi=None):
        """(blobs, first occurrences, their bytes) of documents [lo, hi) (mtr_summary_novel_info)."""
        hi = self._n_docs() if hi is None else hi
        nb, nf, by = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(lib().mtr_summary_novel_info(self.h, lo, hi, C.byref(nb), C.byref(nf), C.byref(by)),
                    "mtr_summary_novel_info")
        return nb.value, nf.value, by.value

    def summary_novel_raw(self, lo=0, hi=None, out=None):
        """The blobs of documents [lo, hi) sorted against the blob-id cache, and the ones to upload in one
        device-to-host copy (mtr_summary_novel).  Returns (buffer, state, rep, blob_off, doc_first): blob k of the
        range has state[k] 0 (the cache holds its id), 1 (new, the first blob of the whole summary with the id: its
        bytes are buffer[blob_off[k]:blob_off[k + 1]]) or 2 (new, a repeat of the earlier blob rep[k]); rep[k] is a
        summary-wide blob index (-1 for state 0).  `out` (a u1 array, e.g. pinned) is reused when big enough."""
        hi = self._n_docs() if hi is None else hi
        nb, _, nbytes = self.summary_novel_info(lo, hi)
        if out is None or out.size < nbytes:
            out = np.zeros(max(nbytes, 1), dtype="u1")
        state = np.zeros(nb, dtype="u1")
        rep = np.zeros(nb, dtype="<i8")
        blob_off = np.zeros(nb + 1, dtype="<i8")
        doc_first = np.zeros(max(hi - lo, 0) + 1, dtype="<i8")
        r = lib().mtr_summary_novel(self.h, lo, hi, out.ctypes.data, out.size, state.ctypes.data, rep.ctypes.data,
                                    blob_off.ctypes.data, nb, doc_first.ctypes.data)
        if r < 0:
            raise EngineError(f"mtr_summary_novel failed ({r}): {_err()}")
        return out, state, rep, blob_off, doc_first

    def summary_novel(self, lo=0, hi=None):
        """Per document of [lo, hi): a list of (id_hex, state, rep, bytes | None) in summary()'s order
        (gitid.summary_novel over all documents is the host definition; this is its rows lo..hi)."""
        hi = self._n_docs() if hi is None else hi
        buf, state, rep, off, first = self.summary_novel_raw(lo, hi)
        ids = self.blob_ids(lo, hi)
        res = []
        for i, doc in enumerate(ids):
            b0 = int(first[i])
            res.append([(x, int(state[b0 + k]), int(rep[b0 + k]),
                         buf[off[b0 + k]:off[b0 + k + 1]].tobytes() if state[b0 + k] == 1 else None)
                        for k, x in enumerate(doc)])
        return res

    def summary_bytes(self) -> int:
        return int(lib().mtr_summary_bytes(self.h))

    def text(self, doc) -> str:
        n = lib().mtr_get_text(self.h, doc, None, 0)
        if n < 0:
            raise EngineError(_err())
        buf = np.zeros(max(n, 1), dtype="<u2")
        lib().mtr_get_text(self.h, doc, buf.ctypes.data, n)
        return buf[:n].tobytes().decode("utf-16-le", "surrogatepass")

    def texts(self, lo, hi) -> list[str]:
        """Local-view texts of documents [lo, hi): one device gather, one download (mtr_get_texts)."""
        off = np.zeros(hi - lo + 1, dtype="<i8")
        n = lib().mtr_get_texts(self.h, lo, hi, None, 0, off.ctypes.data)
        if n < 0:
            raise EngineError(_err())
        buf = np.zeros(max(n, 1), dtype="<u2")
        if n and lib().mtr_get_texts(self.h, lo, hi, buf.ctypes.data, n, off.ctypes.data) != n:
            raise EngineError(f"mtr_get_texts failed: {_err()}")
        return [buf[off[i]:off[i + 1]].tobytes().decode("utf-16-le", "surrogatepass") for i in range(hi - lo)]

    def props(self, doc, ref) -> list:
        """The properties an MTR_DELTA_REGEN_X record references (mtr_get_props): [(key id, value id)]."""
        # (a first buffer of 17 words: an empty set's single word fits, so -1 can only mean an error)
        out = np.zeros(17, dtype="<u4")
        n = lib().mtr_get_props(self.h, doc, ref, out.ctypes.data, len(out))
        if n == -1:
            raise EngineError(_err())
        if n < 0:
            out = np.zeros(-n, dtype="<u4")
            if lib().mtr_get_props(self.h, doc, ref, out.ctypes.data, len(out)) != len(out):
                raise EngineError(f"mtr_get_props failed: {_err()}")
        return [(int(out[1 + 2 * k]), int(out[2 + 2 * k])) for k in range(int(out[0]))]

    def deltas(self, doc) -> np.ndarray:
        """The delta ranges (abi.DELTA_DTYPE) of the MTR_F_DELTA ops of the last batch for one document."""
        cap = 1024  # cap >= 1, so -1 can only mean an error
        while True:
            out = np.zeros(cap, dtype=abi.DELTA_DTYPE)
            n = lib().mtr_get_deltas(self.h, doc, out.ctypes.data, cap)
            if n == -1:
                raise EngineError(_err())
            if n >= 0:
                break
            cap = -n
        return out[:n]

    def deltas_batch(self, docs=None, n=None, props=False):
        """mtr_get_deltas_batch over `docs` (document indices in any order, repeats allowed; None = documents
        0 .. n - 1, n None = every document of the engine): one size query, then one fetch.  Returns (doc_first,
        records): doc_first [n + 1] i8, the listed documents' first records with the total last; records
        [total] abi.DELTA_DTYPE, what deltas(doc) returns for each listed document, back to back.  With props also
        (props_off, words): props_off [total + 1] i8 offsets into words per record, words u4 the sets mtr_get_props
        returns for the MTR_DELTA_REGEN_X records of SharedString documents, [n, key id, value id, ...] each."""
        if docs is None:
            n, dp = (self.max_docs if n is None else int(n)), None
        else:
            d = np.ascontiguousarray(docs, dtype="<u4")
            n, dp = int(d.size), (d.ctypes.data if d.size else None)
        first = np.zeros(n + 1, dtype="<i8")
        fn = lib().mtr_get_deltas_batch
        total = fn(self.h, dp, n, None, 0, first.ctypes.data, None, 0, None)
        if total < 0:
            raise EngineError(f"mtr_get_deltas_batch failed: {_err()}")
        total = int(total)
        recs = np.zeros(total, dtype=abi.DELTA_DTYPE)
        if not props:
            if total and fn(self.h, dp, n, recs.ctypes.data, total, first.ctypes.data, None, 0, None) != total:
                raise EngineError(f"mtr_get_deltas_batch failed: {_err()}")
            return first, recs
        poff = np.zeros(total + 1, dtype="<i8")
        if not total:
            return first, recs, poff, np.zeros(0, dtype="<u4")
        # (the words' size query carries the records and the offsets; a second fetch only where there are words)
        if fn(self.h, dp, n, recs.ctypes.data, total, first.ctypes.data, None, 0, poff.ctypes.data) != total:
            raise EngineError(f"mtr_get_deltas_batch failed: {_err()}")
        words = np.zeros(int(poff[total]), dtype="<u4")
        if words.size and fn(self.h, dp, n, recs.ctypes.data, total, first.ctypes.data, words.ctypes.data, words.size,
                             poff.ctypes.data) != total:
            raise EngineError(f"mtr_get_deltas_batch failed: {_err()}")
        return first, recs, poff, words

    def deltas_many(self, docs) -> list:
        """deltas(doc) of every document of `docs` from one batched call (mtr_get_deltas_batch): an abi.DELTA_DTYPE
        array per document."""
        first, recs = self.deltas_batch(docs)
        return [recs[int(a):int(b)] for a, b in zip(first[:-1], first[1:])]

    def containing_segment(self, doc, pos, ref_seq, client):
        """Client.getContainingSegment(pos, {referenceSequenceNumber, clientId}) on the device:
        None when no segment covers pos, else a dict of mtr_segment_info fields plus the text."""
        info = SegmentInfo()
        text = np.zeros(1 << 12, dtype="<u2")
        self._check(lib().mtr_get_containing_segment(self.h, doc, pos, ref_seq, client, C.byref(info),
                                                     text.ctypes.data, text.size), "mtr_get_containing_segment")
        if info.leaf < 0:
            return None
        if not info.marker and info.length > text.size:  # the text did not fit: ask again with room for it
            text = np.zeros(info.length, dtype="<u2")
            self._check(lib().mtr_get_containing_segment(self.h, doc, pos, ref_seq, client, C.byref(info),
                                                         text.ctypes.data, text.size), "mtr_get_containing_segment")
        r = {n: getattr(info, n) for n, _ in SegmentInfo._fields_}
        r["text"] = None if info.marker else text[:info.length].tobytes().decode("utf-16-le", "surrogatepass")
        return r

    def view_length(self, doc, ref_seq, client) -> int:
        """nodeLength(root) at the (ref_seq, client) view (mtr_get_containing_segment past the end); this client's own
        short id at its currentSeq is SharedString.getLength."""
        info = SegmentInfo()
        self._check(lib().mtr_get_containing_segment(self.h, doc, 0x7fffffff, ref_seq, client, C.byref(info), None, 0),
                    "mtr_get_containing_segment")
        return int(info.start)

    def _segment_queries(self, queries, want_text, want_props):
        """mtr_get_containing_segments over `queries` ((doc, pos, ref_seq, client) tuples): one size query, then one
        fetch.  Returns (info, text, text_off, props, props_off); a half that is not wanted comes back as None."""
        n = len(queries)
        q = np.zeros(max(n, 1), dtype=abi.VIEW_QUERY_DTYPE)
        for i, (doc, pos, ref_seq, client) in enumerate(queries):
            q[i] = (doc, pos, ref_seq, client)
        info = (SegmentInfo * max(n, 1))()
        toff = np.zeros(n + 1, dtype="<i8") if want_text else None
        poff = np.zeros(n + 1, dtype="<i8") if want_props else None
        tp = toff.ctypes.data if want_text else None
        pp = poff.ctypes.data if want_props else None
        fn = lib().mtr_get_containing_segments
        if fn(self.h, q.ctypes.data, n, C.addressof(info), None, 0, tp, None, 0, pp) != n:
            raise EngineError(f"mtr_get_containing_segments failed: {_err()}")
        text = np.zeros(max(int(toff[n]), 1), dtype="<u2") if want_text else None
        props = np.zeros(max(int(poff[n]), 1), dtype="<u4") if want_props else None
        if (want_text and toff[n]) or (want_props and poff[n]):
            if fn(self.h, q.ctypes.data, n, C.addressof(info), text.ctypes.data if want_text else None,
                  text.size if want_text else 0, tp, props.ctypes.data if want_props else None,
                  props.size if want_props else 0, pp) != n:
                raise EngineError(f"mtr_get_containing_segments failed: {_err()}")
        return info, text, toff, props, poff

    def containing_segments(self, queries) -> list:
        """Engine.containing_segment for many (doc, pos, ref_seq, client) views in one batched call
        (mtr_get_containing_segments): per query None when no segment covers pos, else containing_segment's dict with
        an added "properties" entry, the segment's properties as Engine.props gives them (None when it has no set, and
        for every segment of a matrix vector; "props" stays the set's index in the document's arena, as
        containing_segment reports it)."""
        queries = list(queries)
        info, text, toff, props, poff = self._segment_queries(queries, True, True)
        out = []
        for i in range(len(queries)):
            x = info[i]
            if x.leaf < 0:
                out.append(None)
                continue
            r = {n: getattr(x, n) for n, _ in SegmentInfo._fields_}
            # (a matrix vector's segment has no units in the batch: containing_segment reports `length` zero units)
            u = text[toff[i]:toff[i + 1]] if toff[i + 1] > toff[i] else np.zeros(x.length, dtype="<u2")
            r["text"] = None if x.marker else u.tobytes().decode("utf-16-le", "surrogatepass")
            w = props[poff[i]:poff[i + 1]]
            # (no words: no property set -- or a matrix vector's segment, whose "props" is a tracking id)
            r["properties"] = [(int(w[1 + 2 * k]), int(w[2 + 2 * k])) for k in range(int(w[0]))] if len(w) else None
            out.append(r)
        return out

    def view_lengths(self, queries) -> list:
        """Engine.view_length for many (doc, ref_seq, client) views in one batched call."""
        info = self._segment_queries([(d, 0x7fffffff, r, c) for d, r, c in queries], False, False)[0]
        return [int(info[i].start) for i in range(len(queries))]

    def _range_queries(self, queries, placeholder, want_info, want_text, want_props):
        """mtr_get_range_segments over `queries` ((doc, start, end, ref_seq, client) tuples; end None = the view's
        end): a sizing call, then the fetch (and a second fetch for the property words, whose total the first one
        reports).  Returns (seg_first, info, text, text_first, text_off, props, props_off); what is not wanted is None."""
        n = len(queries)
        q = np.zeros(max(n, 1), dtype=abi.RANGE_QUERY_DTYPE)
        for i, (doc, start, end, ref_seq, client) in enumerate(queries):
            q[i] = (doc, start, 0x7fffffff if end is None else end, ref_seq, client)
        ph = ord(placeholder) if placeholder else 0
        if ph > 0xffff:
            raise ValueError("the placeholder is one UTF-16 unit")
        fn = lib().mtr_get_range_segments
        first = np.zeros(n + 1, dtype="<i8")
        tfirst = np.zeros(n + 1, dtype="<i8") if want_text else None
        tfp = tfirst.ctypes.data if want_text else None
        total = fn(self.h, q.ctypes.data, n, ph, first.ctypes.data, None, 0, None, 0, tfp, None, None, 0, None)
        if total < 0:
            raise EngineError(f"mtr_get_range_segments failed: {_err()}")
        info = (SegmentInfo * max(total, 1))() if want_info else None
        text = np.zeros(max(int(tfirst[n]), 1), dtype="<u2") if want_text else None
        toff = np.zeros(total + 1, dtype="<i8") if want_text and want_info else None
        poff = np.zeros(total + 1, dtype="<i8") if want_props else None
        props = None
        if total and (want_info or want_text or want_props):
            if fn(self.h, q.ctypes.data, n, ph, first.ctypes.data, C.addressof(info) if want_info else None, total,
                  text.ctypes.data if want_text else None, text.size if want_text else 0, tfp,
                  toff.ctypes.data if toff is not None else None, None, 0,
                  poff.ctypes.data if want_props else None) != total:
                raise EngineError(f"mtr_get_range_segments failed: {_err()}")
        if want_props:
            props = np.zeros(max(int(poff[total]), 1), dtype="<u4")
            if poff[total] and fn(self.h, q.ctypes.data, n, ph, first.ctypes.data, None, 0, None, 0, None, None,
                                  props.ctypes.data, props.size, poff.ctypes.data) != total:
                raise EngineError(f"mtr_get_range_segments failed: {_err()}")
        return first, info, text, tfirst, toff, props, poff

    def range_segments(self, queries, placeholder="") -> list:
        """Client.walkSegments over [start, end) at a (ref_seq, client) view, for many (doc, start, end, ref_seq,
        client) queries in one batched call (mtr_get_range_segments; end None = the view's end).  Per query the list
        of its segments, each containing_segment's dict for the walk's position in it ("offset" is the clip at the
        range's start) with "text" = the segment's units inside the range (a marker: the one-unit `placeholder`, ""
        without one) and "properties" as containing_segments gives them."""
        queries = list(queries)
        first, info, text, _, toff, props, poff = self._range_queries(queries, placeholder, True, True, True)
        out = []
        for i in range(len(queries)):
            segs = []
            for k in range(int(first[i]), int(first[i + 1])):
                x = info[k]
                r = {n: getattr(x, n) for n, _ in SegmentInfo._fields_}
                r["text"] = text[toff[k]:toff[k + 1]].tobytes().decode("utf-16-le", "surrogatepass")
                w = props[poff[k]:poff[k + 1]]
                r["properties"] = [(int(w[1 + 2 * j]), int(w[2 + 2 * j])) for j in range(int(w[0]))] if len(w) else None
                segs.append(r)
            out.append(segs)
        return out

    def range_texts(self, queries, placeholder="") -> list:
        """MergeTreeTextHelper.getText(refSeq, clientId, placeholder, start, end) for many (doc, start, end, ref_seq,
        client) queries in one batched call: the text-only form of mtr_get_range_segments (no segment rows are built
        or downloaded)."""
        queries = list(queries)
        _, _, text, tfirst, _, _, _ = self._range_queries(queries, placeholder, False, True, False)
        return [text[tfirst[i]:tfirst[i + 1]].tobytes().decode("utf-16-le", "surrogatepass") for i in range(len(queries))]

    def properties_at(self, queries) -> list:
        """SharedString.getPropertiesAtPosition for many (doc, pos, ref_seq, client) queries in one batched call: the
        properties of the segment of the range [pos, pos + 1), as Engine.props gives them; None where no segment covers
        pos or the segment has no property set."""
        queries = [(d, p, p + 1, r, c) for d, p, r, c in queries]
        first, _, _, _, _, props, poff = self._range_queries(queries, "", False, False, True)
        out = []
        for i in range(len(queries)):
            w = props[poff[first[i]]:poff[first[i + 1]]]
            out.append([(int(w[1 + 2 * j]), int(w[2 + 2 * j])) for j in range(int(w[0]))] if len(w) else None)
        return out

    def _position_rows(self, q) -> np.ndarray:
        """mtr_transform_positions over an abi.POSITION_QUERY_DTYPE array: the abi.POSITION_DTYPE rows."""
        n = len(q)
        out = np.zeros(max(n, 1), dtype=abi.POSITION_DTYPE)
        if lib().mtr_transform_positions(self.h, q.ctypes.data if n else None, n, out.ctypes.data) != n:
            raise EngineError(f"mtr_transform_positions failed: {_err()}")
        return out[:n]

    def transform_positions(self, queries) -> list:
        """mtr_transform_positions over `queries` ((doc, pos, ref_seq, client, to_ref_seq, to_client, mode, offset)
        tuples, mode abi.POS_FROM_VIEW or abi.POS_FROM_LEAF) in one batched call: per query a dict of mtr_position's
        fields (pos -1 = undefined, leaf -1 = no segment, offset, flags: abi.POS_FOUND | POS_VISIBLE | POS_AT_END)."""
        q = np.array([tuple(x) for x in queries], dtype=abi.POSITION_QUERY_DTYPE).reshape(-1)
        rows = self._position_rows(np.ascontiguousarray(q))
        return [{n: int(r[n]) for n in abi.POSITION_DTYPE.names} for r in rows]

    def resolve_remote_positions(self, queries) -> list:
        """Client.resolveRemoteClientPosition(pos, ref_seq, client) for many (doc, pos, ref_seq, client, to_ref_seq,
        to_client) queries in one batched call: the position in the (to_ref_seq, to_client) view of what `pos` names in
        the (ref_seq, client) view, None where the reference returns undefined."""
        q = np.zeros(0, dtype=abi.POSITION_QUERY_DTYPE)
        queries = list(queries)
        if queries:
            q = np.array([(d, p, r, c, tr, tc, abi.POS_FROM_VIEW, 0) for d, p, r, c, tr, tc in queries],
                         dtype=abi.POSITION_QUERY_DTYPE)
        return [None if p < 0 else int(p) for p in self._position_rows(q)["pos"]]

    def segment_positions(self, queries) -> list:
        """Client.getPosition(segment) + offset at the (ref_seq, client) view for many (doc, leaf, offset, ref_seq,
        client) queries in one batched call, the segment named by its tree-order ordinal (containing_segment's
        "leaf"); None for an ordinal the document does not hold."""
        q = np.zeros(0, dtype=abi.POSITION_QUERY_DTYPE)
        queries = list(queries)
        if queries:
            q = np.array([(d, leaf, 0, 0, r, c, abi.POS_FROM_LEAF, off) for d, leaf, off, r, c in queries],
                         dtype=abi.POSITION_QUERY_DTYPE)
        return [None if p < 0 else int(p) for p in self._position_rows(q)["pos"]]

    def ref_positions(self, doc) -> list:
        """Client.localReferencePositionToPosition of every local reference of `doc`, by id
        (abi.DETACHED_POSITION = -1 when it has none)."""
        n = lib().mtr_get_ref_positions(self.h, doc, None, 0)
        if n < 0:
            raise EngineError(f"mtr_get_ref_positions: {_err()}")
        if n == 0:
            return []
        out = np.zeros(n, dtype="<i4")
        self._check(int(lib().mtr_get_ref_positions(self.h, doc, out.ctypes.data, n) != n), "mtr_get_ref_positions")
        return [int(x) for x in out]

    def ref_states(self, doc) -> list:
        """[(position, state bits abi.REF_ST_*)] of every local reference of `doc`, by id (mtr_get_ref_states)."""
        n = lib().mtr_get_ref_states(self.h, doc, None, 0)
        if n < 0:
            raise EngineError(f"mtr_get_ref_states: {_err()}")
        if n == 0:
            return []
        out = np.zeros(2 * n, dtype="<i4")
        self._check(int(lib().mtr_get_ref_states(self.h, doc, out.ctypes.data, 2 * n) != n), "mtr_get_ref_states")
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]

    def ref_keys(self, doc) -> list:
        """[(position, state bits, compare key, offset)] of every local reference of `doc`, by id (mtr_get_ref_keys:
        the key increases in tree order; -1 = no segment, -2 = a segment no longer in the tree)."""
        n = lib().mtr_get_ref_keys(self.h, doc, None, 0)
        if n < 0:
            raise EngineError(f"mtr_get_ref_keys: {_err()}")
        if n == 0:
            return []
        out = np.zeros(4 * n, dtype="<i4")
        self._check(int(lib().mtr_get_ref_keys(self.h, doc, out.ctypes.data, 4 * n) != n), "mtr_get_ref_keys")
        return [tuple(int(x) for x in out[4 * i:4 * i + 4]) for i in range(n)]

    def refs_batch(self, docs, mode):
        """mtr_get_refs over `docs` (document indices in any order, repeats allowed; None = every document of the
        engine): one size query, then one fetch.  mode: abi.REFS_POSITIONS / REFS_STATES / REFS_KEYS, the words per
        reference.  Returns (doc_first, words): doc_first [n + 1] i8, the listed documents' first references with the
        total last; words [total * mode] i4, what the single call of that mode writes for each listed document, back
        to back."""
        mode = int(mode)
        if docs is None:
            n, dp = self.max_docs, None
        else:
            d = np.ascontiguousarray(docs, dtype="<u4")
            n, dp = int(d.size), (d.ctypes.data if d.size else None)
        first = np.zeros(n + 1, dtype="<i8")
        fn = lib().mtr_get_refs
        total = fn(self.h, dp, n, mode, None, 0, first.ctypes.data)
        if total < 0:
            raise EngineError(f"mtr_get_refs failed: {_err()}")
        words = np.zeros(int(total) * mode, dtype="<i4")
        if total and fn(self.h, dp, n, mode, words.ctypes.data, words.size, first.ctypes.data) != total:
            raise EngineError(f"mtr_get_refs failed: {_err()}")
        return first, words

    def _refs_many(self, docs, mode):
        first, w = self.refs_batch(docs, mode)
        return [w[mode * int(a):mode * int(b)].reshape(-1, mode).tolist() for a, b in zip(first[:-1], first[1:])]

    def ref_positions_many(self, docs=None) -> list:
        """ref_positions of every document of `docs` from one batched call (mtr_get_refs): a list per document."""
        return [[r[0] for r in x] for x in self._refs_many(docs, abi.REFS_POSITIONS)]

    def ref_states_many(self, docs=None) -> list:
        """ref_states of every document of `docs` from one batched call (mtr_get_refs): a list per document."""
        return [[tuple(r) for r in x] for x in self._refs_many(docs, abi.REFS_STATES)]

    def ref_keys_many(self, docs=None) -> list:
        """ref_keys of every document of `docs` from one batched call (mtr_get_refs): a list per document."""
        return [[tuple(r) for r in x] for x in self._refs_many(docs, abi.REFS_KEYS)]

    def query_intervals(self, sets, refs, queries):
        """mtr_query_intervals in one batched call.  sets: (doc, first, count) per interval collection; refs: the
        start and end reference ids of every interval, [n_intervals, 2] (interval k of a set is row first + k);
        queries: (set, start, end, mode) with mode abi.IVQ_OVERLAP / IVQ_PREVIOUS / IVQ_NEXT.  Returns (hit_first
        [n + 1] i8, status [n] i4 (abi.IVQ_UNLINKED), hits: an abi.INTERVAL_HIT_DTYPE array, query i's rows at
        hit_first[i] .. hit_first[i + 1])."""
        s = np.array([tuple(x) for x in sets], dtype=abi.INTERVAL_SET_DTYPE).reshape(-1)
        r = np.ascontiguousarray(refs, dtype="<u4").reshape(-1)
        q = np.array([tuple(x) for x in queries], dtype=abi.INTERVAL_QUERY_DTYPE).reshape(-1)
        n = int(q.size)
        first = np.zeros(n + 1, dtype="<i8")
        status = np.zeros(max(n, 1), dtype="<i4")
        # (room for every row the queries can have -- an OVERLAP query at most its set's intervals, the others one -- so
        # that one call answers; the pages are touched only where rows land.  Past 2^22 rows: a size query first.)
        if n and int(q["set"].max()) >= s.size:
            raise EngineError(f"query_intervals: a query names set {int(q['set'].max())} of {s.size}")
        overlap = q["mode"] == abi.IVQ_OVERLAP
        bound = int(s["count"][q["set"][overlap]].sum()) + int((~overlap).sum())
        hits = np.empty(bound if bound <= 1 << 22 else 0, dtype=abi.INTERVAL_HIT_DTYPE)

        def call():
            return int(lib().mtr_query_intervals(self.h, s.ctypes.data if s.size else None, int(s.size),
                                                 r.ctypes.data if r.size else None, int(r.size) // 2,
                                                 q.ctypes.data if n else None, n, first.ctypes.data, status.ctypes.data,
                                                 hits.ctypes.data, int(hits.size)))

        total = call()
        if total == abi.MTR_SUMMARY_TOO_SMALL or total > hits.size:  # (hit_first is filled: ask again with room)
            hits = np.zeros(int(first[n]), dtype=abi.INTERVAL_HIT_DTYPE)
            total = call()
        if total < 0:
            raise EngineError(f"mtr_query_intervals failed: {_err()}")
        return first, status[:n], hits[:total]

    def find_markers(self, labels, vals, queries) -> np.ndarray:
        """mtr_find_markers in one batched call.  labels: (key id or abi.LABEL_ANY, first, count) per label; vals: the
        value ids the labels' [first, first + count) ranges index, ascending inside a range; queries: (doc, pos,
        ref_seq, client, mode, label) with mode abi.MK_PRECEDING / MK_FOLLOWING / MK_BY_ID (pos = the marker ordinal).
        Returns the abi.MARKER_HIT_DTYPE rows (pos -1, leaf -1 = none)."""
        lb = np.array([tuple(x) for x in labels], dtype=abi.MARKER_LABEL_DTYPE).reshape(-1)
        v = np.ascontiguousarray(vals, dtype="<u4").reshape(-1)
        q = np.array([tuple(x) for x in queries], dtype=abi.MARKER_QUERY_DTYPE).reshape(-1)
        n = int(q.size)
        out = np.zeros(max(n, 1), dtype=abi.MARKER_HIT_DTYPE)
        if lib().mtr_find_markers(self.h, lb.ctypes.data if lb.size else None, int(lb.size),
                                  v.ctypes.data if v.size else None, int(v.size), q.ctypes.data if n else None, n,
                                  out.ctypes.data) != n:
            raise EngineError(f"mtr_find_markers failed: {_err()}")
        return out[:n]

    @staticmethod
    def _marker_hits(rows) -> list:
        names = ("pos", "leaf", "ref_type", "props", "seq")
        return [{k: int(r[k]) for k in names} | {"visible": bool(r["flags"] & abi.MK_VISIBLE)}
                if r["flags"] & abi.MK_FOUND else None for r in rows]

    def find_tiles(self, interner, queries) -> list:
        """SharedString.findTile(pos, label, preceding) at a (ref_seq, client) view, for many (doc, pos, ref_seq,
        client, label, preceding) queries in one batched call (mtr_find_markers): the nearest marker at or before
        (preceding) or at or after pos whose "referenceTileLabels" hold the label.  Per query None when there is none,
        else {pos, leaf, ref_type, props, seq, visible}: the marker's position in the view and mtr_segment_info's
        fields of it.  interner: the Interner the documents' batches were built with."""
        queries = list(queries)
        labels, vals, index, qs = [], [], {}, []
        for doc, pos, ref_seq, client, label, preceding in queries:
            if label not in index:
                key, ids = interner.label_values("referenceTileLabels", label)
                index[label] = len(labels)
                # (a key no batch ever held comes with no values: a label without values matches nothing)
                labels.append((0 if key is None else key, len(vals), len(ids)))
                vals += ids
            qs.append((doc, pos, ref_seq, client, abi.MK_PRECEDING if preceding else abi.MK_FOLLOWING, index[label]))
        return self._marker_hits(self.find_markers(labels, vals, qs))

    def markers_from_ids(self, logs, queries) -> list:
        """SharedString.getMarkerFromId(id) followed by getPosition at a (ref_seq, client) view, for many (doc, id,
        ref_seq, client) queries in one batched call.  logs[doc] is the document's DocLog, which maps ids to marker
        ordinals.  Per query None for an id no marker has (or whose marker zamboni took out of the tree), else
        find_tiles' dict, "visible" telling whether the view shows the marker.  An id that block updates may have
        remapped raises Unsupported, as a relative position on it does."""
        from .batch import DocLog, Unsupported

        qs, known = [], []
        for doc, mid, ref_seq, client in queries:
            log = logs[doc]
            k = DocLog._id_key(mid)
            if k is None or k not in log.marker_ids:
                known.append(False)
                continue
            if k in log.marker_dup or log.marker_id_annotated:
                raise Unsupported("a marker id remapped by block updates")
            known.append(True)
            qs.append((doc, log.marker_ids[k], ref_seq, client, abi.MK_BY_ID, 0))
        hits = iter(self._marker_hits(self.find_markers([], [], qs)))
        return [next(hits) if k else None for k in known]

    def leaves(self, doc) -> np.ndarray:
        """A matrix vector's segments in tree order, [n, 5] int32: cachedLength, removed, start handle, tracking id
        (-1: none), tracking-group bits (mtr_get_leaves)."""
        n = lib().mtr_get_leaves(self.h, doc, None, 0)
        if n < 0:
            raise EngineError(f"mtr_get_leaves: {_err()}")
        out = np.zeros(5 * max(n, 1), dtype="<i4")
        self._check(int(lib().mtr_get_leaves(self.h, doc, out.ctypes.data, n) != n), "mtr_get_leaves")
        return out[:5 * n].reshape(n, 5)

    def ref_info(self, doc, ref_id):
        """(leaf index of the reference's segment or -1, offset, refType, held by the segment's collection)"""
        out = np.zeros(4, dtype="<i4")
        if lib().mtr_get_ref_info(self.h, doc, ref_id, out.ctypes.data) == -2:
            raise EngineError(f"mtr_get_ref_info: {_err()}")
        return int(out[0]), int(out[1]), int(out[2]), bool(out[3])

    def pending_groups(self, doc) -> int:
        """MergeTree.pendingSegments.length of document doc (its unacked local ops' SegmentGroups)."""
        n = lib().mtr_pending_groups(self.h, doc)
        if n < 0:
            raise EngineError(f"mtr_pending_groups: bad document {doc}")
        return int(n)

    def status(self, doc):
        op = C.c_int32(-1)
        st = lib().mtr_doc_status(self.h, doc, C.byref(op))
        return st, op.value

    def export(self, doc):
        h = C.c_int32(0)
        n = lib().mtr_export(self.h, doc, None, 0, C.byref(h))
        n = -n if n < 0 else n
        out = np.zeros((max(n, 1), 8), dtype="<i4")
        lib().mtr_export(self.h, doc, out.ctypes.data, n, C.byref(h))
        return out[:n], h.value

    def stats(self) -> dict:
        out = np.zeros(10, dtype="<i8")
        self._check(lib().mtr_stats(self.h, out.ctypes.data, 10), "mtr_stats")
        keys = ["ops", "docs", "max_leaves", "sum_leaves", "bad_docs", "launches", "max_heap", "max_text",
                "sum_leaves_before_op", "text_units_inserted"]
        return dict(zip(keys, (int(x) for x in out)))

    def profile(self, reset=True) -> dict:
        """Phase timers of a -DMTR_PROF build (empty dict otherwise)."""
        out = np.zeros(len(PROFILE_KEYS), dtype="<u8")
        if lib().mtr_profile(self.h, out.ctypes.data, len(PROFILE_KEYS), int(reset)) != 0:
            return {}
        return dict(zip(PROFILE_KEYS, (int(x) for x in out)))

    def launch_counts(self) -> dict:
        """mtr_debug_launch_counts: the apply launches since the engine was created or last reset().  Per name of
        LAUNCH_VARIANTS the launches of that runtime-layout kernel; "fixed_cap" those of the fixed-capacity kernels;
        "min_cap" / "max_cap" the smallest and largest leaf capacity launched and "max_lds_cap" the largest of an
        LDS-resident launch (0 when there was none); "global_mode" the HBM-resident launches; "launches" all of them."""
        tail = ["fixed_cap", "min_cap", "max_cap", "global_mode", "max_lds_cap"]
        n = len(LAUNCH_VARIANTS) + len(tail)
        out = np.zeros(n, dtype="<i8")
        got = lib().mtr_debug_launch_counts(self.h, out.ctypes.data, n)
        if got != n:
            raise EngineError(f"mtr_debug_launch_counts: the library reports {got} counters, this binding knows {n}")
        res = dict(zip(LAUNCH_VARIANTS + tail, (int(x) for x in out)))
        res["launches"] = sum(res[k] for k in LAUNCH_VARIANTS) + res["fixed_cap"]
        return res

    def timing(self) -> dict:
        out = np.zeros(17, dtype="<f8")
        lib().mtr_last_timing(self.h, out.ctypes.data, 17)
        return {"apply_ms": float(out[0]), "summary_ms": float(out[1]), "apply_launches": int(out[2]),
                "apply_kernel_ms": float(out[3]), "blob_ids_ms": float(out[4]), "delta_ms": float(out[5]),
                "delta_gather_ms": float(out[6]), "tree_ids_ms": float(out[7]), "novel_ms": float(out[8]),
                "novel_gather_ms": float(out[9]), "novel_classify_ms": float(out[10]),
                "cache_trim_ms": float(out[11]), "cache_ages_ms": float(out[12]),
                "handover_copied_bytes": float(out[13]), "handover_ids_ms": float(out[14]),
                "handover_novel_ms": float(out[15]), "handover_ranges": int(out[16])}


# enum ApplyVariant (csrc/apply.hip.h) in its order, without the AV_ prefix: mtr_debug_launch_counts' first counters
LAUNCH_VARIANTS = ["LDS_X", "HBM_X", "LDS_LEAN", "HBM_LEAN", "LDS_DL", "HBM_DL", "LDS_GN", "HBM_GN", "PAIR_LDS",
                   "PAIR_HBM", "PAIR_LDS_DL", "PAIR_HBM_DL", "PAIR_LDS_GN", "PAIR_HBM_GN", "PAIR2_LDS", "PAIR2_HBM"]

PROFILE_KEYS = ["op", "prefix", "split", "shift", "insert", "range", "zamboni", "zblock", "compact", "find_uid",
                "text_gc", "loadstore", "text_copy", "update_seq", "n_zblock", "n_compact", "scour1", "pack", "nlq",
                "pmatch", "tappend", "heap", "overflow", "n_pack", "n_merge", "n_pmatch", "n_nlq", "split1", "ins1",
                "fetch", "x1", "x2", "pf_sum", "pf_dirty", "materialize", "csum", "n_chunks", "n_listed", "n_dirty", "spread", "chunk_of", "n_spread",
                "load", "pre", "view", "post", "n_sup", "n_dch", "helper", "sink",
                "ovf_bounds", "ovf_parent", "n_ovf_nowin", "n_ovf_rounds", "sup_refresh", "px_list_eval", "px_eval",
                "px_sync", "n_px_rounds", "n_walk", "n_dirty_rounds", "walk", "n_pop", "n_pop_noop"]


def caps_for(batch, margin=1.25):
    """Per-document arena capacities that a batch can never exceed (host-side bound)."""
    ops = batch.ops
    docs = batch.docs
    n_ops = docs["op_count"].astype(np.int64)
    max_ops = int(n_ops.max()) if len(docs) else 0
    max_text = int(docs["text_count"].max()) if len(docs) else 0
    seg = 2 * max_ops + 64
    text = int(2 * max_text * margin) + 4096
    npk = np.diff(batch.propop_off.astype(np.int64)) if len(batch.propop_off) > 1 else np.zeros(1, np.int64)
    max_keys = int(npk.max()) if npk.size else 0
    prop = int((2 * max_ops) * (1 + 2 * (max_keys + 8)) * 0.25) + 4096
    rem = max_ops + 64
    return dict(max_segments=seg, heap_entries=seg, text_units=text, prop_words=prop, remover_cells=rem)
