"""Build the HIP engine (libmtr.so, gfx950) and the synthetic op-log generator in-tree.

Only hipcc/g++ invocations -- no cmake, no JIT caches -- so the built .so files travel to the GPU
box with the repository snapshot.
"""
from __future__ import annotations

import json
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

ENGINE_SRC = ["mtr_engine.hip", "apply_run.hip", "handover.hip", "blob_id.hip", "summary_delta.hip", "tree_id.hip",
              "blob_cache.hip", "query.hip"]
ENGINE_DEPS = ENGINE_SRC + ["apply_caps.hip", "apply_variants.hip", "engine.hip.h", "apply.hip.h", "summary.hip.h",
                            "blob_id.hip.h", "summary_delta.hip.h", "tree_id.hip.h", "git_object_id.hip.h",
                            "blob_cache.hip.h"]
CAP_PARTS = 3  # kCapParts in apply.hip.h
VARIANT_PARTS = 16  # kVariantParts in apply.hip.h


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


_REMARK = re.compile(r"remark: +([A-Za-z][A-Za-z /\[\]]*?): (.*?) \[-Rpass-analysis=kernel-resource-usage\]")


def kernel_resources(stderr_texts):
    """Per kernel (mangled name): the compiler's resource-usage remarks (VGPRs, ScratchSize, spills, occupancy)."""
    res, cur = {}, None
    for text in stderr_texts:
        for line in text.splitlines():
            m = _REMARK.search(line)
            if not m:
                continue
            k, v = m.group(1).strip(), m.group(2).strip()
            if k == "Function Name":
                cur = res.setdefault(v, {})
            elif cur is not None:
                cur[k] = int(v) if v.lstrip("-").isdigit() else v
    return res


# No apply kernel may spill VGPRs (apply_kernel / apply_pair_kernel / apply_pair2_kernel, LDS- and HBM-resident), and
# the lean HBM-resident one (CAP = -1: C5's kernel) must use no scratch at all.  A round-3 build whose lean HBM kernel
# spilled produced wrong views; the main build refuses one.  (The X / delta / record-mode
# kernels keep some scratch that is no spill: the call frames of their out-of-line rare paths -- regenerate, normalize,
# props_apply_serial, props_restore -- whose by-reference document structs live on the stack, and a few dynamically
# indexed private arrays)
_APPLY_KERNELS = re.compile(r"^_ZN3mtr(12apply_kernel|17apply_pair_kernel|18apply_pair2_kernel)I")
_HBM_LEAN = re.compile(r"^_ZN3mtr12apply_kernelILb1ELin1E")


def check_no_scratch(res, strict=True):
    bad = {}
    for k, v in res.items():
        if not _APPLY_KERNELS.match(k):
            continue
        scratch, vspill = v.get("ScratchSize [bytes/lane]", 0), v.get("VGPRs Spill", 0)
        if vspill or (_HBM_LEAN.match(k) and scratch):
            bad[k] = (scratch, vspill)
    if bad:
        msg = "apply kernels spill VGPRs: " + ", ".join(
            f"{k} (scratch {a} B/lane, {b} VGPRs spilled)" for k, (a, b) in sorted(bad.items()))
        if strict:
            raise RuntimeError(msg)
        print("warning: " + msg, file=sys.stderr)
    return bad


def check_kernel_no_scratch(res, pattern, what, strict=True):
    """One kernel (mangled names matching `pattern`, called `what` in the message) must use no scratch at all."""
    bad = {k: (v.get("ScratchSize [bytes/lane]", 0), v.get("VGPRs Spill", 0)) for k, v in res.items()
           if pattern.match(k) and (v.get("ScratchSize [bytes/lane]", 0) or v.get("VGPRs Spill", 0))}
    if bad:
        msg = f"the {what} kernel uses scratch: " + ", ".join(
            f"{k} (scratch {a} B/lane, {b} VGPRs spilled)" for k, (a, b) in sorted(bad.items()))
        if strict:
            raise RuntimeError(msg)
        print("warning: " + msg, file=sys.stderr)
    return bad


# The git blob id kernel (blob_id.hip) keeps its 16-word SHA-1 schedule window in VGPRs: any scratch means the window
# went to memory (a dynamically indexed round) or registers spilled, and the main build refuses it.
_BLOB_ID_KERNEL = re.compile(r"^_ZN3mtr18git_blob_id_kernelE")


def check_blob_id_no_scratch(res, strict=True):
    return check_kernel_no_scratch(res, _BLOB_ID_KERNEL, "blob id", strict)


# The delta gather kernel (summary_delta.hip) holds a lane's 16 bytes and the two aligned source words in named
# registers; scratch would put a memory round trip on every 16 bytes it copies, and the main build refuses it.  Its
# range variant (the pipelined hand-over's) shares the 16-byte step and the rule.
_DELTA_GATHER_KERNEL = re.compile(r"^_ZN3mtr(19delta_gather_kernel|25delta_gather_range_kernel)E")


def check_delta_gather_no_scratch(res, strict=True):
    return check_kernel_no_scratch(res, _DELTA_GATHER_KERNEL, "delta gather", strict)


# The tree id kernel (tree_id.hip) hashes materialised tree bodies with the blob kernel's loader and rounds; scratch
# would mean its schedule window went to memory, and the main build refuses it.
_TREE_ID_KERNEL = re.compile(r"^_ZN3mtr18git_tree_id_kernelE")


def check_tree_id_no_scratch(res, strict=True):
    return check_kernel_no_scratch(res, _TREE_ID_KERNEL, "tree id", strict)


# The novel pass's classify kernel (blob_cache.hip) keeps a lane's five id words in named registers through both of its
# probe loops; scratch would put a memory round trip into every probe step, and the main build refuses it.  The same
# holds for its range variant (the pipelined hand-over's).
_NOVEL_CLASSIFY_KERNEL = re.compile(r"^_ZN3mtr(12_GLOBAL__N_1)?(21novel_classify_kernel|27novel_classify_range_kernel)E")


def check_novel_classify_no_scratch(res, strict=True):
    return check_kernel_no_scratch(res, _NOVEL_CLASSIFY_KERNEL, "novel classify", strict)


# The stamp kernel (blob_cache.hip) probes as the has kernel does, the five id words in named registers, before its one
# atomicMax; scratch would put a memory round trip into every probe step, and the main build refuses it.
_CACHE_STAMP_KERNEL = re.compile(r"^_ZN3mtr(12_GLOBAL__N_1)?18cache_stamp_kernelE")


def check_cache_stamp_no_scratch(res, strict=True):
    return check_kernel_no_scratch(res, _CACHE_STAMP_KERNEL, "cache stamp", strict)


# The range-query kernels (query.hip) hold a round's lane values -- lengths, places, sources -- in registers between the
# scans and the copy loops that read them across lanes; scratch would put a memory round trip into every round, and the
# main build refuses it.
_RANGE_QUERY_KERNEL = re.compile(r"^_ZN(3mtr)?(12_GLOBAL__N_1)?(18range_count_kernel|17range_scan_kernel|18range_write_kernel)E")


def check_range_query_no_scratch(res, strict=True):
    return check_kernel_no_scratch(res, _RANGE_QUERY_KERNEL, "range query", strict)


# The batched delta-record kernels (query.hip) hold a round's record, its word count and the scan in registers between
# the 16-byte copy and the set-by-set copy loop that reads them across lanes; scratch would put a memory round trip into
# every round, and the main build refuses it.
_DELTA_QUERY_KERNEL = re.compile(r"^_ZN(3mtr)?(12_GLOBAL__N_1)?(18delta_count_kernel|20delta_records_kernel)E")


def check_delta_query_no_scratch(res, strict=True):
    return check_kernel_no_scratch(res, _DELTA_QUERY_KERNEL, "delta query", strict)


# The position-transform kernel (query.hip) holds a round's two view lengths and their two scans in registers until the
# ballot that finds the leaf reads them across lanes; scratch would put a memory round trip into every round, and the
# main build refuses it.
_POSITION_KERNEL = re.compile(r"^_ZN(3mtr)?(12_GLOBAL__N_1)?15position_kernelE")


def check_position_no_scratch(res, strict=True):
    return check_kernel_no_scratch(res, _POSITION_KERNEL, "position transform", strict)


# The interval-query kernels (query.hip) hold a round's lane values -- an endpoint's reference words and the answer of
# its leaf walk, an interval's two packed keys, the reduction's candidates -- in registers between the scans, ballots and
# reductions that read them across lanes; scratch would put a memory round trip into every round, and the main build
# refuses it.
_INTERVAL_QUERY_KERNEL = re.compile(
    r"^_ZN(3mtr)?(12_GLOBAL__N_1)?(20interval_keys_kernel|21interval_count_kernel|21interval_write_kernel)E")


def check_interval_query_no_scratch(res, strict=True):
    return check_kernel_no_scratch(res, _INTERVAL_QUERY_KERNEL, "interval query", strict)


# The marker-search kernel (query.hip) holds a round's visible lengths, their scan and the candidate lanes in registers
# until the ballot that picks the marker reads them across lanes, and takes the hit's words from leaf_row through a
# private array that must stay in registers; scratch would put a memory round trip into every round, and the main build
# refuses it.
_MARKER_FIND_KERNEL = re.compile(r"^_ZN(3mtr)?(12_GLOBAL__N_1)?18marker_find_kernelE")


def check_marker_find_no_scratch(res, strict=True):
    return check_kernel_no_scratch(res, _MARKER_FIND_KERNEL, "marker search", strict)


def build_engine(force=False, verbose=False, prof=False, variant=None, extra=()):
    """libmtr.so; prof: the phase-timer build (libmtr_prof.so); variant: an experiment build
    libmtr_<variant>.so with extra compiler flags (selected at run time with MTR_LIB)."""
    name = "libmtr_prof.so" if prof else (f"libmtr_{variant}.so" if variant else "libmtr.so")
    out = os.path.join(HERE, name)
    deps = [os.path.join(CSRC, f) for f in ENGINE_DEPS] + [os.path.join(ROOT, "include", h)
                                                           for h in ("mtr.h", "mtr_types.h", "mtr_synth.h", "mtr_digest.h")]
    # (each translation unit is checked against its sources below; the library against its objects)
    # translation units compiled in parallel (the fixed-capacity kernels in CAP_PARTS parts), then linked
    flags = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"] + \
        (["-DMTR_PROF"] if prof else []) + list(extra)
    objdir = os.path.join(HERE, "build_prof" if prof else (f"build_{variant}" if variant else "build"))
    os.makedirs(objdir, exist_ok=True)
    units = [(os.path.join(CSRC, f), os.path.join(objdir, f + ".o"), []) for f in ENGINE_SRC]
    units += [(os.path.join(CSRC, "apply_caps.hip"), os.path.join(objdir, f"apply_caps_{q}.o"), [f"-DMTR_CAP_PART={q}"])
              for q in range(CAP_PARTS)]
    units += [(os.path.join(CSRC, "apply_variants.hip"), os.path.join(objdir, f"apply_variants_{q}.o"),
               [f"-DMTR_VARIANT_PART={q}"]) for q in range(VARIANT_PARTS)]
    procs = []
    hdrs = [d for d in deps if d.endswith(".h")]
    flag_file = os.path.join(objdir, "flags.txt")
    same_flags = os.path.exists(flag_file) and open(flag_file).read() == " ".join(flags)
    reuse = variant and os.environ.get("MTR_REUSE_VARIANTS") == "1"
    # (development: MTR_ONLY=apply_variants_3,mtr_engine recompiles just the units named, keeping the other
    # objects as they are -- for an edit whose effect is confined to those units' kernels)
    only = [x for x in os.environ.get("MTR_ONLY", "").split(",") if x]
    for src, obj, extra in units:
        if only and not any(x in os.path.basename(obj) for x in only):
            main_obj = os.path.join(HERE, "build", os.path.basename(obj))
            if not os.path.exists(obj) and os.path.exists(main_obj):  # (a variant: the main build's object)
                shutil.copy(main_obj, obj)
            if os.path.exists(obj):
                continue
        if same_flags and not force and not _stale(obj, [src] + hdrs):
            continue  # (per translation unit: an edit of one .hip recompiles that unit only)
        if reuse and "apply_variants" in obj:  # (a C3 experiment: the runtime-layout kernels from the main build)
            shutil.copy(os.path.join(HERE, "build", os.path.basename(obj)), obj)
            continue
        cmd = flags + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", obj, src]
        if verbose:
            print(" ".join(cmd))
        procs.append(subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True))
    if not procs and not _stale(out, [u[1] for u in units]):
        return out
    outs = [p.communicate()[1] for p in procs]
    rcs = [p.returncode for p in procs]
    if any(rcs):
        for o in outs:
            sys.stderr.write("\n".join(l for l in o.splitlines() if "kernel-resource-usage" not in l) + "\n")
        raise subprocess.CalledProcessError(max(rcs), "hipcc")
    rpath = os.path.join(objdir, "kernel_resources.json")
    res = json.load(open(rpath)) if os.path.exists(rpath) else {}
    res.update(kernel_resources(outs))
    with open(rpath, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    with open(flag_file, "w") as f:
        f.write(" ".join(flags))
    strict = not (variant or prof) or os.environ.get("MTR_REQUIRE_NO_SCRATCH") == "1"
    check_no_scratch(res, strict=strict)
    check_blob_id_no_scratch(res, strict=strict)
    check_delta_gather_no_scratch(res, strict=strict)
    check_tree_id_no_scratch(res, strict=strict)
    check_novel_classify_no_scratch(res, strict=strict)
    check_cache_stamp_no_scratch(res, strict=strict)
    check_range_query_no_scratch(res, strict=strict)
    check_delta_query_no_scratch(res, strict=strict)
    check_position_no_scratch(res, strict=strict)
    check_interval_query_no_scratch(res, strict=strict)
    check_marker_find_no_scratch(res, strict=strict)
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + [u[1] for u in units]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return out


NODE_INCLUDE = "/usr/include/node"


def build_node_addon(force=False, verbose=False):
    """The N-API addon (node/mtr_napi.node) a Node host loads; needs the Node headers, links libmtr.so."""
    src = os.path.join(HERE, "node", "mtr_napi.cc")
    out = os.path.join(HERE, "node", "mtr_napi.node")
    if not os.path.exists(os.path.join(NODE_INCLUDE, "node_api.h")):
        if verbose:
            print("node headers not found: skipping the N-API addon")
        return None
    deps = [src, os.path.join(ROOT, "include", "mtr.h"), os.path.join(HERE, "libmtr.so")]
    if force or _stale(out, deps):
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-DNODE_GYP_MODULE_NAME=mtr_napi",
               f"-I{NODE_INCLUDE}", "-o", out, src, f"-L{HERE}", "-lmtr", "-Wl,-rpath,$ORIGIN/.."]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return out


def build_all(force=False, verbose=False):
    build_engine(force, verbose)
    build_node_addon(force, verbose)


if __name__ == "__main__":
    if "--prof" in sys.argv:
        build_engine(force="--force" in sys.argv, verbose=True, prof=True)
    elif "--variant" in sys.argv:  # python -m fluidframework_amd.build --variant NAME [flags...]
        i = sys.argv.index("--variant")
        build_engine(force=True, verbose=False, variant=sys.argv[i + 1], extra=sys.argv[i + 2:])
    else:
        build_all(force="--force" in sys.argv, verbose=True)
