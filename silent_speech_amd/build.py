"""Build ``libss_hotpath.so`` in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m silent_speech_amd.build [--force]
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libss_hotpath.so")
SOURCES = ["features.hip", "batch.hip", "stream.hip", "crop_resize.hip", "roi_cnn.hip", "roi_cnn_bwd.hip", "roi_cnn_generic.hip", "gemm.hip", "gru.hip", "pool_head.hip", "eval.hip", "calib.hip", "tail.hip", "optim.hip", "step_helpers.hip", "abi.hip", "gemm_bf16.hip", "gru_bf16.hip", "cnn_bf16.hip", "cnn_bf16_bwd.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


# the streaming kernels of these files keep everything in registers: a by-value table indexed per lane, or a spill, would show as a
# private segment in the code object's metadata (ss_adamw_clip_groups)
NO_SCRATCH = ["optim.hip", "step_helpers.hip", "batch.hip"]


def _llvm_tool(name: str):
    hipcc = shutil.which(_hipcc()) or _hipcc()
    roots = [os.environ.get("ROCM_PATH"), os.path.join(os.path.dirname(os.path.realpath(hipcc)), ".."), "/opt/rocm"]
    for root in roots:
        for sub in (("llvm", "bin"), ("lib", "llvm", "bin"), ("bin",)):
            cand = os.path.join(root, *sub, name) if root else None
            if cand and os.path.exists(cand):
                return cand
    return shutil.which(name)


def kernel_private_segments(obj: str) -> dict:
    """{kernel symbol: .private_segment_fixed_size} of the gfx950 code object inside the host object ``obj`` (its AMDGPU metadata
    note), or None when the LLVM tools that read it are not installed."""
    objdump, readelf = _llvm_tool("llvm-objdump"), _llvm_tool("llvm-readelf")
    if not objdump or not readelf:
        return None
    with tempfile.TemporaryDirectory() as tmp:  # (the bundles are written next to the file that is read)
        copy = shutil.copy(obj, tmp)
        subprocess.check_call([objdump, "--offloading", copy], stdout=subprocess.DEVNULL, cwd=tmp)
        device = [os.path.join(tmp, f) for f in os.listdir(tmp) if "amdgcn" in f]
        if len(device) != 1:
            raise RuntimeError(f"{obj}: expected one device code object, found {len(device)}")
        notes = subprocess.check_output([readelf, "--notes", device[0]], text=True)
    sizes, pending = {}, None
    for line in notes.splitlines():  # (the keys of a kernel's record are sorted: the size comes before the symbol)
        key, _, value = line.strip().lstrip("- ").partition(":")
        if key == ".private_segment_fixed_size":
            pending = int(value)
        elif key == ".symbol" and pending is not None:
            sizes[value.strip().strip("'\"")], pending = pending, None
    if not sizes:
        raise RuntimeError(f"{obj}: no kernel metadata found")
    return sizes


def check_no_scratch(verbose: bool = True) -> None:
    for src in NO_SCRATCH:
        sizes = kernel_private_segments(os.path.join(CSRC, src[:-4] + ".o"))
        if sizes is None:
            print(f"silent_speech_amd.build: llvm-objdump / llvm-readelf not found, the private segments of {src} are unchecked",
                  file=sys.stderr)
            return
        bad = {k: v for k, v in sizes.items() if v}
        if bad:
            raise RuntimeError(f"{src}: kernels with a private (scratch) segment, bytes per lane: {bad}")
        if verbose:
            print(f"{src}: {len(sizes)} kernels, private segment 0 bytes each", flush=True)


def build(force: bool = False, verbose: bool = True, stamp: bool = False) -> str:
    """``stamp=True`` builds the diagnostic library (in-kernel stage timers) next to the real one."""
    if stamp:
        # A/B experiments: SS_STAMP_DEFS="-DSS_FWD_STOP=1" SS_STAMP_OUT=libss_hotpath_stampB.so builds a second variant
        out = os.path.join(HERE, os.environ.get("SS_STAMP_OUT", "libss_hotpath_stamp.so"))
        srcs = [os.path.join(CSRC, s) for s in SOURCES]
        cmd = [_hipcc(), *FLAGS, "-DSS_STAMP", *os.environ.get("SS_STAMP_DEFS", "").split(), "-shared", "-o", out, *srcs]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return out
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hdrs.append(os.path.join(HERE, "..", "include", "ss_hotpath.h"))
    srcs = [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    objs = []
    procs = []
    for s in srcs:
        o = s[:-4] + ".o"
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            cmd = [_hipcc(), *FLAGS, "-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((s, subprocess.Popen(cmd)))
    for s, pr in procs:
        if pr.wait() != 0:
            raise RuntimeError(f"hipcc failed on {s}")
    if force or procs or _stale(OUT, objs):
        check_no_scratch(verbose)
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT, *objs]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv, stamp="--stamp" in sys.argv)
