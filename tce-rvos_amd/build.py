"""Builds libtce_rvos.so (all HIP kernels + the C ABI) and, after it, its training-side sibling libtce_rvos_train.so (the criterion,
train/tce_rvos_train.h) for gfx950, in-tree.

    python -m tce_rvos_amd.build        (or __graft_entry__.build())

hipcc cross-compiles without a GPU.  Objects are cached by source mtime under csrc/_obj/; translation units are
compiled in parallel (TCE_BUILD_JOBS, default = CPU count capped at 8).
"""
import glob
import os
from concurrent.futures import ThreadPoolExecutor
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libtce_rvos.so")
# slowest first (they gate the parallel build): the GEMM translation units carry one epilogue body per (act, res) combination
SOURCES = ["gemm_f16x3_big_256_split.hip", "gemm_f16x3_big_256_single.hip", "gemm_f16x3_big_128_split.hip", "gemm_f16x3_big_128_single.hip",
           "ffn.hip", "rowlin.hip", "conv3x3.hip", "gemm_f16x3_big.hip", "gemm_f16x3_small.hip", "gemm.hip", "attn.hip", "misc.hip", "norm.hip", "msda.hip",
           "text.hip", "resnet.hip", "frontend.hip", "fewrow.hip", "swinattn.hip", "patch_embed.hip", "thin.hip", "label.hip", "eval.hip", "score.hip", "capi.hip", "a2d_score.hip", "a2d_group.hip", "refexp.hip", "vis.hip", "pngfile.hip", "png.hip"]
# the training-side sibling library: sources of csrc_train/, its header in train/ (not part of SOURCES / dependencies(): the
# inference library's registry is closed by its tests)
TRAIN_CSRC = os.path.join(HERE, "csrc_train")
TRAIN_OBJ = os.path.join(TRAIN_CSRC, "_obj")
TRAIN_LIB = os.path.join(LIBDIR, "libtce_rvos_train.so")
TRAIN_SOURCES = ["criterion.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"] + \
    os.environ.get("HIPCC_EXTRA", "").split()  # audit builds only (e.g. -DFEWROW_RPT2); the shipped library has none


def _newer(src_list, target):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in src_list)


def dependencies():
    """Of every object, besides its own source: csrc's headers, every public header"""
    return sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc")) +
                  glob.glob(os.path.join(HERE, "..", "include", "*.h")))


def train_dependencies():
    """Of every object of the train library, besides its own source: its private headers, train/*.h, and csrc's headers (common.h)"""
    return sorted(glob.glob(os.path.join(TRAIN_CSRC, "*.h")) + glob.glob(os.path.join(HERE, "..", "train", "*.h")) +
                  glob.glob(os.path.join(CSRC, "*.h")))


def _build_lib(sources, csrc, objdir, headers, target, verbose, force):
    os.makedirs(objdir, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    objs, todo = [], []
    for s in sources:
        src = os.path.join(csrc, s)
        obj = os.path.join(objdir, s.replace(".hip", ".o"))
        if force or _newer([src] + headers, obj):
            todo.append([HIPCC] + FLAGS + ["-c", src, "-o", obj])
        objs.append(obj)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    jobs = int(os.environ.get("TCE_BUILD_JOBS", min(8, os.cpu_count() or 1)))
    with ThreadPoolExecutor(max_workers=max(1, jobs)) as pool:
        list(pool.map(run, todo))
    if force or _newer(objs, target):
        tmp = target + f".tmp{os.getpid()}"  # link beside the target, rename into place: no reader ever sees a partial file
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        os.replace(tmp, target)
    return target


def build_train(verbose=True, force=False):
    """libtce_rvos_train.so alone (what _train_lib.lib() calls when the file is absent)"""
    return _build_lib(TRAIN_SOURCES, TRAIN_CSRC, TRAIN_OBJ, train_dependencies(), TRAIN_LIB, verbose, force)


def build(verbose=True, force=False):
    lib = _build_lib(SOURCES, CSRC, OBJ, dependencies(), LIB, verbose, force)
    build_train(verbose, force)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
