"""Build libdad_hip.so (the C-ABI library of include/dad.h) in-tree for gfx950.

Plain `hipcc --offload-arch=gfx950` per translation unit + one shared-library link; the
result (and every variant library, lib_path()) lands in lib/ at the top of the repository, not
inside the package: the package folder's name alone is 104 characters, which inside it puts the
library's absolute path past 255 characters in any checkout whose own path has 134 or more, and
a record of a process's mapped libraries that holds 255 characters per path then loses it.
"""
import concurrent.futures
import os
import subprocess
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_DIR = os.path.join(os.path.dirname(PKG_DIR), "lib")
OBJ_DIR = os.path.join(PKG_DIR, "build")
LIB_PATH = os.path.join(LIB_DIR, "libdad_hip.so")
SOURCES = ["encode.hip", "encode_ws.hip", "tail_general.hip", "tail_w.hip", "tail_w_s16.hip", "wgrad_f32.hip", "wgrad_direct.hip", "reduce.hip", "optim.hip", "dad_abi.hip", "timing.hip", "encoder_ops.hip", "rccl_dp.hip", "collate.hip", "eval.hip", "utils_abi.hip", "prep.hip", "eval_split.hip", "trace.hip", "pairwise.hip", "cluster.hip", "tsne.hip", "domain_gap.hip", "knn.hip", "scl.hip", "eval_windows.hip", "eval_noise.hip", "input_grad.hip", "attribution.hip", "rank.hip", "eval_models.hip",
           "encode_ws_rg.hip", "wgrad_direct_rg.hip", "tail_w_rg.hip", "prep_rg.hip"]   # (the ragged step's `_rg` sibling kernels)
HEADERS = ["dad_common.h", "dad_kernels.h", "dad_probe.h", "dad_prep.h", "step_plan.h", "dad_host.h", "dad_timing.h",
           "tail_common.h", "pool.h", "wgrad_common.h", "wgrad_direct.h", "pairwise.h", "scl.h", "eval_rows.h", "tail_w.hip", "encode_ws.hip",
           os.path.join("..", "..", "include", "dad.h")]   # (tail_w_s16.hip / the `_rg` units include tail_w.hip, encode_ws.hip)
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")
ARCH = os.environ.get("DAD_OFFLOAD_ARCH", "gfx950")
CFLAGS = ["--offload-arch=" + ARCH, "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off",
          "-I" + os.path.join(ROCM, "include")]


def _newest(paths):
    return max(os.path.getmtime(p) for p in paths)


def lib_path(variant=None):
    """Diagnostic builds (e.g. DAD_PROBE_* kernels) live beside the product library."""
    return LIB_PATH if not variant else os.path.join(LIB_DIR, "libdad_hip_%s.so" % variant)


def _compile(src, variant=None, extra=()):
    odir = OBJ_DIR if not variant else os.path.join(OBJ_DIR, variant)
    obj = os.path.join(odir, os.path.splitext(src)[0] + ".o")
    deps = [os.path.join(CSRC, src)] + [os.path.join(CSRC, h) for h in HEADERS]
    if os.path.exists(obj) and os.path.getmtime(obj) >= _newest(deps):
        return obj
    cmd = [HIPCC] + CFLAGS + list(extra) + ["-c", os.path.join(CSRC, src), "-o", obj]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stdout))
    return obj


def build(verbose=True, variant=None, extra=()):
    """Compile (incrementally) and link; returns the library path.

    variant/extra: a diagnostic build with extra compiler flags into lib/libdad_hip_<variant>.so
    (loaded only when DAD_LIB_VARIANT names it; the product library is never replaced).
    """
    path = lib_path(variant)
    os.makedirs(OBJ_DIR if not variant else os.path.join(OBJ_DIR, variant), exist_ok=True)
    os.makedirs(LIB_DIR, exist_ok=True)
    jobs = min(len(SOURCES), int(os.environ.get("MAX_JOBS", "8")))
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        objs = list(ex.map(lambda s: _compile(s, variant, extra), SOURCES))
    if not os.path.exists(path) or os.path.getmtime(path) < _newest(objs):
        cmd = [HIPCC, "-shared", "-o", path] + objs + ["-L" + os.path.join(ROCM, "lib"), "-lrccl"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s" % r.stdout)
    if verbose:
        print("built", path)
    return path


if __name__ == "__main__":
    build()
    sys.exit(0)
