"""The CPU restatement of eslam_gpu_fit_pose_gmm (tests/c/gmm_ref.c): built with gcc
into tests/c/_build/ (git-ignored) and bound with ctypes -- test infrastructure."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
import eslam_abi as A  # noqa: E402

SRC = os.path.join(ROOT, "tests", "c", "gmm_ref.c")
LIB_PATH = os.path.join(ROOT, "tests", "c", "_build", "libgmm_ref.so")
# the oracle's flags (oracle/Makefile): the arithmetic rounds as on the device
CFLAGS = ["-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=gnu11", "-Wall", "-Wno-unused-function"]
DEPS = [SRC, os.path.join(ROOT, "include", "eslam_detmath.h"), os.path.join(ROOT, "include", "eslam_gpu.h")]

_lib = None


def build(verbose=False):
    """gcc the restatement unless the library is newer than its sources."""
    if os.path.exists(LIB_PATH) and all(os.path.getmtime(d) <= os.path.getmtime(LIB_PATH) for d in DEPS):
        return LIB_PATH
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    cmd = [os.environ.get("CC", "gcc")] + CFLAGS + [f"-I{os.path.join(ROOT, 'include')}", "-shared", "-o", LIB_PATH, SRC, "-lm"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        dp = C.POINTER(C.c_double)
        L.gmm_ref_fit.restype = C.c_int
        L.gmm_ref_fit.argtypes = [dp, dp, dp, C.c_uint64, C.c_uint32, C.POINTER(A.GmmParams), C.POINTER(A.GmmComponent),
                                  C.POINTER(A.GmmInfo)]
        _lib = L
    return _lib


def fit(x, y, w, components=3, max_iterations=10, tolerance=1e-5, min_variance=1e-6, sum_chunk_rows=0):
    """(rc, weights[K], means[K, 2], covs[K, 3], GmmInfo) of the restatement on the particles
    (x, y, w), summed in chunks of dm_chunk_rows_cfg(n, sum_chunk_rows) rows."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    assert x.shape == y.shape == w.shape and x.ndim == 1
    dp = C.POINTER(C.c_double)
    p = A.GmmParams(components, max_iterations, tolerance, min_variance)
    k = int(components)
    out = (A.GmmComponent * max(k, 1))()
    info = A.GmmInfo()
    rc = lib().gmm_ref_fit(x.ctypes.data_as(dp), y.ctypes.data_as(dp), w.ctypes.data_as(dp), x.shape[0], sum_chunk_rows,
                           C.byref(p), out, C.byref(info))
    weights = np.array([out[i].weight for i in range(k)], dtype=np.float64)
    means = np.array([list(out[i].mean) for i in range(k)], dtype=np.float64).reshape(k, 2)
    covs = np.array([list(out[i].cov) for i in range(k)], dtype=np.float64).reshape(k, 3)
    return rc, weights, means, covs, info


def info_tuple(info):
    """every field of a GmmInfo, doubles as their bits (NaN compares equal to itself)"""
    d = np.array([info.log_likelihood, info.centre[0], info.centre[1]], dtype=np.float64).view(np.uint64)
    return (info.components_live, info.live_mask, info.iterations, info.converged, info.particles_used, info.particles_skipped,
            int(d[0]), int(d[1]), int(d[2]), info.weight_exp)
