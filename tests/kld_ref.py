"""The CPU restatement of eslam_gpu_kld_count (tests/c/kld_ref.c): built with gcc
into tests/c/_build/ (git-ignored) and bound with ctypes -- test infrastructure."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
import eslam_abi as A  # noqa: E402

SRC = os.path.join(ROOT, "tests", "c", "kld_ref.c")
LIB_PATH = os.path.join(ROOT, "tests", "c", "_build", "libkld_ref.so")
# the oracle's flags (oracle/Makefile): the arithmetic rounds as on the device
CFLAGS = ["-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=gnu11", "-Wall", "-Wno-unused-function"]
DEPS = [SRC, os.path.join(ROOT, "include", "eslam_detmath.h"), os.path.join(ROOT, "include", "eslam_gpu.h")]
LIMIT = 2 ** 32 - 2                # the largest count the one-GPU resample accepts

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
        L.kld_ref_count.restype = C.c_int
        L.kld_ref_count.argtypes = [dp, dp, dp, dp, C.c_uint64, C.POINTER(A.KldParams), C.c_uint64, C.c_uint64,
                                    C.POINTER(A.KldInfo)]
        L.kld_ref_bound.restype = C.c_double
        L.kld_ref_bound.argtypes = [C.c_uint64, C.c_double, C.c_double]
        L.kld_ref_samples.restype = C.c_uint64
        L.kld_ref_samples.argtypes = [C.c_double, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double,
                                      C.POINTER(C.c_uint32)]
        L.kld_ref_inv_2pi.restype = C.c_double
        L.kld_ref_inv_2pi.argtypes = []
        _lib = L
    return _lib


def count(x, y, theta, w, limit=LIMIT, capacity=0, **params):
    """(rc, KldInfo) of the restatement on the particles (x, y, theta, w) as a filter of that many
    particles; params: fields of eslam_kld_params over KldParams()'s defaults (n_min 1)."""
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, theta, w)]
    assert all(a.ndim == 1 and a.shape == arrs[0].shape for a in arrs)
    dp = C.POINTER(C.c_double)
    p = A.KldParams(**params)
    info = A.KldInfo()
    rc = lib().kld_ref_count(*[a.ctypes.data_as(dp) for a in arrs], arrs[0].shape[0], C.byref(p), limit, capacity, C.byref(info))
    return rc, info


def bound(k, epsilon=0.05, z_quantile=2.3263478740408408):
    return lib().kld_ref_bound(k, epsilon, z_quantile)


def samples(bound_, n_min, limit, capacity, n_global, min_change):
    """(samples, clamped) of dm_kld_samples"""
    c = C.c_uint32()
    s = lib().kld_ref_samples(bound_, n_min, limit, capacity, n_global, min_change, C.byref(c))
    return int(s), int(c.value)
