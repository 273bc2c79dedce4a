"""The CPU reference of eslam_gpu_resample_stratified / _multinomial (tests/c/resample_ref.c):
built with gcc into tests/c/_build/ (git-ignored) and bound with ctypes -- test infrastructure."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "resample_ref.c")
LIB_PATH = os.path.join(ROOT, "tests", "c", "_build", "libresample_ref.so")
# the oracle's flags (oracle/Makefile): the arithmetic rounds as on the device
CFLAGS = ["-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=gnu11", "-Wall", "-Wno-unused-function"]
DEPS = [SRC, os.path.join(ROOT, "include", "eslam_detmath.h")]

_lib = None


def build(verbose=False):
    """gcc the reference unless the library is newer than its sources."""
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
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
        for fn in (L.rr_stratified, L.rr_multinomial):
            fn.restype = C.c_uint64
            fn.argtypes = [dp, C.c_uint64, C.c_uint64, up, C.c_int, up, C.POINTER(C.c_uint64)]
        L.rr_shift.restype = C.c_int
        L.rr_shift.argtypes = [C.c_double]
        L.rr_uniforms.restype = None
        L.rr_uniforms.argtypes = [C.c_uint32, C.c_uint64, dp]
        L.rr_minstd_seed.restype = C.c_uint32
        L.rr_minstd_seed.argtypes = [C.c_uint64]
        _lib = L
    return _lib


def shift_of(weight_sum):
    """the fixed-point shift of a standalone resample: 61 - (dm_weight_exp(S) + 1)"""
    return int(lib().rr_shift(float(weight_sum)))


def minstd_seed(seed):
    return int(lib().rr_minstd_seed(seed))


def uniforms(minstd, count):
    """the boost uniforms of the next `count` minstd draws after state `minstd`"""
    out = np.zeros(count)
    lib().rr_uniforms(minstd, count, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def _run(fn, weights, samples, minstd, shift):
    w = np.ascontiguousarray(weights, dtype=np.float64)
    anc = np.zeros(max(samples, 1), np.uint32)
    x = C.c_uint32(minstd)
    beyond = C.c_uint64()
    m = fn(w.ctypes.data_as(C.POINTER(C.c_double)), w.shape[0], samples, C.byref(x), shift,
           anc.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(beyond))
    return anc[:m].copy(), int(beyond.value), int(x.value)


def stratified(weights, samples, minstd, shift):
    """(ancestors of the `samples` outputs, overruns, new minstd state)"""
    return _run(lib().rr_stratified, weights, samples, minstd, shift)


def multinomial(weights, samples, minstd, shift):
    """(ancestors of the kept draws in draw order, dropped, new minstd state)"""
    return _run(lib().rr_multinomial, weights, samples, minstd, shift)
