"""The CPU restatement of eslam_gpu_pose_moments (tests/c/moments_ref.c): built with
gcc into tests/c/_build/ (git-ignored) and bound with ctypes -- test infrastructure."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
import eslam_abi as A  # noqa: E402

SRC = os.path.join(ROOT, "tests", "c", "moments_ref.c")
LIB_PATH = os.path.join(ROOT, "tests", "c", "_build", "libmoments_ref.so")
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
        L.moments_ref.restype = C.c_int
        L.moments_ref.argtypes = [dp] * 6 + [C.c_uint64, C.c_uint32, C.POINTER(A.PoseGate), C.POINTER(A.PoseMoments)]
        L.moments_ref_atan2.restype = None
        L.moments_ref_atan2.argtypes = [dp, dp, dp, C.c_uint64]
        L.moments_ref_wrap_pi.restype = None
        L.moments_ref_wrap_pi.argtypes = [dp, dp, C.c_uint64]
        L.moments_ref_sizeof.restype = C.c_uint64
        L.moments_ref_sizeof.argtypes = [C.c_int]
        _lib = L
    return _lib


def moments(x, y, z, theta, zsigma, w, gate=None, sum_chunk_rows=0):
    """(rc, PoseMoments) of the restatement on the particles as a filter of that many particles,
    summed in chunks of dm_chunk_rows_cfg(n, sum_chunk_rows) rows; gate: None or a PoseGate"""
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, z, theta, zsigma, w)]
    assert all(a.ndim == 1 and a.shape == arrs[0].shape for a in arrs)
    dp = C.POINTER(C.c_double)
    out = A.PoseMoments()
    rc = lib().moments_ref(*[a.ctypes.data_as(dp) for a in arrs], arrs[0].shape[0], sum_chunk_rows,
                           None if gate is None else C.byref(gate), C.byref(out))
    return rc, out


def of_particles(pa, gate=None, sum_chunk_rows=0):
    """moments() of an eslam_abi.ParticleArrays"""
    return moments(pa.x, pa.y, pa.zpos, pa.orientation, pa.zsigma, pa.weight, gate, sum_chunk_rows)


def atan2(y, x):
    y, x = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
    y, x = np.ascontiguousarray(y), np.ascontiguousarray(x)
    out = np.empty_like(y)
    dp = C.POINTER(C.c_double)
    lib().moments_ref_atan2(y.ctypes.data_as(dp), x.ctypes.data_as(dp), out.ctypes.data_as(dp), y.size)
    return out


def wrap_pi(d):
    d = np.ascontiguousarray(d, dtype=np.float64)
    out = np.empty_like(d)
    dp = C.POINTER(C.c_double)
    lib().moments_ref_wrap_pi(d.ctypes.data_as(dp), out.ctypes.data_as(dp), d.size)
    return out
