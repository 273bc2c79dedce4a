"""The CPU reference of the shared-map merge (tests/c/shared_map_ref.c): built with gcc into
tests/c/_build/ (git-ignored) and bound with ctypes -- test infrastructure."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
import eslam_abi as A  # noqa: E402

SRC = os.path.join(ROOT, "tests", "c", "shared_map_ref.c")
LIB_PATH = os.path.join(ROOT, "tests", "c", "_build", "libshared_map_ref.so")
# the oracle's flags (oracle/Makefile): the arithmetic rounds as on the device
CFLAGS = ["-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=gnu11", "-Wall", "-Wno-unused-function"]
DEPS = [SRC, os.path.join(ROOT, "include", "eslam_detmath.h"), os.path.join(ROOT, "include", "eslam_gpu.h")]

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
        dp, fp, up = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        L.smr_merge.argtypes = [C.POINTER(A.MlsGrid), C.c_uint64, dp, dp, dp, dp, dp, C.POINTER(A.ScanPatch), C.c_uint32,
                                up, fp, fp, fp, C.c_uint64, C.POINTER(A.SharedMergeInfo)]
        L.smr_info_size.restype = C.c_size_t
        _lib = L
    return _lib


def merge(grid, pa, patches):
    """The sequential merge of `patches` (a ctypes array of eslam_scan_patch) into `grid`
    (GridArrays) once per particle of `pa` (ParticleArrays: x, y, orientation, zpos, zsigma),
    in index order: (merged GridArrays, SharedMergeInfo)."""
    count = len(patches)
    cap = int(grid.mean.shape[0]) + pa.n * count
    cells = np.zeros(grid.width * grid.height + 1, np.uint32)
    mean = np.zeros(max(cap, 1), np.float32)
    sd = np.zeros(max(cap, 1), np.float32)
    hgt = np.zeros(max(cap, 1), np.float32)
    info = A.SharedMergeInfo()
    g = grid.view()
    d = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    arrs = [d(getattr(pa, f)) for f in ("x", "y", "orientation", "zpos", "zsigma")]
    rc = lib().smr_merge(C.byref(g), pa.n, *[A._ptr(a, C.c_double) for a in arrs], patches, count,
                         A._ptr(cells, C.c_uint32), A._ptr(mean, C.c_float), A._ptr(sd, C.c_float), A._ptr(hgt, C.c_float),
                         cap, C.byref(info))
    if rc != 0:
        raise RuntimeError(f"smr_merge failed ({rc})")
    n = int(info.n_patches)
    merged = A.GridArrays(grid.width, grid.height, grid.scale, grid.offset, cells, mean[:n].copy(), sd[:n].copy(),
                          None if grid.patch_height is None else hgt[:n].copy(), grid.g2l)
    return merged, info
