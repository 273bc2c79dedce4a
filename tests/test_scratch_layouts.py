"""The two scratch blocks whose size is a plain function of the caller's sizes, asked of the built
library in its size-only mode (no GPU call): the scan build's and the particle-grid composition's.
The expected totals are the hand-written offset chains these functions had before they were
written with the Carver of csrc/eslam_buf.h, restated here as plain arithmetic: every array
rounded up to 256 bytes, in the same order.  (tests/cpp/test_buf.cpp checks every array's offset,
for these and for the layouts that only the context can ask for.)"""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "slam-eslam_amd", "lib", "libeslam_gpu.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import sys
        sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
        import build_lib
        build_lib.build(verbose=False)
    L = C.CDLL(LIB)
    L.eslam_scan_work_bytes.restype = C.c_size_t
    L.eslam_scan_work_bytes.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p]
    L.eslam_pgrid_work_bytes.restype = C.c_size_t
    L.eslam_pgrid_work_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def up(b):
    return (b + 255) & ~255


@pytest.mark.parametrize("n", [0, 1, 63, 257, 2048, 2049])
def test_scan_work_block_has_the_size_it_had(lib, n):
    # the radix sort's scratch is an input of the layout: asked of the sort itself (its tmp == NULL
    # mode, as eslam_scan_work_bytes asks), so a change of the sort does not fail a layout test
    sort_bytes = C.c_size_t(0)
    assert lib.eslam_radix_sort_pairs_passes(None, None, None, None, C.c_uint64(n), None, C.byref(sort_bytes), 4, None) == 0
    sort_bytes = sort_bytes.value
    assert sort_bytes > 0
    u, d = up((n + 1) * 4), up(max(n, 1) * 8)
    want = 6 * u + 4 * d + up(4 * 8) + up(sort_bytes)      # a b c d e raw; pz var sz sv; cnt; sort_tmp
    assert lib.eslam_scan_work_bytes(n, None, None) == want


@pytest.mark.parametrize("w,h", [(1, 1), (63, 1), (1, 257), (63, 257), (257, 63), (257, 257)])
def test_particle_grid_work_block_has_the_size_it_had(lib, w, h):
    tx, ty, blocks = (w + 7) // 8, (h + 7) // 8, (w * h + 1 + 255) // 256
    want = up(tx * ty * 4) + up((blocks + 1) * 4) + up(8)   # dir; bsum; own
    assert lib.eslam_pgrid_work_bytes(w, h, None, None) == want
