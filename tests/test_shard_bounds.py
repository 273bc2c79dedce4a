"""eslam_gpu_shard_bounds (pure host code of the built library, no GPU call): the canonical shard
table in C equals eslam_abi.shard_bounds, and fails exactly where that raises.  A resample of a
sharded filter to another count lays the filter out by this table."""
import ctypes as C
import os

import pytest

import eslam_abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "slam-eslam_amd", "lib", "libeslam_gpu.so")

COUNTS = [65, 128, 129, 130, 3000, 327680, 327681, 330000, 2 ** 30 - 64]
RANKS = [1, 2, 3, 8, 16]
ROWS = [0, 1, 2]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import sys
        sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
        import build_lib
        build_lib.build(verbose=False)
    return C.CDLL(LIB)


def python_table(n, ranks, rows):
    try:
        return A.shard_bounds(n, ranks, rows)
    except ValueError:
        return None


def c_table(lib, n, ranks, rows):
    try:
        return A.shard_bounds_c(lib, n, ranks, rows)
    except ValueError:
        return None


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("ranks", RANKS)
def test_equals_the_python_table(lib, ranks, rows):
    split = 0
    for n in COUNTS:
        want = python_table(n, ranks, rows)
        assert c_table(lib, n, ranks, rows) == want, (n, ranks, rows)
        split += want is not None
    assert split >= 5                                    # most counts can be split on every rank count


def test_chunk_rows_change_between_327680_and_327681(lib):
    assert A.shard_bounds_c(lib, 327680, 2) == [0, 163840, 327680]
    assert A.shard_bounds_c(lib, 327681, 2)[1] % 128 == 0
    assert A.shard_bounds_c(lib, 330000, 2) == [0, 164992, 330000]
    assert A.shard_bounds_c(lib, 129, 3) == [0, 64, 128, 129]


@pytest.mark.parametrize("n,ranks", [(64, 3), (128, 3), (64, 2), (65, 3), (1, 2), (0, 1)])
def test_refuses_where_python_raises(lib, n, ranks):
    assert python_table(n, ranks, 0) is None
    out = (C.c_uint64 * (ranks + 1))(*([7] * (ranks + 1)))
    lib.eslam_gpu_shard_bounds.argtypes = A.SHARD_BOUNDS_ARGTYPES
    assert lib.eslam_gpu_shard_bounds(n, ranks, 0, out) == A.ERR_INVALID_ARG


def test_bad_arguments(lib):
    lib.eslam_gpu_shard_bounds.argtypes = A.SHARD_BOUNDS_ARGTYPES
    out = (C.c_uint64 * 4)()
    assert lib.eslam_gpu_shard_bounds(3000, 0, 0, out) == A.ERR_INVALID_ARG
    assert lib.eslam_gpu_shard_bounds(3000, -1, 0, out) == A.ERR_INVALID_ARG
    assert lib.eslam_gpu_shard_bounds(3000, 2, 0, None) == A.ERR_INVALID_ARG
