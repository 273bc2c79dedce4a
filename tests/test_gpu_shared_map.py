"""processMap's merge into the shared map on the GPU (useSharedMap = true, update = true:
eslam_gpu_shared_map_update, src/EmbodiedSlamFilter.cpp:184-227 and the camera path's call at
:301).  The merged grid equals the sequential reference (tests/c/
shared_map_ref.c) applied to the oracle's particles, bit for bit, after every update; the
next step on the merged grid stays bit-identical with the oracle's, so the rebuilt cell
table, occupancy bits and K1's window are right.  The fuse rule is the build's own (envire's
MLSGrid::merge is not in the reference)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import shared_map_ref as R
import synthetic as S
from parity_util import assert_bit_identical

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 5003                                  # not a multiple of 64
COUNTERS = [f for f, _ in A.SharedMergeInfo._fields_ if f != "runs"]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def counters(info):
    return {f: int(getattr(info, f)) for f in COUNTERS}


def assert_same_grid(got, want, label):
    assert np.array_equal(got.cell_start, want.cell_start), label
    assert np.array_equal(u32(got.mean), u32(want.mean)), label
    assert np.array_equal(u32(got.stdev), u32(want.stdev)), label
    assert (got.patch_height is None) == (want.patch_height is None), label
    if want.patch_height is not None:
        assert np.array_equal(u32(got.patch_height), u32(want.patch_height)), label


def rotated(grid, yaw=0.3, tx=0.4, ty=-0.25):
    """the grid in a local frame rotated by yaw and shifted: global2local = Rz(-yaw) (p - t)"""
    c, s = math.cos(yaw), math.sin(yaw)
    grid.g2l = [c, s, 0.0, -(c * tx + s * ty), -s, c, 0.0, -(-s * tx + c * ty), 0.0, 0.0, 1.0, 0.0]
    return grid


def case_grid(case):
    if case == "flat":
        return S.flat_map(cells=120)
    if case == "spread":
        return S.rough_map(cells=60)
    if case in ("rect", "rect_rotated"):  # 150 x 110 cells of 0.10 x 0.08 m (tests/rect_grids.py)
        import rect_grids
        grid = rect_grids.rect_rough_map(150, 110, (0.10, 0.08))
        return rotated(grid) if case == "rect_rotated" else grid
    grid = S.rough_map(cells=120)
    if case == "rough_heights":           # as test_shared_map_match_bit_exact builds them
        rng = np.random.default_rng(3)
        grid.patch_height = np.where(rng.random(grid.mean.shape[0]) < 0.3, rng.uniform(0.05, 0.5, grid.mean.shape[0]),
                                     0.0).astype(np.float32)
    if case == "rotated_grid":
        grid = rotated(grid)
    return grid


def case_sigma(case):
    return {"concentrated": [0.005, 0.005, 0.005], "spread": [0.5, 0.5, 0.05]}.get(case, [0.1, 0.1, 0.05])


def make_pair(gpu_mod, grid, sigma, flags=0):
    cfg = S.bench_config(A.default_config(), N)
    cfg.flags |= A.FLAG_RECORD_ANCESTORS | flags
    gpu = gpu_mod.GpuFilter(cfg)
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    for f in (gpu, orc):
        f.set_map(grid)
        f.init_gaussian(N, [0.0, 0.0, 0.0], sigma, 0.18, 0.05)
    return gpu, orc


def wide_scans():
    return [S.scan_patches(nx=12, ny=9, x0=-1.0, x1=2.5, y0=-1.5, y1=1.2, z=z) for z in (-0.18, -0.1, 0.4)]


@pytest.mark.parametrize("case", ["flat", "rough", "rough_heights", "rotated_grid", "concentrated", "spread", "rect",
                                  "rect_rotated"])
def test_shared_map_update_bit_exact(gpu_mod, oracle, case):
    grid = case_grid(case)
    gpu, orc = make_pair(gpu_mod, grid, case_sigma(case))
    scan48, wide = S.scan_patches(), wide_scans()
    assert len(scan48) == 48
    stream = S.step_stream(5, tilt=case != "flat")
    total = {f: 0 for f in COUNTERS}
    cur = grid
    for k, st in enumerate(stream):
        # on the merged grid both filters step alike: the rebuilt cell_tab, occ and K1's window
        assert gpu.step(st) == orc.step(st)
        assert_bit_identical(gpu.download(), orc.download(), f"{case} step {k}")
        assert np.array_equal(gpu.ancestors(), orc.ancestors()), (case, k)
        if k == 4:
            break
        before = gpu.download()
        for j, scan in enumerate((scan48, wide[k % 3])):
            info = gpu.shared_map_update(scan)
            want, winfo = R.merge(cur, orc.download(), scan)
            print(case, k, j, counters(info), "runs", info.runs)
            assert_same_grid(gpu.get_map(), want, f"{case} step {k} scan {j}")
            assert counters(info) == counters(winfo), (case, k, j)
            assert info.particles_done == N and info.patches_placed + info.patches_off_grid == N * len(scan)
            assert info.patches_placed == info.fused + info.absorbed + info.inserted
            assert info.n_patches == want.mean.shape[0]
            for f in COUNTERS:
                total[f] += int(getattr(info, f))
            cur = want
        assert_bit_identical(gpu.download(), before, f"{case} step {k}: the merge leaves the particles alone")
        orc.set_map(cur)
    # a no-op cannot pass
    assert total["fused"] > 0 and total["inserted"] > 0, total
    assert cur.mean.shape[0] > grid.mean.shape[0]
    if case == "rough_heights":
        assert total["absorbed"] > 0, total
    if case == "spread":
        assert total["patches_off_grid"] > 0, total
    else:
        assert total["patches_off_grid"] == 0, total
    if case == "concentrated":            # long segments: hundreds of records per touched cell
        assert total["cells_touched"] * 300 < total["patches_placed"], total
    gpu.close()


def test_shared_map_update_is_independent_of_the_runs(gpu_mod, oracle):
    """max_records only splits the particles into runs: hundreds of runs (7 particles each) and
    one particle per run (a value below the scan's 48 patches) give the default's bytes"""
    grid = case_grid("rough")
    scan, ledge = S.scan_patches(), wide_scans()[2]       # the 48 patches fuse; the 108 at z = 0.4 insert
    st = S.step_stream(1, tilt=True)[0]
    got = []
    for max_records in (0, 7 * 48, 40):
        gpu, _ = make_pair(gpu_mod, grid, case_sigma("rough"))
        gpu.step(st)
        a = gpu.shared_map_update(scan, max_records)
        b = gpu.shared_map_update(ledge, max_records)
        got.append((gpu.get_map(), counters(a), counters(b), (int(a.runs), int(b.runs))))
        gpu.close()
    assert [g[3] for g in got] == [(1, 1), (-(-N // 7), -(-N // 3)), (N, N)]
    assert got[0][1]["fused"] > 0 and got[0][2]["inserted"] > 0 and got[0][2]["fused"] > 0
    for g, ca, cb, _ in got[1:]:
        assert_same_grid(g, got[0][0], "runs")
        assert (ca, cb) == got[0][1:3]


@pytest.mark.parametrize("case", ["rough", "rough_heights"])
def test_get_map_after_set_map(gpu_mod, case):
    grid = case_grid(case)
    gpu = gpu_mod.GpuFilter(S.bench_config(A.default_config(), 64))
    gpu.set_map(grid)
    assert_same_grid(gpu.get_map(), grid, case)
    gpu.close()


def test_shared_map_update_errors(gpu_mod):
    grid = case_grid("flat")
    scan = S.scan_patches()

    def code(f, patches=scan):
        with pytest.raises(gpu_mod.EslamError) as e:
            f.shared_map_update(patches)
        return e.value.code

    cfg = S.bench_config(A.default_config(), 256)
    # per-particle maps have their own merge
    pm = S.bench_config(A.default_config(), 256)
    pm.flags |= A.FLAG_PARTICLE_MAPS
    f = gpu_mod.GpuFilter(pm)
    f.set_map(grid)
    f.init_gaussian(256, [0.0, 0.0, 0.0], [0.1, 0.1, 0.05], 0.18, 0.05)
    assert code(f) == A.ERR_INVALID_ARG
    f.close()
    # no map, then no particles
    f = gpu_mod.GpuFilter(cfg)
    assert code(f) == A.ERR_NO_ENVIRONMENT
    f.set_map(grid)
    assert code(f) == A.ERR_NOT_INITIALISED
    f.init_gaussian(256, [0.0, 0.0, 0.0], [0.1, 0.1, 0.05], 0.18, 0.05)
    # a NaN patch and an empty scan leave the map as it is
    bad = S.scan_patches()
    bad[17].position[2] = float("nan")
    assert code(f, bad) == A.ERR_INVALID_ARG
    assert_same_grid(f.get_map(), grid, "NaN patch")
    info = f.shared_map_update((A.ScanPatch * 0)())
    assert counters(info) == dict.fromkeys(COUNTERS, 0) | {"n_patches": grid.mean.shape[0]}
    assert_same_grid(f.get_map(), grid, "empty scan")
    # and a real scan still merges afterwards
    assert f.shared_map_update(scan).fused > 0
    f.close()


def test_shared_map_update_unsupported_on_a_sharded_filter(gpu_mod):
    """a world-size-1 eslam_gpu_set_comm filter: the merge is refused, loudly (no collective runs)"""
    n = 256
    cfg = S.bench_config(A.default_config(), n)
    f = gpu_mod.GpuFilter(cfg)
    ag = A.ALLGATHER_FN(lambda *a: 1)
    a2a = A.ALLTOALLV_FN(lambda *a: 1)
    comm = A.Comm(None, 0, 1, 0, 0, ag, a2a)
    bounds = (C.c_uint64 * 2)(0, n)
    f._check(f.L.eslam_gpu_set_comm(f.h, C.byref(comm), n, bounds))
    f.set_map(case_grid("flat"))
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.05], 0.18, 0.05)
    with pytest.raises(gpu_mod.EslamError) as e:
        f.shared_map_update(S.scan_patches())
    assert e.value.code == A.ERR_UNSUPPORTED and "sharded" in str(e.value)
    f.close()


def test_cpp_facade_shared_map():
    """EmbodiedSlamFilter::processMap(scan, match, true) with the shared map == the raw ABI"""
    sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
    import build_lib
    exe = build_lib.build_facade_test(verbose=False, name="test_facade_shared_map")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade shared map OK" in r.stdout
