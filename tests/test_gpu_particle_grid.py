"""A particle's whole map as one MLS grid, composed on the device (eslam_gpu_get_particle_grid,
eslam_gpu_adopt_particle_map): particles[i].grid.getMap() of the reference
(src/PoseEstimator.hpp:79-87).  The device's grid equals the numpy model (particle_grid_ref.py)
applied to the two older getters and to the oracle's maps, bit for bit; a shared-map filter
given the exported grid computes for particle i what the per-particle-maps filter computes
(the acceptance criterion); adopting a map equals exporting it and setting it."""
import ctypes as C

import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import synthetic as S
import particle_grid_ref as R
from parity_util import assert_bit_identical

pytestmark = pytest.mark.gpu

CELLS = 83                                   # the width: a multiple of neither 8 nor 32
MAP_INFO = ("map_patches_dropped", "map_stores_copied", "map_stores_changed", "map_patches_covered", "map_tiles_evicted")


def map_info(i):
    return tuple(int(getattr(i, f)) for f in MAP_INFO)


def corner_grid(case):
    """the prior with the origin 0.4 m from the grid's top left corner in x and in y: the
    windows of particles initialised at the origin overhang the grid on both sides"""
    side = CELLS * 0.1
    return R.prior_grid(case, CELLS, offset=(-0.4, 0.4 - side))


def maps_config(n, forced=True):
    cfg = S.bench_config(A.default_config(), n)
    if not forced:
        cfg.min_effective = 0
    cfg.flags |= A.FLAG_PARTICLE_MAPS | A.FLAG_RECORD_ANCESTORS
    cfg.local_map_pages = 48                 # the copies of covered cells and of shared tables
    return cfg


def check_against_models(gpu, orc, grid, idx, label):
    shared = gpu.get_map()
    assert R.grids_equal(shared, grid), label            # the shared grid itself never changes
    out = {}
    for i in idx:
        got = gpu.particle_grid(i)
        pm = gpu.particle_map(i)
        assert R.grids_equal(got, R.compose(pm, shared)), (label, i, "the device's own getters")
        if orc is not None:
            assert R.grids_equal(got, R.compose(orc.particle_map(i), grid)), (label, i, "the oracle's map")
        assert got.scale == grid.scale and got.offset == grid.offset and list(got.g2l) == list(grid.g2l)
        out[i] = (got, len(pm[0]))
    return out


@pytest.mark.parametrize("case", ["beyond", "mapped", "empty", "heights", "rotated_grid"])
def test_particle_grid_equals_model(gpu_mod, oracle, case):
    n = 600
    cfg = maps_config(n)
    grid = corner_grid(case)
    gpu = gpu_mod.GpuFilter(cfg)
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    for f in (gpu, orc):
        f.set_map(grid)
        f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.05], 0.18, 0.05)
    # before any map update a particle's map was never centred: the shared grid itself
    assert R.grids_equal(gpu.particle_grid(0), grid) and R.grids_equal(gpu.particle_grid(n - 1), grid)
    scan = S.scan_patches()
    stream = S.step_stream(14, tilt=True)
    for st in stream[:12]:
        assert gpu.step(st) == orc.step(st)
        gpu.map_update(scan)
        orc.map_update(scan)
    assert_bit_identical(gpu.download(), orc.download(), f"{case}: the mapping run")
    got = check_against_models(gpu, orc, grid, [0, 1, n // 2, n - 1], case)
    assert sum(k for _, k in got.values()) > 0           # own cells were composed in
    if case == "mapped":
        assert gpu.sync().map_patches_covered > 0        # copies of covered cells (the shadow flag)
    # a resample: two copies of one ancestor name one table, and export equal grids ...
    assert gpu.step(stream[12]) == orc.step(stream[12])
    anc = gpu.ancestors().astype(np.int64)
    assert np.array_equal(anc, orc.ancestors())
    i = int(np.argmax(np.diff(anc) == 0))
    assert anc[i] == anc[i + 1]
    two = check_against_models(gpu, orc, grid, [i, i + 1], case + " copies")
    assert R.grids_equal(two[i][0], two[i + 1][0])
    # ... until they move apart and a map update gives each its own table
    gpu.project(stream[13])
    orc.project(stream[13])
    gpu.map_update(scan)
    orc.map_update(scan)
    two = check_against_models(gpu, orc, grid, [i, i + 1], case + " copies, separated")
    assert not R.grids_equal(two[i][0], two[i + 1][0])
    gpu.close()


def test_particle_grid_with_trail(gpu_mod, oracle):
    """a 3 x 3-tile window (maxSensorRange 0.8 m) and a trail of 3 tiles, walked 2.4 m: the trail
    fills and forgets, and the export holds the trail's cells, outside the current window"""
    n = 512
    cfg = maps_config(n)
    cfg.max_sensor_range = 0.8
    cfg.local_map_trail = 3
    grid = R.prior_grid("beyond", CELLS)
    gpu = gpu_mod.GpuFilter(cfg)
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    for f in (gpu, orc):
        f.set_map(grid)
        f.init_gaussian(n, [0.0, 0.0, 0.0], [0.05, 0.05, 0.02], 0.18, 0.05)
    scan = S.scan_patches(nx=6, ny=5, x0=0.3, x1=0.7, y0=-0.6, y1=0.1)     # within 0.8 m
    evicted = dropped = 0
    for k, st in enumerate(S.step_stream(120, dx=0.02, dyaw=0.0)):
        assert gpu.step(st) == orc.step(st)
        gpu.map_update(scan)
        orc.map_update(scan)
        gi = gpu.sync()
        assert map_info(gi) == map_info(orc.info()), k
        evicted += gi.map_tiles_evicted
        dropped += gi.map_patches_dropped
    print("trail: tiles evicted", evicted, "patches dropped", dropped)
    assert evicted > 0 and dropped == 0
    idx = [0, 1, n // 2, n - 1]
    got = check_against_models(gpu, orc, grid, idx, "trail")
    # the window is the 3 x 3 tiles around the particle's tile at the last map update
    p = gpu.download()
    outside = 0
    for i in idx:
        g = got[i][0]
        cs, base = g.cell_start.astype(np.int64), grid.cell_start.astype(np.int64)
        cells = np.nonzero(np.diff(cs) > np.diff(base))[0]                 # the cells with an own patch
        assert len(cells) == got[i][1]
        ta, tb = (cells % CELLS) >> 3, (cells // CELLS) >> 3
        ca = int(np.floor((p.x[i] - grid.offset[0]) / grid.scale[0])) >> 3
        cb = int(np.floor((p.y[i] - grid.offset[1]) / grid.scale[1])) >> 3
        outside += int(np.sum((np.abs(ta - ca) > 1) | (np.abs(tb - cb) > 1)))
    assert outside > 0
    gpu.close()


@pytest.mark.parametrize("case", ["beyond", "mapped", "empty", "heights"])
def test_exported_grid_answers_like_the_particle(gpu_mod, case):
    """the equivalence on the device: set_map(particle_grid(i)) on a shared-map filter holding the
    same particles, one update on both: the eight local fields of particle i are equal"""
    n = 600
    cfg = maps_config(n, forced=False)
    grid = R.prior_grid(case, CELLS)
    gpu = gpu_mod.GpuFilter(cfg)
    gpu.set_map(grid)
    gpu.init_gaussian(n, [0.0, 0.0, 0.0], [0.05, 0.05, 0.02], 0.18, 0.05)
    scan = S.scan_patches()
    stream = S.step_stream(13, tilt=True)
    for st in stream[:12]:
        gpu.step(st)
        gpu.map_update(scan)
    st = stream[12]
    gpu.project(st)
    before = gpu.download()
    probes = (0, 1, n // 2, n - 1)
    grids = {i: gpu.particle_grid(i) for i in probes}
    gpu.update(st)
    assert gpu.sync().resampled == 0
    after = gpu.download()
    scfg = S.bench_config(A.default_config(), n)
    scfg.min_effective = 0
    shared = gpu_mod.GpuFilter(scfg)

    def answer(g):
        shared.set_map(g)
        shared.upload(before)
        shared.update(st)
        return shared.download()

    for i in probes:
        assert R.local_fields_equal(answer(grids[i]), after, i), (case, i)
    if case == "beyond":
        differ = 0
        for j in probes[1:]:
            got = answer(grids[j])
            differ += int(got.zpos[0] != after.zpos[0] or got.mprob[0] != after.mprob[0])
        print("beyond: other particles' grids that change particle 0:", differ)
        assert differ > 0
    shared.close()
    gpu.close()


def test_adopt_equals_export_then_set_map(gpu_mod):
    n = 600
    cfg = maps_config(n)
    grid = R.prior_grid("beyond", CELLS)
    a = gpu_mod.GpuFilter(cfg)
    a.set_map(grid)
    a.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.05], 0.18, 0.05)
    scan = S.scan_patches()
    stream = S.step_stream(20, tilt=True)
    for st in stream[:12]:
        a.step(st)
        a.map_update(scan)
    b = gpu_mod.GpuFilter(cfg)
    b.load_state(a.save_state())
    i = a.best_index()
    assert len(a.particle_map(i)[0]) > 0
    exported = b.particle_grid(i)
    a.adopt_particle_map(i)
    b.set_map(exported)
    assert R.grids_equal(a.get_map(), exported) and R.grids_equal(b.get_map(), exported)
    assert int(exported.cell_start[-1]) > int(grid.cell_start[-1])
    for f in (a, b):
        assert all(len(f.particle_map(k)[0]) == 0 for k in range(n))
        assert R.grids_equal(f.particle_grid(n // 2), exported)    # nothing of its own: the adopted grid
    for st in stream[12:18]:
        assert a.step(st) == b.step(st)
        a.map_update(scan)
        b.map_update(scan)
        assert map_info(a.sync()) == map_info(b.sync())
    assert_bit_identical(a.download(), b.download(), "adopt vs export + set_map")
    for k in (0, 1, n // 3, n - 1):
        assert R.grids_equal(a.particle_grid(k), b.particle_grid(k)), k
        ca, cb = a.particle_map(k), b.particle_map(k)
        assert all(np.array_equal(R.u32(x), R.u32(y)) for x, y in zip(ca, cb)), k
    # the adopting twin's state saves, loads and continues
    c = gpu_mod.GpuFilter(cfg)
    c.load_state(a.save_state())
    assert R.grids_equal(c.get_map(), a.get_map())
    for st in stream[18:20]:
        assert a.step(st) == c.step(st)
        a.map_update(scan)
        c.map_update(scan)
    assert_bit_identical(a.download(), c.download(), "adopt, save, load, continue")
    assert R.grids_equal(a.particle_grid(5), c.particle_grid(5))
    for f in (a, b, c):
        f.close()


def test_particle_grid_errors(gpu_mod):
    n = 300
    grid = R.prior_grid("beyond", CELLS)
    count = C.c_uint64()
    # no per-particle maps
    f = gpu_mod.GpuFilter(S.bench_config(A.default_config(), n))
    f.set_map(grid)
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.05, 0.05, 0.02], 0.18, 0.05)
    for call in (lambda: f.particle_grid(0), lambda: f.adopt_particle_map(0)):
        with pytest.raises(gpu_mod.EslamError) as e:
            call()
        assert e.value.code == A.ERR_INVALID_ARG
    f.close()
    # before set_map, and before the particles
    g = gpu_mod.GpuFilter(maps_config(n))
    assert g.L.eslam_gpu_particle_grid_size(g.h, 0, C.byref(count)) == A.ERR_NO_ENVIRONMENT
    assert g.L.eslam_gpu_adopt_particle_map(g.h, 0) == A.ERR_NO_ENVIRONMENT
    g.set_map(grid)
    assert g.L.eslam_gpu_particle_grid_size(g.h, 0, C.byref(count)) == A.ERR_NOT_INITIALISED
    assert g.L.eslam_gpu_adopt_particle_map(g.h, 0) == A.ERR_NOT_INITIALISED
    g.init_gaussian(n, [0.0, 0.0, 0.0], [0.05, 0.05, 0.02], 0.18, 0.05)
    for st in S.step_stream(3):
        g.step(st)
        g.map_update(S.scan_patches())
    # null pointers, the index
    assert g.L.eslam_gpu_particle_grid_size(g.h, 0, None) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_particle_grid_size(None, 0, C.byref(count)) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_get_particle_grid(g.h, 0, None, None, None, None, 1 << 20) == A.ERR_INVALID_ARG
    for call in (lambda: g.particle_grid(n), lambda: g.adopt_particle_map(n)):
        with pytest.raises(gpu_mod.EslamError) as e:
            call()
        assert e.value.code == A.ERR_INVALID_ARG
    # a capacity one too small: refused, and nothing changed
    whole = g.particle_grid(1)
    k = int(whole.cell_start[-1])
    assert k > int(grid.cell_start[-1])
    with pytest.raises(gpu_mod.EslamError) as e:
        g.particle_grid(1, capacity=k - 1)
    assert e.value.code == A.ERR_INVALID_ARG
    assert R.grids_equal(g.get_map(), grid) and R.grids_equal(g.particle_grid(1), whole)
    assert R.grids_equal(g.particle_grid(1, capacity=k + 5), whole)
    g.close()
    # a sharded filter (one rank, collectives that fail): adopt is refused before any collective,
    # the export is rank-local and works
    s = gpu_mod.GpuFilter(maps_config(n))
    ag = A.ALLGATHER_FN(lambda *a: 1)
    a2a = A.ALLTOALLV_FN(lambda *a: 1)
    comm = A.Comm(None, 0, 1, 0, 0, ag, a2a)
    bounds = (C.c_uint64 * 2)(0, n)
    s._check(s.L.eslam_gpu_set_comm(s.h, C.byref(comm), n, bounds))
    s.set_map(grid)
    s.init_gaussian(n, [0.0, 0.0, 0.0], [0.05, 0.05, 0.02], 0.18, 0.05)
    with pytest.raises(gpu_mod.EslamError) as e:
        s.adopt_particle_map(0)
    assert e.value.code == A.ERR_UNSUPPORTED and "sharded" in str(e.value)
    assert R.grids_equal(s.particle_grid(0), grid)
    s.close()
