"""The scan MLS built on the GPU from a laser scan or a depth image (eslam_gpu_scan_from_laser /
eslam_gpu_scan_from_depth): every case equals the sequential C reference
(tests/c/scan_ref.c, itself checked against a numpy model in tests/test_scan_ref.py) bit for bit
-- the patches, their order and the counters -- and the device-built patches drive the map
updates to the same particles, maps and counters as the oracle given the same patches."""
import ctypes as C

import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import scan_ref as SR
import shared_map_ref as R
import synthetic as S
from parity_util import assert_bit_identical
from test_gpu_particle_maps import assert_maps_equal, map_info
from test_gpu_shared_map import assert_same_grid, counters

pytestmark = pytest.mark.gpu

N = 5003                                  # not a multiple of 64


def build(f, rd):
    """the device's scan of a Reading: ((n, 4) float64 patches, ScanInfo)"""
    if rd.kind == "laser":
        out, info = f.scan_from_laser(rd.ranges, rd.start_angle, rd.angular_resolution, rd.min_range, rd.max_range, rd.params)
    else:
        out, info = f.scan_from_depth(rd.data, rd.scale_x, rd.scale_y, rd.center_x, rd.center_y, rd.params)
    assert len(out) == info.patches
    return SR.patches_array(out), info


def assert_same_scan(got, ginfo, want, winfo, label):
    assert ginfo.as_dict() == winfo.as_dict(), label
    assert got.shape == want.shape, label
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (label, np.abs(got - want).max())


@pytest.fixture(scope="module")
def refs():
    return {name: SR.reference(rd) for name, rd in SR.cases().items()}


@pytest.fixture()
def bare(gpu_mod):
    """a context with no map and no particles"""
    f = gpu_mod.GpuFilter(S.bench_config(A.default_config(), 64))
    yield f
    f.close()


@pytest.mark.parametrize("name", list(SR.cases()))
def test_scan_bit_exact(bare, refs, name):
    want, winfo, sizes = refs[name]
    got, ginfo = build(bare, SR.cases()[name])
    print(name, ginfo.as_dict(), "largest cluster", int(sizes.max()) if sizes.size else 0)
    assert_same_scan(got, ginfo, want, winfo, name)
    if name == "no_point":
        assert ginfo.patches == 0 and got.shape == (0, 4)
    if name == "one_point":
        assert ginfo.patches == 1


def test_scan_twice_and_scratch_reuse(bare, refs):
    """the same reading twice gives the same bytes; a small laser build after a large depth build
    on one context gives the laser's result (nothing of the larger build is left in the scratch)"""
    cs = SR.cases()
    a, ai = build(bare, cs["depth_301x233"])
    b, bi = build(bare, cs["depth_301x233"])
    assert a.tobytes() == b.tobytes() and ai.as_dict() == bi.as_dict()
    for name in ("laser_67", "one_point", "laser_1081", "no_point", "two_levels"):
        got, ginfo = build(bare, cs[name])
        assert_same_scan(got, ginfo, refs[name][0], refs[name][1], name)
    # the patches stay with the context until the next build
    again = SR.patches_array(bare.scan_patches())
    assert np.array_equal(again.view(np.uint64), refs["two_levels"][0].view(np.uint64))


def test_scan_params_default(bare):
    p = bare.scan_params()
    q = SR.params_default(bare.cfg.max_sensor_range)
    assert bytes(p) == bytes(q)
    assert p.min_sigma == 1e-3 and p.resolution == 0.05 and p.patch_thickness == 0.1
    assert list(p.sensor_rot_sigma) == [np.deg2rad(5.0), 0.0, 0.0] and list(p.body_rot_sigma)[2] == 0.0


def test_scan_invalid_arguments(gpu_mod, bare, refs):
    """every refused argument: ESLAM_ERR_INVALID_ARG with a message, and the context goes on working"""
    f, L = bare, bare.L
    rd = SR.cases()["laser_67"]
    img = SR.cases()["depth_61x47"]
    ls, _k1 = rd.c_reading()
    im, _k2 = img.c_reading()
    info = A.ScanInfo()

    def refused(rc):
        assert rc == A.ERR_INVALID_ARG
        assert len(L.eslam_gpu_last_error(f.h)) > 0
        got, ginfo = build(f, rd)                            # still usable
        assert_same_scan(got, ginfo, refs["laser_67"][0], refs["laser_67"][1], "after a refusal")

    # null pointers
    refused(L.eslam_gpu_scan_from_laser(f.h, None, C.byref(rd.params), C.byref(info)))
    refused(L.eslam_gpu_scan_from_laser(f.h, C.byref(ls), None, C.byref(info)))
    refused(L.eslam_gpu_scan_from_depth(f.h, None, C.byref(img.params), C.byref(info)))
    refused(L.eslam_gpu_scan_from_depth(f.h, C.byref(im), None, C.byref(info)))
    nul = A.LaserScan.from_buffer_copy(bytes(ls))
    nul.ranges = None
    refused(L.eslam_gpu_scan_from_laser(f.h, C.byref(nul), C.byref(rd.params), C.byref(info)))
    nim = A.DepthImage.from_buffer_copy(bytes(im))
    nim.data = None
    refused(L.eslam_gpu_scan_from_depth(f.h, C.byref(nim), C.byref(img.params), C.byref(info)))
    refused(L.eslam_gpu_scan_patches(f.h, None, 0, None))
    assert L.eslam_gpu_scan_from_laser(None, C.byref(ls), C.byref(rd.params), C.byref(info)) == A.ERR_INVALID_ARG
    # a zero-size image
    for w, h in ((0, 47), (61, 0)):
        z = A.DepthImage.from_buffer_copy(bytes(im))
        z.width, z.height = w, h
        refused(L.eslam_gpu_scan_from_depth(f.h, C.byref(z), C.byref(img.params), C.byref(info)))
    # non-finite transforms and sigmas; sizes that are not positive
    def with_field(field, value, index=None):
        p = A.ScanParams.from_buffer_copy(bytes(rd.params))
        if index is None:
            setattr(p, field, value)
        else:
            getattr(p, field)[index] = value
        return p

    bad = [with_field("sensor2body", float("nan"), 3), with_field("sensor2body", float("inf"), 4),
           with_field("orientation", float("nan"), 0), with_field("sensor_rot_sigma", float("inf"), 0),
           with_field("body_rot_sigma", float("nan"), 1), with_field("min_sigma", 0.0), with_field("min_sigma", -1e-3),
           with_field("min_sigma", float("nan")), with_field("resolution", 0.0), with_field("resolution", -0.05),
           with_field("patch_thickness", 0.0), with_field("patch_thickness", float("nan")),
           with_field("max_sensor_range", 0.0), with_field("max_sensor_range", -3.0),
           with_field("max_sensor_range", float("inf")), with_field("resolution", 1e-9)]
    for p in bad:
        refused(L.eslam_gpu_scan_from_laser(f.h, C.byref(ls), C.byref(p), C.byref(info)))
        assert info.patches == 0
    refused(L.eslam_gpu_scan_from_depth(f.h, C.byref(im), C.byref(bad[0]), C.byref(info)))
    with pytest.raises(gpu_mod.EslamError) as e:
        f.scan_from_depth(np.zeros((0, 5), np.float32), 0.01, 0.01, 0.0, 0.0)
    assert e.value.code == A.ERR_INVALID_ARG and "zero-size" in str(e.value)


def test_scan_on_a_sharded_filter(gpu_mod, refs):
    """a world-size-1 eslam_gpu_set_comm filter builds the same scan (rank-local, no collective runs)"""
    n = 256
    f = gpu_mod.GpuFilter(S.bench_config(A.default_config(), n))
    ag = A.ALLGATHER_FN(lambda *a: 1)
    a2a = A.ALLTOALLV_FN(lambda *a: 1)
    comm = A.Comm(None, 0, 1, 0, 0, ag, a2a)
    bounds = (C.c_uint64 * 2)(0, n)
    f._check(f.L.eslam_gpu_set_comm(f.h, C.byref(comm), n, bounds))
    got, ginfo = build(f, SR.cases()["depth_61x47"])
    assert_same_scan(got, ginfo, refs["depth_61x47"][0], refs["depth_61x47"][1], "sharded")
    f.close()


def scan_readings():
    cs = SR.cases()
    return [cs["depth_61x47"], cs["laser_1081"], cs["two_levels"]]


@pytest.mark.parametrize("prior", ["rough", "unmapped", "rect", "rect_rotated"])
def test_scan_drives_particle_maps(gpu_mod, oracle, prior):
    """per-particle maps: device-built patches into eslam_gpu_map_match / eslam_gpu_map_update over
    three steps == the oracle given the reference's patches (particles, sampled maps, counters)"""
    cfg = S.bench_config(A.default_config(), N)
    cfg.flags |= A.FLAG_PARTICLE_MAPS | A.FLAG_RECORD_ANCESTORS
    cfg.local_map_pages = 128                  # the laser's fan reaches most of a window's 81 tiles (default pool: 16 a particle)
    grid = S.rough_map(cells=120)
    if prior == "unmapped":                    # the scans' cells are the maps' own beyond x = 0.3
        grid = S.unmapped_beyond(grid, 0.3)
    if prior.startswith("rect"):               # 150 x 110 cells of 0.10 x 0.08 m: a 9 x 11-tile window
        import rect_grids
        grid = rect_grids.rect_prior("beyond", (0.10, 0.08), yaw=0.3 if prior == "rect_rotated" else None)
    gpu = gpu_mod.GpuFilter(cfg)
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    for f in (gpu, orc):
        f.set_map(grid)
        f.init_gaussian(N, [0.0, 0.0, 0.0], [0.05, 0.05, 0.02], 0.18, 0.05)
    written = 0
    for k, (st, rd) in enumerate(zip(S.step_stream(3, tilt=True), scan_readings())):
        assert gpu.step(st) == orc.step(st)
        if rd.kind == "laser":
            scan, sinfo = gpu.scan_from_laser(rd.ranges, rd.start_angle, rd.angular_resolution, rd.min_range, rd.max_range,
                                              rd.params)
        else:
            scan, sinfo = gpu.scan_from_depth(rd.data, rd.scale_x, rd.scale_y, rd.center_x, rd.center_y, rd.params)
        want, winfo = SR.reference_patches(rd)
        assert bytes(scan) == bytes(want) and sinfo.as_dict() == winfo.as_dict() and len(scan) > 1
        if k >= 1:
            gpu.map_match(scan)
            orc.map_match(want)
        gpu.map_update(scan)
        orc.map_update(want)
        gi = gpu.sync()
        assert_bit_identical(gpu.download(), orc.download(), f"{prior} step {k}")
        assert map_info(gi) == map_info(orc.info()), (prior, k, map_info(gi), map_info(orc.info()))
        written += gi.map_cells_written
    assert np.array_equal(gpu.ancestors(), orc.ancestors())
    assert_maps_equal(gpu, orc, list(range(0, N, N // 40)) + [N - 1], prior)
    if prior == "unmapped":
        assert written > 0                     # a no-op cannot pass
    gpu.close()


def test_scan_drives_the_shared_map(gpu_mod, oracle):
    """the shared map: device-built patches into eslam_gpu_shared_map_update over three steps ==
    the sequential reference merge of the reference's patches, and the steps on the merged grid"""
    cfg = S.bench_config(A.default_config(), N)
    cfg.flags |= A.FLAG_RECORD_ANCESTORS
    grid = S.rough_map(cells=120)
    gpu = gpu_mod.GpuFilter(cfg)
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    for f in (gpu, orc):
        f.set_map(grid)
        f.init_gaussian(N, [0.0, 0.0, 0.0], [0.1, 0.1, 0.05], 0.18, 0.05)
    cur = grid
    changed = 0
    stream = S.step_stream(4, tilt=True)
    for k, (st, rd) in enumerate(zip(stream, scan_readings())):
        assert gpu.step(st) == orc.step(st)
        assert_bit_identical(gpu.download(), orc.download(), f"shared step {k}")
        if rd.kind == "laser":
            scan, _ = gpu.scan_from_laser(rd.ranges, rd.start_angle, rd.angular_resolution, rd.min_range, rd.max_range, rd.params)
        else:
            scan, _ = gpu.scan_from_depth(rd.data, rd.scale_x, rd.scale_y, rd.center_x, rd.center_y, rd.params)
        want, _ = SR.reference_patches(rd)
        info = gpu.shared_map_update(scan)
        cur, winfo = R.merge(cur, orc.download(), want)
        assert_same_grid(gpu.get_map(), cur, f"shared step {k}")
        assert counters(info) == counters(winfo), k
        changed += info.fused + info.inserted
        orc.set_map(cur)
    assert changed > 0
    assert gpu.step(stream[3]) == orc.step(stream[3])          # a step on the grid the last merge left
    assert_bit_identical(gpu.download(), orc.download(), "shared, after the last merge")
    assert np.array_equal(gpu.ancestors(), orc.ancestors())
    gpu.close()
