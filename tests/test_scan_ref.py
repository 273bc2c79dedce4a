"""The scan MLS contract on the CPU: the C reference (tests/c/scan_ref.c) against an
independent numpy model of the same rule on every input the GPU tests use, and the closed forms
the rule implies.

The model takes two primitives from outside numpy, so that every value can be compared bit for
bit: the contract's dm_sincos (through the reference library; tests/test_detmath.py checks it) for
the beam angles, and the C library's cos / sin / atan2 (Python's math) for removeYaw, as the
library's host side uses them.  Everything else is IEEE + - * / sqrt floor in the contract's
order; the cluster sums are plain Python floats, added one by one.  The comparison is exact (no
ulp allowance was needed)."""
import math

import numpy as np
import pytest

import scan_ref as SR


# ---- the numpy model -----------------------------------------------------------------------
def q_to_mat(q):
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def remove_yaw(q):
    R = q_to_mat(q)
    yaw = math.atan2(R[1, 0], R[0, 0]) if math.sqrt(R[2, 2] * R[2, 2] + R[2, 1] * R[2, 1]) > 1e-12 else 0.0
    ha = 0.5 * -yaw
    s = math.sin(ha)
    a = (math.cos(ha), s * 0.0, s * 0.0, s * 1.0)
    b = q
    return q_to_mat((a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]))


def model(rd):
    """(patches (n, 4), info dict, points per cluster) of a Reading, by the rule of DESIGN.md 5f"""
    p = rd.params
    S = np.array(list(p.sensor2body)).reshape(3, 4)
    Rs, ts = S[:, :3], S[:, 3]
    Rw = remove_yaw(tuple(p.orientation))
    res, thick, rmax = p.resolution, p.patch_thickness, p.max_sensor_range
    # the points in the sensor frame
    if rd.kind == "laser":
        mm = np.asarray(rd.ranges, np.uint32)
        n = mm.size
        ok = (mm > 5) & (mm >= rd.min_range) & (mm <= rd.max_range)
        r = mm.astype(np.float64) * 1e-3
        far = ok & (r > rmax)
        ang = rd.start_angle + np.arange(n, dtype=np.float64) * rd.angular_resolution
        sc = np.array([SR.sincos(a) for a in ang]).reshape(n, 2)
        q = np.stack([r * sc[:, 1], r * sc[:, 0], np.zeros(n)])
        ray = 1.0
    else:
        img = np.asarray(rd.data, np.float32)
        h, w = img.shape
        n = img.size
        d = img.reshape(-1).astype(np.float64)
        ok = np.isfinite(d) & (d > 0.0)
        far = ok & (d > rmax)
        idx = np.arange(n)
        u, v = (idx % w).astype(np.float64), (idx // w).astype(np.float64)
        dz = np.where(ok, d, 0.0)
        q = np.stack([(u * rd.scale_x + rd.center_x) * dz, (v * rd.scale_y + rd.center_y) * dz, dz])
        xm = max(abs(rd.center_x), abs((w - 1.0) * rd.scale_x + rd.center_x))
        ym = max(abs(rd.center_y), abs((h - 1.0) * rd.scale_y + rd.center_y))
        ray = math.sqrt((xm * xm + ym * ym) + 1.0)
    info = {"points": n, "points_invalid": int((~ok).sum()), "points_out_of_range": int(far.sum())}
    keep = ok & ~far
    # placement
    b = [((Rs[k, 0] * q[0] + Rs[k, 1] * q[1]) + Rs[k, 2] * q[2]) + ts[k] for k in range(3)]
    pw = [(Rw[k, 0] * b[0] + Rw[k, 1] * b[1]) + Rw[k, 2] * b[2] for k in range(3)]
    # the height's variance: first-order in the six rotation errors
    a = [(Rw[2, 0] * Rs[0, c] + Rw[2, 1] * Rs[1, c]) + Rw[2, 2] * Rs[2, c] for c in range(3)]

    def row_cross(r, v):                                   # r . (e_k x v) for k = x, y, z
        return [r[2] * v[1] - r[1] * v[2], r[0] * v[2] - r[2] * v[0], r[1] * v[0] - r[0] * v[1]]

    g = row_cross(a, q) + row_cross(Rw[2], b)
    sig = list(p.sensor_rot_sigma) + list(p.body_rot_sigma)
    var = np.zeros(n)
    for k in range(6):
        term = (sig[k] * sig[k]) * (g[k] * g[k])
        var = term if k == 0 else var + term
    var = np.maximum(var, p.min_sigma * p.min_sigma)
    # cells on the grid the host sizes
    inv = 1.0 / res
    tn = math.sqrt((ts[0] * ts[0] + ts[1] * ts[1]) + ts[2] * ts[2])
    half = int(math.floor((rmax * ray + tn) * inv) + 2.0)
    width = 2 * half
    mx = np.floor(pw[0] * inv) + half
    my = np.floor(pw[1] * inv) + half
    on = (mx >= 0) & (mx < width) & (my >= 0) & (my < width)
    info["points_out_of_range"] += int((keep & ~on).sum())
    keep &= on
    info["points_valid"] = int(keep.sum())
    ids = np.nonzero(keep)[0]
    cell = (my[ids] * width + mx[ids]).astype(np.int64)
    zf = pw[2][ids].astype(np.float32) + np.float32(0.0)   # -0 -> +0
    order = np.lexsort((ids, zf, cell))                     # cell, then (float) z, then index
    ids, cell = ids[order], cell[order]
    z, vr = pw[2][ids], var[ids]
    patches, sizes = [], []
    cells = 0
    j0 = 0
    m = ids.size
    while j0 < m:
        j1 = j0
        while j1 < m and cell[j1] == cell[j0]:
            j1 += 1
        cells += 1
        cx = ((float(cell[j0] % width) - half) + 0.5) * res
        cy = ((float(cell[j0] // width) - half) + 0.5) * res
        k = j0
        while k < j1:
            e = k + 1
            while e < j1 and z[e] - z[e - 1] <= thick:
                e += 1
            sw = swz = 0.0
            for t in range(k, e):
                wt = 1.0 / float(vr[t])
                sw = sw + wt
                swz = swz + wt * float(z[t])
            mu = swz / sw
            sd = 0.0
            for t in range(k, e):
                wt = 1.0 / float(vr[t])
                dd = float(z[t]) - mu
                sd = sd + wt * (dd * dd)
            patches.append((cx, cy, mu, math.sqrt(1.0 / sw + sd / sw)))
            sizes.append(e - k)
            k = e
        j0 = j1
    info["cells"] = cells
    info["patches"] = len(patches)
    return np.array(patches, np.float64).reshape(-1, 4), info, np.array(sizes, np.uint32)


# ---- the reference against the model, on every input of the GPU tests -----------------------
@pytest.fixture(scope="module")
def refs():
    return {name: SR.reference(rd) for name, rd in SR.cases().items()}


@pytest.mark.parametrize("name", list(SR.cases()))
def test_reference_equals_numpy_model(refs, name):
    ref, info, sizes = refs[name]
    mod, minfo, msizes = model(SR.cases()[name])
    assert info.as_dict() == minfo
    assert np.array_equal(sizes, msizes)
    assert ref.shape == mod.shape
    assert np.array_equal(ref.view(np.uint64), mod.view(np.uint64)), np.abs(ref - mod).max()


def test_case_list_preconditions(refs):
    """what the GPU cases must exercise, asserted on the reference so no test passes vacuously"""
    def cells_with(ref, k):
        _, cnt = np.unique(ref[:, :2], axis=0, return_counts=True)
        return int((cnt >= k).sum())

    assert any(cells_with(r[0], 2) > 0 for r in refs.values())
    assert cells_with(refs["two_levels"][0], 2) > 0
    assert any((r[2] > 64).any() for r in refs.values())
    assert refs["one_cell"][2].tolist() == [5000]
    assert refs["depth_301x233"][1].points_valid > 65536          # more than one sort block of any size in use
    for name in ("laser_1081", "depth_61x47"):
        assert refs[name][1].points_invalid > 0, name
        assert refs[name][1].points_out_of_range > 0, name
    i = refs["laser_1081"][1]
    assert i.points == 1081 and i.points_valid + i.points_invalid + i.points_out_of_range == 1081
    assert refs["laser_67"][1].points == 67 and refs["laser_67"][1].patches > 0
    assert refs["depth_61x47"][1].points_invalid >= 5            # NaN, inf, -inf, 0, negative
    assert refs["no_point"][1].patches == 0 and refs["no_point"][1].points_valid == 0
    assert refs["one_point"][1].points_valid == 1 and refs["one_point"][1].patches == 1
    # patches come out by cell index (y-major), then by height
    for name, (ref, _, _) in refs.items():
        key = list(zip(ref[:, 1], ref[:, 0], ref[:, 2]))
        assert key == sorted(key), name


# ---- the reference's patches on a grid that is square in neither sense -----------------------
@pytest.mark.parametrize("yaw", [None, 0.7])
@pytest.mark.parametrize("name", ["laser_1081", "depth_61x47", "two_levels"])
def test_reference_patches_on_a_rectangular_grid(oracle, name, yaw):
    """The scan MLS has a square grid of its own; the map it is merged into need not be.  The
    reference's patches, merged by the oracle into three particles' maps on 150 x 110 cells of
    0.10 x 0.08 m (empty prior; identity and rotated global2local), fill the cells numpy's
    floor((l - offset) / scale) names per axis, n * width + m, inside the particle's 9 x 11-tile
    window; the patches beyond it are the ones counted as dropped.  A patch closer than 1e-6 of a
    cell to a border may land on either side (the oracle multiplies by 1 / scale)."""
    import eslam_abi as A
    import oracle_ffi as O
    import rect_grids as G
    import synthetic as S
    scale, (hx, hy) = G.RECT_CASES["9x11"]
    grid = G.rect_prior("empty", scale, yaw=yaw)
    scan, _ = SR.reference_patches(SR.cases()[name])
    assert len(scan) > 0
    pa = A.ParticleArrays(3)
    pa.x[:], pa.y[:], pa.orientation[:] = [0.013, -0.431, 0.377], [0.021, 0.263, -0.305], [0.0, 0.4, -1.1]
    pa.zpos[:], pa.zsigma[:], pa.weight[:] = 0.18, 0.05, 1.0 / 3
    cfg = S.bench_config(A.default_config(), 3)
    cfg.flags |= A.FLAG_PARTICLE_MAPS
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    orc.set_map(grid)
    orc.upload(pa)
    orc.map_update(scan)
    sx = np.array([s.position[0] for s in scan])
    sy = np.array([s.position[1] for s in scan])
    sz = np.array([s.position[2] for s in scan])
    dropped = filled = 0
    for i in range(3):
        co, sn = math.cos(pa.orientation[i]), math.sin(pa.orientation[i])
        lx, ly = G.to_local(grid, co * sx - sn * sy + pa.x[i], sn * sx + co * sy + pa.y[i], sz + pa.zpos[i])
        m, n = G.cell_coords(grid, lx, ly)
        pm, pn = G.cell_coords(grid, *G.to_local(grid, pa.x[i], pa.y[i], pa.zpos[i]))
        assert min(abs(pm - round(pm)), abs(pn - round(pn))) > 1e-6
        ca, cb = int(math.floor(pm)) >> 3, int(math.floor(pn)) >> 3
        fm, fn = np.floor(m).astype(np.int64), np.floor(n).astype(np.int64)
        on = (fm >= 0) & (fm < grid.width) & (fn >= 0) & (fn < grid.height)
        inside = on & (np.abs((fm >> 3) - ca) <= hx) & (np.abs((fn >> 3) - cb) <= hy)
        sure = (np.abs(m - np.round(m)) > 1e-6) & (np.abs(n - np.round(n)) > 1e-6)
        assert sure.mean() > 0.99
        got = set(orc.particle_map(i)[0].astype(np.int64).tolist())
        must = set((fn * grid.width + fm)[inside & sure].tolist())
        may = set((fn * grid.width + fm)[inside].tolist())
        for dm_ in (-1, 0, 1):                             # a border patch: the neighbouring cell
            for dn in (-1, 0, 1):
                may |= set(((fn + dn) * grid.width + fm + dm_)[on & ~sure].tolist())
        assert must <= got <= may, (name, yaw, i, len(must - got), len(got - may))
        dropped += int(np.count_nonzero(on & ~inside))
        filled += len(got)
    assert filled > 0
    if all_sure(grid, pa, scan):                           # no patch near a border: the count is exact
        assert orc.info().map_patches_dropped == dropped


def all_sure(grid, pa, scan):
    """every patch of every particle keeps off the cell borders (then the dropped count is exact)"""
    import rect_grids as G
    sx = np.array([s.position[0] for s in scan])
    sy = np.array([s.position[1] for s in scan])
    sz = np.array([s.position[2] for s in scan])
    for i in range(pa.n):
        co, sn = math.cos(pa.orientation[i]), math.sin(pa.orientation[i])
        lx, ly = G.to_local(grid, co * sx - sn * sy + pa.x[i], sn * sx + co * sy + pa.y[i], sz + pa.zpos[i])
        m, n = G.cell_coords(grid, lx, ly)
        if not ((np.abs(m - np.round(m)) > 1e-6) & (np.abs(n - np.round(n)) > 1e-6)).all():
            return False
    return True


# ---- closed forms --------------------------------------------------------------------------
H = 0.37


def _level_laser(angles_mm, rpy=(0.0, 0.0, 0.0), **kw):
    """a laser with an identity rotation, H below the body's origin, on a body with attitude rpy"""
    start, res, mm = angles_mm
    p = SR.make_params(np.eye(3), (0.0, 0.0, -H), rpy, **kw)
    return SR.Reading("closed", "laser", p, ranges=np.asarray(mm, np.uint32), start_angle=start, angular_resolution=res,
                      min_range=20, max_range=30000)


def test_flat_floor_level_body():
    rng = np.random.default_rng(11)
    mm = rng.integers(300, 2900, 500)
    ref, info, sizes = SR.reference(_level_laser((-2.0, 0.008, mm)))
    assert info.points_valid == 500 and info.patches > 100
    # a weighted mean of L equal heights: L products, L - 1 sums and a division, each rounded once
    assert np.abs(ref[:, 2] + H).max() <= (int(sizes.max()) + 1) * np.finfo(float).eps * H


def test_variance_of_a_point_ahead():
    """body (x, 0, -h), level: only the body's pitch term is left, var = sigma_by^2 x^2; one point
    in the patch, so stdev^2 = var"""
    for x_mm in (410, 1010, 2760):
        ref, info, _ = SR.reference(_level_laser((0.0, 0.0, [x_mm])))
        assert info.patches == 1
        x = x_mm * 1e-3
        sby = math.radians(3.0)
        assert ref[0, 3] == pytest.approx(sby * x, rel=1e-14)
        assert ref[0, 2] == pytest.approx(-H, rel=1e-15)
        assert ref[0, 0] == (math.floor(x / 0.05) + 0.5) * 0.05 and ref[0, 1] == 0.025


def test_variance_floor():
    """without rotation sigmas the variance is min_sigma^2"""
    rd = _level_laser((0.3, 0.0, [1000]), sensor_rot_sigma=(0.0, 0.0, 0.0), body_rot_sigma=(0.0, 0.0, 0.0), min_sigma=2e-3)
    ref, _, _ = SR.reference(rd)
    assert ref[0, 3] == pytest.approx(2e-3, rel=1e-15)


def test_tilted_body_moves_the_height():
    """p = R_w b: pitch and roll move the height, yaw does not"""
    roll, pitch = 0.11, -0.07
    x = 1.25
    ref, _, _ = SR.reference(_level_laser((0.0, 0.0, [1250]), rpy=(roll, pitch, 0.0)))
    Rw = SR.rot_rpy(roll, pitch, 0.0)
    assert ref[0, 2] == pytest.approx(Rw[2, 0] * x + Rw[2, 2] * -H, rel=1e-13)
    assert abs(ref[0, 2] + H) > 0.05
    yawed, _, _ = SR.reference(_level_laser((0.0, 0.0, [1250]), rpy=(roll, pitch, 1.3)))
    assert yawed[0, 2] == pytest.approx(ref[0, 2], rel=1e-13)
    assert yawed[0, 0] == ref[0, 0] and yawed[0, 1] == ref[0, 1]


def test_two_surfaces_in_one_cell(refs):
    two, _, sizes2 = refs["two_levels"]
    one, _, sizes1 = refs["one_level"]
    assert two.shape[0] == 2 and sizes2.tolist() == [288, 288]
    assert two[0, 0] == two[1, 0] and two[0, 1] == two[1, 1]
    assert two[1, 2] - two[0, 2] == pytest.approx(0.2, abs=1e-6)
    assert one.shape[0] == 1 and sizes1.tolist() == [576]


def test_equal_keys_keep_point_order():
    """Equal (float) heights: the cluster's sums run in point-index order.  The variances differ
    from point to point, so another order would round differently; the model sums in index order."""
    rd = SR.cases()["equal_keys"]
    ref, info, sizes = SR.reference(rd)
    assert sizes.tolist() == [700] and info.cells == 1
    mod, _, _ = model(rd)
    assert np.array_equal(ref.view(np.uint64), mod.view(np.uint64))
    # the same points fed backwards: same set of (z, var), another order -- and other bits
    back = SR.Reading("back", "laser", rd.params, ranges=rd.ranges, start_angle=rd.start_angle + 699 * rd.angular_resolution,
                      angular_resolution=-rd.angular_resolution, min_range=20, max_range=30000)
    rb, _, _ = SR.reference(back)
    assert rb[0, 2] == ref[0, 2] == 0.0
    assert rb[0, 3] == pytest.approx(ref[0, 3], rel=1e-12)


def test_invalid_parameters_are_refused():
    rd = SR.cases()["laser_67"]
    for field, value in (("resolution", 0.0), ("patch_thickness", -1.0), ("max_sensor_range", 0.0), ("min_sigma", 0.0),
                         ("min_sigma", float("nan")), ("resolution", 1e-9)):
        p = SR.make_params()
        setattr(p, field, value)
        bad = SR.Reading("bad", "laser", p, ranges=rd.ranges, start_angle=0.0, angular_resolution=0.01, min_range=20,
                         max_range=30000)
        with pytest.raises(RuntimeError):
            SR.reference(bad)


def test_scan_struct_layouts_match_ctypes(tmp_path):
    """the ctypes mirrors of the scan structs have the C layouts (as tests/test_abi.py checks the others)"""
    import os
    import subprocess

    import eslam_abi as A
    structs = {"eslam_scan_params": A.ScanParams, "eslam_laser_scan": A.LaserScan, "eslam_depth_image": A.DepthImage,
               "eslam_scan_info": A.ScanInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eslam_gpu.h"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{os.path.join(SR.ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    out = dict(ln.rsplit(" ", 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.split("\n") if ln)
    import ctypes
    for cname, py in structs.items():
        assert int(out[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, f"{cname}.{f}"
