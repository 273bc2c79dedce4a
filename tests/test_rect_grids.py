"""The per-axis rules of the per-particle maps on the CPU, on grids that are square in neither
sense (tests/rect_grids.py): the oracle against plain numpy in float64.  The oracle and the
kernels share include/eslam_detmath.h, so GPU == oracle cannot show a rule that is wrong in
both; these tests pin the oracle first.

* the window's half widths per axis (dm_lm_half) and the words of a device table's row
  (dm_lm_row_words) against their formulas;
* the window's reach per axis: a scan patch just inside maxSensorRange is never dropped, one
  more than h + 1 tiles away always is -- x and y separately, on 0.10 x 0.08 m and
  0.08 x 0.10 m cells, so a swapped hx / hy fails one of the two;
* cell placement: the cells of a particle's map after one map update on an empty prior are
  floor((l - offset) / scale) per axis, flattened n * width + m."""
import math

import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import rect_grids as G
import synthetic as S

DM_LM_HALF, DM_LM_ROW_WORDS = 28, 29          # or_dm selectors


def half_formula(r, scale):
    return min(max(math.ceil(r / (8.0 * scale)), 1), 15)


@pytest.mark.parametrize("name", list(G.RECT_CASES))
def test_window_halves(oracle, name):
    (sx, sy), (hx, hy) = G.RECT_CASES[name]
    assert (half_formula(G.RANGE, sx), half_formula(G.RANGE, sy)) == (hx, hy)
    assert (int(oracle.dm(DM_LM_HALF, G.RANGE, sx)), int(oracle.dm(DM_LM_HALF, G.RANGE, sy))) == (hx, hy)
    assert sx != sy and hx != hy
    W = (2 * hx + 1) * (2 * hy + 1)
    assert W % 4 == (3 if name in G.MIXED_PARITY else 1)
    assert name == f"{2 * hx + 1}x{2 * hy + 1}"


def test_half_clamps(oracle):
    assert int(oracle.dm(DM_LM_HALF, 3.0, 10.0)) == 1 and int(oracle.dm(DM_LM_HALF, 0.0, 0.1)) == 1
    assert int(oracle.dm(DM_LM_HALF, 100.0, 0.1)) == 15
    assert int(oracle.dm(DM_LM_HALF, 3.2, 0.1)) == 4             # exactly 4 tiles: no extra one


def test_row_words(oracle):
    """S = ((W + 2 + 3) & ~3) + 4 V: whole 16-byte words, room for the two bookkeeping words
    behind the W window slots for every (hx, hy), never a 16-byte word more than that needs,
    and -- the property the benchmark rests on -- for W = 1 (mod 4), which every window with
    hx and hy of one parity has (square cells among them), the same S as padding W alone."""
    for hx in range(1, 16):
        for hy in range(1, 16):
            W = (2 * hx + 1) * (2 * hy + 1)
            assert W % 4 == (1 if hx % 2 == hy % 2 else 3)
            for V in (0, 2, 16, 4096):
                s = int(oracle.dm(DM_LM_ROW_WORDS, W, V))
                assert s == ((W + 2 + 3) & ~3) + 4 * V
                room = s - 4 * V - W
                assert s % 4 == 0 and 2 <= room < 6
                if W % 4 == 1:
                    assert s == ((W + 3) & ~3) + 4 * V            # no row grows
                else:
                    assert s == ((W + 3) & ~3) + 4 + 4 * V        # one word of padding was one too few
    assert int(oracle.dm(DM_LM_ROW_WORDS, 81, 0)) == 84 and int(oracle.dm(DM_LM_ROW_WORDS, 99, 0)) == 104


# ---- the window's reach per axis -------------------------------------------------------------
REACH_W, REACH_H = 200, 170                   # large enough that no probe patch leaves the grid


def tile_probes(grid):
    """five poses in the tile under the origin: its four corners (1e-3 of a cell inside) and its centre"""
    a0, b0 = (grid.width // 2) >> 3, (grid.height // 2) >> 3
    eps = 1e-3
    pts = [(eps, eps), (8 - eps, eps), (eps, 8 - eps), (8 - eps, 8 - eps), (4.0, 4.0)]
    pa = A.ParticleArrays(len(pts))
    for i, (u, v) in enumerate(pts):
        pa.x[i] = grid.offset[0] + (8 * a0 + u) * grid.scale[0]
        pa.y[i] = grid.offset[1] + (8 * b0 + v) * grid.scale[1]
    pa.orientation[:] = 0.0
    pa.zpos[:] = 0.18
    pa.zsigma[:] = 0.05
    pa.weight[:] = 1.0 / len(pts)
    return pa


def one_update(grid, pa, patches):
    cfg = S.bench_config(A.default_config(), pa.n)
    cfg.flags |= A.FLAG_PARTICLE_MAPS
    assert cfg.max_sensor_range == G.RANGE
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    orc.set_map(grid)
    orc.upload(pa)
    scan = (A.ScanPatch * len(patches))()
    for k, (x, y) in enumerate(patches):
        scan[k].position[:] = [x, y, -0.18]
        scan[k].stdev = 0.03
    orc.map_update(scan)
    return orc


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("name", ["9x11", "11x9"])
def test_window_reach_per_axis(oracle, name, axis):
    scale, (hx, hy) = G.RECT_CASES[name]
    grid = S.unmapped_beyond(G.rect_flat_map(REACH_W, REACH_H, scale), -1e9)
    pa = tile_probes(grid)
    k = 0 if axis == "x" else 1
    h, tile = (hx, hy)[k], 8 * scale[k]
    along = (lambda d: (d, 0.0)) if axis == "x" else (lambda d: (0.0, d))
    # just inside maxSensorRange, both ways: never dropped, and each lands in its own cell
    near = G.RANGE - 1e-3
    assert near < h * tile                              # what dm_lm_half promises
    orc = one_update(grid, pa, [along(near), along(-near)])
    assert orc.info().map_patches_dropped == 0
    for i in range(pa.n):
        cells = orc.particle_map(i)[0].astype(np.int64)
        want = []
        for d in (near, -near):
            px, py = pa.x[i] + along(d)[0], pa.y[i] + along(d)[1]
            m, n = G.cell_coords(grid, px, py)
            want.append(int(math.floor(n)) * grid.width + int(math.floor(m)))
        assert sorted(cells.tolist()) == sorted(want), (name, axis, i)
    # more than h + 1 tiles away on that axis: always outside the window -- and on the grid, so the
    # patches are counted as dropped, not skipped
    far = (h + 1) * tile + 1e-3
    for d in (far, -far):
        px, py = pa.x + along(d)[0], pa.y + along(d)[1]
        m, n = G.cell_coords(grid, px, py)
        assert np.all((m >= 0) & (m < grid.width) & (n >= 0) & (n < grid.height))
    orc = one_update(grid, pa, [along(far), along(-far)])
    assert orc.info().map_patches_dropped == 2 * pa.n
    assert all(len(orc.particle_map(i)[0]) == 0 for i in range(pa.n))
    # the other axis' half width is not this one's: h tiles of the other axis' size fall short or
    # overshoot, so the two cases above tell a swapped hx / hy apart
    assert (hx, hy)[1 - k] != h


# ---- cell placement ---------------------------------------------------------------------------
BORDER = 1e-6                                  # of a cell: beyond the rounding of * (1 / scale) vs / scale


@pytest.mark.parametrize("yaw", [None, 0.7])
@pytest.mark.parametrize("name", ["9x11", "11x9"])
def test_cell_placement(oracle, name, yaw):
    scale, _ = G.RECT_CASES[name]
    grid = G.rect_prior("empty", scale, yaw=yaw)
    n = 96
    cfg = S.bench_config(A.default_config(), n)
    cfg.flags |= A.FLAG_PARTICLE_MAPS
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    orc.set_map(grid)
    orc.init_gaussian(n, [0.0, 0.0, 0.0], [0.3, 0.3, 0.4], 0.18, 0.05)
    scan = S.scan_patches(nx=9, ny=7, x0=-1.3, x1=2.1, y0=-1.7, y1=1.9)
    orc.map_update(scan)
    assert orc.info().map_patches_dropped == 0
    p = orc.download()
    sx = np.array([s.position[0] for s in scan])
    sy = np.array([s.position[1] for s in scan])
    sz = np.array([s.position[2] for s in scan])
    distinct = 0
    for i in range(n):
        co, sn = math.cos(p.orientation[i]), math.sin(p.orientation[i])
        wx = co * sx - sn * sy + p.x[i]
        wy = sn * sx + co * sy + p.y[i]
        lx, ly = G.to_local(grid, wx, wy, sz + p.zpos[i])
        m, nn = G.cell_coords(grid, lx, ly)
        # the inputs keep off the cell borders, so the two ways of dividing agree
        assert np.all(np.abs(m - np.round(m)) > BORDER) and np.all(np.abs(nn - np.round(nn)) > BORDER), i
        fm, fn = np.floor(m).astype(np.int64), np.floor(nn).astype(np.int64)
        assert np.all((fm >= 0) & (fm < grid.width) & (fn >= 0) & (fn < grid.height))
        want = np.unique(fn * grid.width + fm)
        got = np.sort(orc.particle_map(i)[0].astype(np.int64))
        assert np.array_equal(got, want), (name, yaw, i)
        distinct += want.size
    assert distinct > n * len(scan) // 2                # the patches mostly land in cells of their own
