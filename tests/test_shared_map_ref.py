"""The CPU reference of the shared-map merge (tests/c/shared_map_ref.c, the contract of
eslam_gpu_shared_map_update) on hand-computed cases, and the ctypes mirror of its counters."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import eslam_abi as A
import shared_map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W = H = 4            # cells of 1 m, origin (0, 0); the test cell is (m, n) = (1, 2)
CELL = 2 * W + 1


def grid_with(patches=(), heights=False):
    """a 4 x 4 grid whose only patches are `patches` [(mean, stdev, height)] in cell (1, 2)"""
    cs = np.zeros(W * H + 1, np.uint32)
    cs[CELL + 1:] = len(patches)
    col = lambda j: np.array([p[j] for p in patches], np.float32)
    return A.GridArrays(W, H, (1.0, 1.0), (0.0, 0.0), cs, col(0), col(1), col(2) if heights else None)


def particles(rows):
    """rows: (x, y, theta, zpos, zsigma)"""
    pa = A.ParticleArrays(len(rows))
    for i, r in enumerate(rows):
        pa.x[i], pa.y[i], pa.orientation[i], pa.zpos[i], pa.zsigma[i] = r
    return pa


def scan(rows):
    """rows: (x, y, z, stdev) in the body frame"""
    out = (A.ScanPatch * len(rows))()
    for k, r in enumerate(rows):
        out[k].position[:] = r[:3]
        out[k].stdev = r[3]
    return out


def cell(g, c=CELL):
    b, e = int(g.cell_start[c]), int(g.cell_start[c + 1])
    return [(g.mean[k], g.stdev[k]) for k in range(b, e)]


def bits(v):
    return np.float32(v).view(np.uint32)


AT = (1.5, 2.5, 0.0)          # a particle over the test cell, heading along x


def test_insert_into_empty_cell():
    g, info = R.merge(grid_with(), particles([AT + (0.25, 0.125)]), scan([(0.0, 0.0, 0.5, 0.25)]))
    wz, var = 0.5 + 0.25, 0.25 * 0.25 + 0.125 * 0.125
    assert [(bits(m), bits(s)) for m, s in cell(g)] == [(bits(wz), bits(math.sqrt(var)))]
    assert int(g.cell_start[-1]) == 1 and g.patch_height is None
    assert info.as_dict() == dict(particles_done=1, patches_placed=1, patches_off_grid=0, cells_touched=1, fused=0,
                                  absorbed=0, inserted=1, n_patches=1, runs=1)


def test_second_patch_within_three_sigma_fuses():
    m1, s1 = np.float32(0.75), np.float32(0.25)
    g, info = R.merge(grid_with([(m1, s1, 0.0)]), particles([AT + (0.375, 0.125)]), scan([(0.0, 0.0, 0.5, 0.25)]))
    wz, var = 0.5 + 0.375, 0.25 * 0.25 + 0.125 * 0.125
    v1 = float(s1) * float(s1)
    assert (wz - float(m1)) ** 2 < 9.0 * (v1 + var)
    mean = (float(m1) * var + wz * v1) / (v1 + var)
    v = (v1 * var) / (v1 + var)
    assert [(bits(m), bits(s)) for m, s in cell(g)] == [(bits(mean), bits(math.sqrt(v)))]
    assert (info.fused, info.inserted, info.absorbed, info.n_patches) == (1, 0, 0, 1)


def test_patch_beyond_three_sigma_appends_a_second_level():
    g, info = R.merge(grid_with([(0.0, 0.1, 0.0)]), particles([AT + (0.0, 0.0)]), scan([(0.0, 0.0, 5.0, 0.1)]))
    assert [(bits(m), bits(s)) for m, s in cell(g)] == [(bits(0.0), bits(np.float32(0.1))), (bits(5.0), bits(math.sqrt(0.1 * 0.1)))]
    assert (info.fused, info.inserted, info.absorbed, info.n_patches) == (0, 1, 0, 2)


def test_vertical_patch_absorbs():
    # the wall spans [1.0 - 0.8, 1.0]: a scan patch at 0.5 is inside it
    grid = grid_with([(1.0, 0.1, 0.8)], heights=True)
    g, info = R.merge(grid, particles([AT + (0.0, 0.01)]), scan([(0.0, 0.0, 0.5, 0.01)]))
    assert np.array_equal(g.cell_start, grid.cell_start)
    for a, b in ((g.mean, grid.mean), (g.stdev, grid.stdev), (g.patch_height, grid.patch_height)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (info.fused, info.inserted, info.absorbed, info.n_patches) == (0, 0, 1, 1)
    # an appended patch of a grid with heights is horizontal
    g, info = R.merge(grid, particles([AT + (0.0, 0.01)]), scan([(0.0, 0.0, 3.0, 0.01)]))
    assert list(g.patch_height) == [np.float32(0.8), 0.0] and info.inserted == 1


def test_off_grid_and_non_finite_are_skipped_and_counted():
    sc = scan([(0.0, 0.0, 0.0, 0.1), (10.0, 0.0, 0.0, 0.1), (0.0, -7.0, 0.0, 0.1)])
    pa = particles([AT + (0.0, 0.0), (float("nan"), 2.5, 0.0, 0.0, 0.0), (1.5, float("inf"), 0.0, 0.0, 0.0),
                    (1.5, 2.5, float("nan"), 0.0, 0.0)])
    g, info = R.merge(grid_with(), pa, sc)
    assert info.as_dict() == dict(particles_done=4, patches_placed=1, patches_off_grid=11, cells_touched=1, fused=0,
                                  absorbed=0, inserted=1, n_patches=1, runs=1)
    assert len(cell(g)) == 1


def test_particle_order_is_part_of_the_contract():
    # against {0, 0.2}: a particle at 0.5 fuses (mean ~0.4975, sigma ~0.014), after which 0.57 is
    # beyond 3 sigma and starts a second level; the other way round 0.57 fuses first (~0.567)
    # and 0.5 starts the second level
    grid = grid_with([(0.0, 0.2, 0.0)])
    a, b = AT + (0.5, 0.01), AT + (0.57, 0.01)
    sc = scan([(0.0, 0.0, 0.0, 0.01)])
    gab, iab = R.merge(grid, particles([a, b]), sc)
    gba, iba = R.merge(grid, particles([b, a]), sc)
    assert (iab.fused, iab.inserted) == (iba.fused, iba.inserted) == (1, 1)
    assert abs(cell(gab)[0][0] - 0.4975) < 1e-3 and cell(gab)[1][0] == np.float32(0.57)
    assert abs(cell(gba)[0][0] - 0.5672) < 1e-3 and cell(gba)[1][0] == np.float32(0.5)


def test_later_particles_see_earlier_writes():
    # three particles at one height: one insert, then two fuses into the inserted patch
    g, info = R.merge(grid_with(), particles([AT + (0.2, 0.05)] * 3), scan([(0.0, 0.0, 0.0, 0.05)]))
    assert (info.inserted, info.fused, info.n_patches, info.cells_touched) == (1, 2, 1, 1)
    assert cell(g)[0][1] < np.float32(math.sqrt(2 * 0.05 * 0.05))


def test_empty_scan_is_the_identity():
    grid = grid_with([(0.5, 0.1, 0.0), (3.0, 0.2, 0.0)])
    g, info = R.merge(grid, particles([AT + (0.0, 0.1)] * 5), scan([]))
    assert np.array_equal(g.cell_start, grid.cell_start)
    assert np.array_equal(g.mean.view(np.uint32), grid.mean.view(np.uint32))
    assert np.array_equal(g.stdev.view(np.uint32), grid.stdev.view(np.uint32))
    assert (info.patches_placed, info.inserted, info.fused, info.n_patches) == (0, 0, 0, 2)


def test_rotated_particle_and_grid_frame():
    # heading +y: the body's x axis points along y; the patch 1 m ahead lands one row up.  Then
    # the same through a non-identity global2local (a shift by one cell in x)
    pa = particles([(1.5, 1.5, math.pi / 2, 0.0, 0.0)])
    g, _ = R.merge(grid_with(), pa, scan([(1.0, 0.0, 0.25, 0.1)]))
    assert len(cell(g, 2 * W + 1)) == 1
    shifted = grid_with()
    shifted.g2l = [1.0, 0, 0, 1.0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    g, _ = R.merge(shifted, pa, scan([(1.0, 0.0, 0.25, 0.1)]))
    assert len(cell(g, 2 * W + 2)) == 1 and int(g.cell_start[-1]) == 1


RECT_W, RECT_H = 5, 3                   # a grid square in neither sense: 5 x 3 cells of 0.5 m x 2 m, origin (-1, -3)
RECT_SCALE, RECT_OFF = (0.5, 2.0), (-1.0, -3.0)


@pytest.mark.parametrize("m,n", [(0, 0), (4, 0), (1, 2), (4, 2), (3, 1)])
@pytest.mark.parametrize("frame", ["identity", "shifted", "quarter_turn"])
def test_rectangular_grid_with_rectangular_cells(m, n, frame):
    """a patch aimed at the centre of cell (m, n) lands in cell n * width + m and nowhere else:
    per axis floor((l - offset) / scale), with the axis' own offset, scale and extent (a cell
    index below 5 in y or a y extent of 10 m would be another axis' numbers).  Through the
    identity, a global2local shifted by (0.25, -1) and one turned by 90 degrees."""
    cs = np.zeros(RECT_W * RECT_H + 1, np.uint32)
    e = np.zeros(0, np.float32)
    grid = A.GridArrays(RECT_W, RECT_H, RECT_SCALE, RECT_OFF, cs, e, e)
    lx = RECT_OFF[0] + (m + 0.5) * RECT_SCALE[0]             # the cell's centre in the grid's frame
    ly = RECT_OFF[1] + (n + 0.5) * RECT_SCALE[1]
    if frame == "identity":
        wx, wy = lx, ly
    elif frame == "shifted":                                 # l = p + (0.25, -1)
        grid.g2l = [1.0, 0, 0, 0.25, 0, 1.0, 0, -1.0, 0, 0, 1.0, 0]
        wx, wy = lx - 0.25, ly + 1.0
    else:                                                    # l = (p_y, -p_x): exact in floating point
        grid.g2l = [0.0, 1.0, 0, 0, -1.0, 0.0, 0, 0, 0, 0, 1.0, 0]
        wx, wy = -ly, lx
    pa = particles([(wx - 0.125, wy, 0.0, 0.25, 0.125)])     # the patch sits 0.125 m ahead of the particle
    g, info = R.merge(grid, pa, scan([(0.125, 0.0, 0.5, 0.25)]))
    counts = np.diff(g.cell_start.astype(np.int64))
    assert counts.tolist() == [1 if c == n * RECT_W + m else 0 for c in range(RECT_W * RECT_H)]
    assert (g.width, g.height, g.scale, g.offset) == (RECT_W, RECT_H, RECT_SCALE, RECT_OFF)
    assert (info.patches_placed, info.patches_off_grid, info.inserted) == (1, 0, 1)
    assert bits(g.mean[0]) == bits(0.5 + 0.25) and bits(g.stdev[0]) == bits(math.sqrt(0.25 * 0.25 + 0.125 * 0.125))
    # one cell past the grid's edge on either axis is off the grid, though inside the other axis' extent
    for dx, dy in ((RECT_W * RECT_SCALE[0], 0.0), (0.0, RECT_H * RECT_SCALE[1])):
        ox, oy = (lx + dx, ly + dy) if frame != "quarter_turn" else (lx, ly)
        if frame == "quarter_turn":
            far = particles([(-(ly + dy) - 0.125, lx + dx, 0.0, 0.25, 0.125)])
        elif frame == "shifted":
            far = particles([(ox - 0.25 - 0.125, oy + 1.0, 0.0, 0.25, 0.125)])
        else:
            far = particles([(ox - 0.125, oy, 0.0, 0.25, 0.125)])
        g2, info2 = R.merge(grid, far, scan([(0.125, 0.0, 0.5, 0.25)]))
        assert (info2.patches_placed, info2.patches_off_grid, int(g2.cell_start[-1])) == (0, 1, 0), (dx, dy)


def test_merge_info_layout_matches_ctypes(tmp_path):
    py = A.SharedMergeInfo
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eslam_gpu.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(eslam_shared_merge_info));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(eslam_shared_merge_info, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.split("\n") if l)
    assert int(out["size"]) == C.sizeof(py) == R.lib().smr_info_size() == 9 * 8
    for f, t in py._fields_:
        assert int(out[f]) == getattr(py, f).offset and t is C.c_uint64, f
