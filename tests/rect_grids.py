"""Grids that are square in neither sense (test infrastructure): width != height and
scale_x != scale_y, so that a swapped axis, a wx used for wy or an hx used for both halves shows.
The terrain recipe is synthetic.rough_map's (sinusoids plus noise, 1 to 8 stacked patches per
cell); cell (m, n) has its centre at offset + (m + 0.5, n + 0.5) * scale, the offset centres the
grid on the origin, and the cell's index is n * width + m.

RECT_CASES lists one cell size per parity class of the per-particle window's half widths
(hx, hy) = dm_lm_half(3 m, scale): a table row's bookkeeping words sit behind its
(2 hx + 1)(2 hy + 1) window slots, and how many words the padding to 16 bytes leaves there
depends on those parities.  tests/test_rect_grids.py checks the table against
dm_lm_half."""
import math

import numpy as np

import synthetic as S
from eslam_abi import GridArrays

WIDTH, HEIGHT = 150, 110
RANGE = 3.0                                  # max_sensor_range of the default configuration

# name: (scale, (hx, hy)); W = (2 hx + 1)(2 hy + 1) is 3 mod 4 on the first three
RECT_CASES = {
    "9x11": ((0.10, 0.08), (4, 5)),
    "11x9": ((0.08, 0.10), (5, 4)),
    "9x15": ((0.10, 0.06), (4, 7)),
    "9x17": ((0.10, 0.05), (4, 8)),
    "11x15": ((0.08, 0.06), (5, 7)),
}
MIXED_PARITY = ("9x11", "11x9", "9x15")      # hx and hy of different parity


def _offset(width, height, scale):
    return (-width * scale[0] / 2.0, -height * scale[1] / 2.0)


def rect_flat_map(width=WIDTH, height=HEIGHT, scale=(0.10, 0.08), mean=0.0, stdev=0.05):
    n = width * height
    return GridArrays(width, height, scale, _offset(width, height, scale), np.arange(n + 1, dtype=np.uint32),
                      np.full(n, mean, np.float32), np.full(n, stdev, np.float32))


def rect_rough_map(width=WIDTH, height=HEIGHT, scale=(0.10, 0.08), seed=7, multi=True):
    rng = np.random.default_rng(seed)
    ox, oy = _offset(width, height, scale)
    xs = ox + (np.arange(width) + 0.5) * scale[0]
    ys = oy + (np.arange(height) + 0.5) * scale[1]
    X, Y = np.meshgrid(xs, ys, indexing="xy")            # (height, width): Y along rows (n), X along m
    amp = 0.2 / 3.0
    ground = (amp * np.sin(2 * math.pi * X / 1.0 + 0.3)
              + amp * np.sin(2 * math.pi * Y / 3.0 + 1.1)
              + amp * np.sin(2 * math.pi * (X + Y) / 5.0 + 2.0))
    ground = (ground + rng.normal(0.0, 0.02, ground.shape)).reshape(-1)      # index n * width + m
    ncell = width * height
    k = np.where(rng.random(ncell) < 0.6, 1, rng.integers(2, 9, ncell)) if multi else np.ones(ncell, dtype=np.int64)
    cell_start = np.zeros(ncell + 1, dtype=np.uint64)
    np.cumsum(k, out=cell_start[1:])
    total = int(cell_start[-1])
    owner = np.repeat(np.arange(ncell), k)
    rank = np.arange(total) - np.repeat(cell_start[:-1], k).astype(np.int64)
    gaps = 1.5 + rng.random(total)
    csum = np.cumsum(np.where(rank == 0, 0.0, gaps))     # level j sits j gaps above the ground patch
    offs = csum - np.repeat(csum[cell_start[:-1].astype(np.int64)], k)
    mean = ground[owner] + offs
    stdev = rng.uniform(0.02, 0.1, total)
    return GridArrays(width, height, scale, (ox, oy), cell_start.astype(np.uint32), mean.astype(np.float32),
                      stdev.astype(np.float32))


def rotated(grid, yaw=0.3, tx=0.4, ty=-0.25):
    """the grid in a local frame rotated by yaw and shifted: global2local = Rz(-yaw) (p - t)
    (test_gpu_particle_maps.py's helper, importable without a GPU test module)"""
    c, s = math.cos(yaw), math.sin(yaw)
    grid.g2l = [c, s, 0.0, -(c * tx + s * ty), -s, c, 0.0, -(-s * tx + c * ty), 0.0, 0.0, 1.0, 0.0]
    return grid


def rect_prior(kind="beyond", scale=(0.10, 0.08), yaw=None, width=WIDTH, height=HEIGHT, flat=False):
    """the shared grid a mapping run starts from: `beyond` (nothing mapped at local x >= 0.3),
    `mapped` (everything) or `empty`; rotated when yaw is given"""
    base = rect_flat_map(width, height, scale) if flat else rect_rough_map(width, height, scale)
    grid = S.unmapped_beyond(base, {"beyond": 0.3, "mapped": 1e9, "empty": -1e9}[kind])
    return rotated(grid, yaw=yaw) if yaw is not None else grid


def to_local(grid, x, y, z=0.0):
    """global2local applied to points (float64 numpy, the plain formula)"""
    A = grid.g2l
    return (A[0] * x + A[1] * y + A[2] * z + A[3], A[4] * x + A[5] * y + A[6] * z + A[7])


def cell_coords(grid, lx, ly):
    """fractional cell coordinates of grid-local points, by division"""
    return ((np.asarray(lx, np.float64) - grid.offset[0]) / grid.scale[0],
            (np.asarray(ly, np.float64) - grid.offset[1]) / grid.scale[1])
