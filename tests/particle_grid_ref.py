"""The model of eslam_gpu_get_particle_grid: a particle's whole map as one CSR
grid, composed in numpy from the two getters that existed before it -- the particle's own cells
(particle_map(i)) and the shared grid.  Per cell: the own patch (height 0), then the shared
grid's patches in their order with their heights.  tests/test_particle_grid_ref.py checks the
rule against the oracle's per-particle lookups; the GPU tests check the device against it."""
import numpy as np

import eslam_abi as A

LOCAL_FIELDS = ("x", "y", "orientation", "zpos", "zsigma", "mprob", "floating", "n_contact_points")


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def prior_grid(case, cells, offset=None):
    """the shared grid a mapping run starts from: `beyond` (nothing mapped at x >= 0.3), `mapped`
    (the whole rough map: the scans land on covered cells, so the particles hold copies of
    them), `empty` (the reference's own start), `heights` (beyond, with vertical patches as
    test_gpu_shared_map.py's case_grid("rough_heights") draws them), `rotated_grid` (beyond, in
    a local frame rotated and shifted as test_gpu_particle_maps.py's rotated())"""
    import math
    import synthetic as S
    grid = S.rough_map(cells=cells)
    if case == "heights":
        rng = np.random.default_rng(3)
        grid.patch_height = np.where(rng.random(grid.mean.shape[0]) < 0.3, rng.uniform(0.05, 0.5, grid.mean.shape[0]),
                                     0.0).astype(np.float32)
    if case == "rotated_grid":
        c, s, tx, ty = math.cos(0.3), math.sin(0.3), 0.4, -0.25
        grid.g2l = [c, s, 0.0, -(c * tx + s * ty), -s, c, 0.0, -(-s * tx + c * ty), 0.0, 0.0, 1.0, 0.0]
    if offset is not None:                   # the grid's corner elsewhere (default: centred on the origin)
        grid.offset = (float(offset[0]), float(offset[1]))
    x0 = {"mapped": 1e9, "empty": -1e9}.get(case, 0.3)
    return S.unmapped_beyond(grid, x0)


def compose(pmap, grid):
    """(cells, mean, stdev) of one particle + the shared grid (GridArrays) -> GridArrays"""
    cells, mean, sd = pmap
    ncell = grid.width * grid.height
    cells = np.asarray(cells, dtype=np.int64)
    assert cells.size == np.unique(cells).size, "a cell twice in a particle's map"
    assert cells.size == 0 or (cells.min() >= 0 and cells.max() < ncell), "an own cell off the grid"
    cs = grid.cell_start.astype(np.int64)
    counts = np.diff(cs)
    own = np.zeros(ncell, dtype=np.int64)
    own[cells] = 1
    start = np.zeros(ncell + 1, dtype=np.int64)
    np.cumsum(counts + own, out=start[1:])
    total = int(start[-1])
    assert total <= 0xffffffff
    out_m = np.zeros(total, np.float32)
    out_s = np.zeros(total, np.float32)
    out_h = None if grid.patch_height is None else np.zeros(total, np.float32)
    # the shared grid's patches: behind the own patch of their cell, in their order
    owner = np.repeat(np.arange(ncell), counts)
    rank = np.arange(int(cs[-1])) - cs[owner]
    pos = start[owner] + own[owner] + rank
    out_m[pos] = grid.mean
    out_s[pos] = grid.stdev
    if out_h is not None:
        out_h[pos] = grid.patch_height
    out_m[start[cells]] = np.asarray(mean, np.float32)
    out_s[start[cells]] = np.asarray(sd, np.float32)
    return A.GridArrays(grid.width, grid.height, grid.scale, grid.offset, start.astype(np.uint32), out_m, out_s, out_h, grid.g2l)


def grids_equal(a, b):
    """bit for bit: cell_start and the u32 views of mean, stdev and heights"""
    if (a.width, a.height) != (b.width, b.height) or (a.patch_height is None) != (b.patch_height is None):
        return False
    if not np.array_equal(a.cell_start, b.cell_start):
        return False
    if not (np.array_equal(u32(a.mean), u32(b.mean)) and np.array_equal(u32(a.stdev), u32(b.stdev))):
        return False
    return a.patch_height is None or np.array_equal(u32(a.patch_height), u32(b.patch_height))


def local_fields_equal(pa, pb, i):
    """the fields of particle i an update computes from its own lookups alone (weight is
    normalised over all particles), bit for bit"""
    for f in LOCAL_FIELDS:
        x, y = getattr(pa, f)[i:i + 1], getattr(pb, f)[i:i + 1]
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        if x[0] != y[0]:
            return False
    return True
