"""The rule of eslam_gpu_get_particle_grid on the CPU (tests/particle_grid_ref.py): a particle's
own patch per cell, then the shared grid's patches, as one CSR grid.  Acceptance is the
equivalence with the per-particle lookup: a shared-map oracle given the composed grid of
particle i and the same particles computes, in one update, what the per-particle-maps oracle
computes for particle i -- x, y, orientation, zpos, zsigma, mprob, floating and
n_contact_points bit for bit (weight is normalised over all particles).  Another particle's
grid gives different values, so the comparison has teeth."""
import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import synthetic as S
import particle_grid_ref as R

N = 256
PROBES = (0, 1, N // 2, N - 1)


def run_maps_oracle(grid, n=N, steps=12):
    """the mapping run: `steps` steps with a map update each, no resample (min_effective 0),
    then one more projection; returns the filter, the particles before the last update and
    that update's input"""
    cfg = S.bench_config(A.default_config(), n)
    cfg.min_effective = 0
    cfg.flags |= A.FLAG_PARTICLE_MAPS
    f = O.OracleFilter(cfg, O.SUM_CONTRACT)
    f.set_map(grid)
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.05, 0.05, 0.02], 0.18, 0.05)
    scan = S.scan_patches()
    stream = S.step_stream(steps + 1, tilt=True)
    for st in stream[:steps]:
        f.step(st)
        f.map_update(scan)
    f.project(stream[steps])
    return f, f.download(), stream[steps]


def shared_update(grid, particles, st, n=N):
    """one update of a shared-map oracle holding `particles` on `grid`"""
    cfg = S.bench_config(A.default_config(), n)
    cfg.min_effective = 0
    g = O.OracleFilter(cfg, O.SUM_CONTRACT)
    g.set_map(grid)
    g.upload(particles)
    g.update(st)
    return g.download()


def case_grid(case):
    if case.startswith("rect_"):             # 150 x 110 cells of 0.10 x 0.08 m (tests/rect_grids.py), also rotated
        import rect_grids
        kind, _, rot = case[5:].partition("_")
        return rect_grids.rect_prior(kind, (0.10, 0.08), yaw=0.7 if rot else None)
    return R.prior_grid(case, 80)


@pytest.mark.parametrize("case", ["beyond", "mapped", "empty", "heights", "rect_beyond", "rect_mapped", "rect_beyond_rotated"])
def test_composed_grid_answers_like_the_particle(oracle, case):
    grid = case_grid(case)
    f, before, st = run_maps_oracle(grid)
    maps = {i: f.particle_map(i) for i in PROBES}
    f.update(st)
    after = f.download()
    assert f.info().resampled == 0
    own_cells = 0
    for i in PROBES:
        own_cells += len(maps[i][0])
        comp = R.compose(maps[i], grid)
        assert (comp.patch_height is None) == (grid.patch_height is None)
        assert int(comp.cell_start[-1]) == int(grid.cell_start[-1]) + len(maps[i][0])
        got = shared_update(comp, before, st)
        assert R.local_fields_equal(got, after, i), (case, i)
    assert own_cells > 0
    if case == "beyond":
        # another particle's map answers differently for particle 0
        differ = 0
        for j in PROBES[1:]:
            got = shared_update(R.compose(maps[j], grid), before, st)
            differ += int(got.zpos[0] != after.zpos[0] or got.mprob[0] != after.mprob[0])
        print("beyond: other particles' grids that change particle 0:", differ)
        assert differ > 0


def test_compose_layout():
    """the layout on a hand-made grid: the own patch leads its cell's list with height 0, the
    grid's patches keep their order and heights, cells without an own patch are copied"""
    cs = np.array([0, 2, 2, 3, 3], np.uint32)                      # 2 x 2 cells: 2, 0, 1, 0 patches
    grid = A.GridArrays(2, 2, (0.1, 0.1), (0.0, 0.0), cs, np.array([1, 2, 3], np.float32), np.array([.1, .2, .3], np.float32),
                        np.array([0, .5, 0], np.float32))
    pm = (np.array([3, 0], np.uint32), np.array([9, 8], np.float32), np.array([.9, .8], np.float32))
    c = R.compose(pm, grid)
    assert c.cell_start.tolist() == [0, 3, 3, 4, 5]
    assert c.mean.tolist() == [8, 1, 2, 3, 9]
    assert np.array_equal(c.stdev, np.array([.8, .1, .2, .3, .9], np.float32))
    assert c.patch_height.tolist() == [0, 0, .5, 0, 0]
    assert R.grids_equal(R.compose((pm[0][:0], pm[1][:0], pm[2][:0]), grid), grid)
