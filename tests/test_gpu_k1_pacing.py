"""K1 (k_project_weight) with its waves paced by rows done: a wave sets its priority from the
row it is at ("K1's waves paced by rows done").  A priority cannot change a value,
but the band arithmetic sits at the top of every row of every instantiation and can be wrong at
the edges, so every case here compares every particle and the update info with the oracle bit
for bit after each of three forced-resample steps (run_pair does, as in test_gpu_k1_rows.py).

Band positions: chunk rows J = 2 (fewer rows than the four bands), 4 and 5 (the band changes
at every row), 13 (the bench's J at 4M), each at n = 64 J - 1 (one chunk, its last row one lane
short, so the wave leaves the loop in whatever band that row has) and n = 2 * 64 J + 1 (two
full chunks and a chunk of one row with one lane, which leaves the loop in the first band).

The prologue's paths (the Box-Muller tables are staged in the tail of the window's LDS, or read
from global memory when the window needs that tail, or there is no window at all; the
project-only launch always stages them): the cloud's spread is chosen so that the staged window
has the size the case is about, and the size is asserted on the host from a second oracle run.

A sharded filter's split launches (ChunkSel) run paced in the existing `chunks` scenario of the
distributed tests (three-row chunks at two and more ranks); no sharded case is repeated here.
"""
import os
import re

import pytest

import contact_layouts as L
import eslam_abi as A
import oracle_ffi as O
import synthetic as S
from parity_util import assert_bit_identical, info_tuple, run_pair

pytestmark = pytest.mark.gpu

STEPS = 3
ROWS = (2, 4, 5, 13)
SPLIT_ROWS = 5


def sizes(J):
    return (64 * J - 1, 2 * 64 * J + 1)


@pytest.fixture(scope="module")
def grids():
    return {"flat": S.flat_map(cells=200), "rough": S.rough_map(cells=200)}


def paced_config(n, J):
    cfg = S.bench_config(A.default_config(), n)
    cfg.sum_chunk_rows = J
    return cfg


def factory(gpu_mod):
    return lambda cfg: gpu_mod.GpuFilter(cfg)


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("J", ROWS)
@pytest.mark.parametrize("terrain", ("flat", "rough"))
def test_band_positions(gpu_mod, grids, terrain, J, which):
    n = sizes(J)[which]
    stream = S.step_stream(STEPS, tilt=terrain == "rough")
    gpu, orc = run_pair(paced_config(n, J), grids[terrain], stream, n, gpu_factory=factory(gpu_mod),
                        label=f"{terrain} J={J} n={n}")
    assert gpu.sync().resampled == 1 and orc.info().resampled == 1


def test_project_then_update_paced(gpu_mod, grids):
    """The PROJECT-only and the WEIGHT-only instantiations, five-row chunks: two chunks, then a
    chunk of one row with one lane.  The project-only launch always stages the tables."""
    n = sizes(SPLIT_ROWS)[1]
    stream = S.step_stream(STEPS)
    gpu, orc = run_pair(paced_config(n, SPLIT_ROWS), grids["flat"], stream, n, gpu_factory=factory(gpu_mod),
                        mode="project", label="project")
    for k, st in enumerate(stream):
        orc.update(st)
        gpu.update(st)
        gpu.sync()
        assert_bit_identical(gpu.download(), orc.download(), f"update {k}")
        assert info_tuple(gpu.sync()) == info_tuple(orc.info())


def lds_constants():
    """kWindowLds and kBmLds (bytes) from the source, and the 16-byte window cell."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(A.__file__)), "csrc", "eslam_internal.h")).read()
    window = int(re.search(r"#define ESLAM_WINDOW_LDS (\d+)", src).group(1))
    tables = int(re.search(r"constexpr int kBmLds = (\d+);", src).group(1))
    return window // 16, (window - tables) // 16


# the cloud's sigma in x and y for each prologue path (641 particles on the flat map of 0.1 m
# cells; the window is the cloud's box plus a margin of about 0.72 m and three cells each way)
PROLOGUE = {"tables_staged": 0.1, "tables_global": 0.34, "no_window": 0.6}


@pytest.mark.parametrize("path", list(PROLOGUE))
def test_prologue_paths(gpu_mod, oracle, grids, path):
    cells_window, cells_with_tables = lds_constants()
    assert cells_window == L.WINDOW_LDS_CELLS
    n = sizes(SPLIT_ROWS)[1]
    cfg = paced_config(n, SPLIT_ROWS)
    grid = grids["flat"]
    stream = S.step_stream(STEPS)
    sigma = PROLOGUE[path]
    init = dict(mu=[0.0, 0.0, 0.0], sigma=[sigma, sigma, 0.1], z=0.18, zs=1.001)
    # the windows of the weightings after the first (the first has no box yet: no window), from
    # an oracle that runs each step as project + update: a weighting sees the projected cloud
    f = O.OracleFilter(cfg, O.SUM_CONTRACT)
    f.set_map(grid)
    f.init_gaussian(n, init["mu"], init["sigma"], init["z"], init["zs"])
    cells, seen = [], None
    for st in stream:
        f.project(st)
        now = f.download()
        if seen is not None:
            cells.append(L.window_cells(seen, st, cfg, grid, max_weight=f.info().max_weight))
        assert f.update(st) == 0
        seen = now
    assert len(cells) == STEPS - 1
    if path == "tables_staged":
        assert all(0 < c <= cells_with_tables for c in cells), cells
    elif path == "tables_global":
        assert all(cells_with_tables < c <= cells_window for c in cells), cells
    else:
        assert all(c > cells_window for c in cells), cells
    gpu, orc = run_pair(cfg, grid, stream, n, init=init, gpu_factory=factory(gpu_mod), label=path)
    assert_bit_identical(orc.download(), f.download(), f"{path}: the window sizes are of another run")
    assert orc.info().resampled == 1
