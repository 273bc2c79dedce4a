"""K1 (k_project_weight) at row and chunk edges: three-row chunks (192 particles) at sizes where
a lone lane, a full row, a row plus one lane, a chunk one short / exact / one over, and a last
chunk of one row with one lane all occur.  Every particle is compared with the oracle bit for
bit after every step; the first step runs with no pending gather, the others read their
particles through the segment marks of the forced resample."""
import pytest

import eslam_abi as A
import synthetic as S
from parity_util import assert_bit_identical, info_tuple, run_pair

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 191, 192, 193, 385)
CHUNK_ROWS = 3


@pytest.fixture(scope="module")
def grids():
    return {"flat": S.flat_map(cells=200), "rough": S.rough_map(cells=200)}


def edge_config(n):
    cfg = S.bench_config(A.default_config(), n)
    cfg.sum_chunk_rows = CHUNK_ROWS
    return cfg


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("terrain", ("flat", "rough"))
def test_row_and_chunk_edges(gpu_mod, grids, terrain, n):
    stream = S.step_stream(5, tilt=terrain == "rough")
    gpu, orc = run_pair(edge_config(n), grids[terrain], stream, n, gpu_factory=lambda cfg: gpu_mod.GpuFilter(cfg),
                        label=f"{terrain} n={n}")
    assert gpu.sync().resampled == 1 and orc.info().resampled == 1


def test_project_then_update_three_row_chunks(gpu_mod, grids):
    """The PROJECT-only and the WEIGHT-only instantiations: a chunk, then one row of one lane."""
    n = 193
    stream = S.step_stream(4)
    gpu, orc = run_pair(edge_config(n), grids["flat"], stream, n, gpu_factory=lambda cfg: gpu_mod.GpuFilter(cfg),
                        mode="project", label="project")
    for k, st in enumerate(stream):
        orc.update(st)
        gpu.update(st)
        gpu.sync()
        assert_bit_identical(gpu.download(), orc.download(), f"update {k}")
        assert info_tuple(gpu.sync()) == info_tuple(orc.info())
