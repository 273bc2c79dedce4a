"""The SurfaceHash respawn and getBestParticleIndex on the device at the edge values of their
orderings: the cases of test_hash_ref.py (hash_edge_cases.py) through GpuFilter, compared with
hash_ref.py (an independent restatement in plain Python) under the same rules, and with the CPU
oracle bit for bit.  The float conversion of k_hash_keys must equal the host's IEEE
round-to-nearest-even (float) at ties, in the denormal range and at overflow; -0 and +0 tie in
both orderings; a NaN weight sorts after +inf in the respawn and is never the best particle."""
import numpy as np
import pytest

import eslam_abi as A
import hash_edge_cases as E
import hash_ref as H
import oracle_ffi as O
from parity_util import assert_bit_identical

pytestmark = pytest.mark.gpu


def oracle_filter(cfg):
    return O.OracleFilter(cfg, O.SUM_CONTRACT)


def against_oracle(gpu, orc, runs_g, runs_o):
    for (_, after_g, _, _, label), (_, after_o, _, _, _) in zip(runs_g, runs_o):
        assert_bit_identical(after_g, after_o, label)
    sg, so = gpu.rng_state(), orc.rng_state()
    assert sg.libc_rand_pos == so.libc_rand_pos and list(sg.libc_rand) == list(so.libc_rand)


@pytest.mark.parametrize("n", [1, 2049])
def test_init_hash_against_ref(gpu_mod, oracle, n):
    cfg = E.edge_config(n, 0.05)
    gpu, orc = gpu_mod.GpuFilter(cfg), oracle_filter(cfg)
    for f in (gpu, orc):
        f.set_map(E.hash_grid(cells=E.CELLS))
        f.hash_create()
    ref = E.make_ref(gpu)
    gpu.init_hash(n)
    orc.init_hash(n)
    pa = gpu.download()
    E.check_init(pa, ref, ref.init(n))
    E.assert_rand_state(gpu, ref, "init")
    assert_bit_identical(pa, orc.download(), "init")
    gpu.close()


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_respawn_against_ref(gpu_mod, oracle, case):
    runs, gpu, cfg = E.run_case(gpu_mod.GpuFilter, case)
    E.check_case(case, runs, cfg)
    runs_o, orc, _ = E.run_case(oracle_filter, case)
    against_oracle(gpu, orc, runs, runs_o)
    gpu.close()


def test_two_respawns_in_a_row(gpu_mod, oracle):
    case = ("twice", E.N3, "dyadic", 0.05, "slope")
    runs, gpu, cfg = E.run_case(gpu_mod.GpuFilter, case, then=("one_float",))
    assert len(runs) == 2 and all(r.k > 0 for _, _, r, _, _ in runs)
    E.check_case(case, runs, cfg)
    runs_o, orc, _ = E.run_case(oracle_filter, case, then=("one_float",))
    against_oracle(gpu, orc, runs, runs_o)
    gpu.close()


@pytest.fixture(scope="module")
def best_filter(gpu_mod):
    f = gpu_mod.GpuFilter(A.default_config())
    yield f
    f.close()


@pytest.mark.parametrize("n", E.BEST_SIZES)
def test_best_index_against_loop(best_filter, n):
    """eslam_gpu_get_best_particle_index == the plain loop of getBestParticleIndex
    (hash_ref.best_index).  [-0.0, ..., +0.0] above negative weights returns the -0.0's index 0:
    before k_best_max and k_best_index dropped the zero's sign, the ordered key of +0 was the
    larger one and the device returned n - 1."""
    for name, w in E.best_cases(n):
        best_filter.upload(E.particles(w))
        assert best_filter.best_index() == H.best_index(w.tolist()), name


def test_best_index_signed_zero_pair(best_filter):
    for w, want in (([-0.0, 0.0], 0), ([0.0, -0.0], 0), ([-1.0, -0.0, 0.0], 1)):
        best_filter.upload(E.particles(np.array(w)))
        assert best_filter.best_index() == want == H.best_index(w), w
