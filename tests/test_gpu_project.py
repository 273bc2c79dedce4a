"""The predict step on the device on full odometry covariances and pose edges: every case of
project_cases.py through eslam_gpu_project alone (K1's PROJECT, no-WEIGHT instantiation), through
eslam_gpu_step with a resample pending from the step before (the fused gather + project + weight
kernel) and, for one case set, with per-particle maps (the DELTA instantiation).  Every path is
bit-identical to the CPU oracle; the project-alone path also lies within project_ref.py's derived
bounds of the mpmath restatement, with zsigma equal to the exactly rounded double -- the device's
dm_sqrt_fast on both sides of its 2^-767 switch, at 0, in the denormal range and at squares that
overflow.  The bit-identity carries the bounds to the other paths.  (An exchange of L10 and L20 in
fill_step_params, or a reordering of StepParams against K1's batched argument loads, changes x, y
or orientation of the covariance cases and fails both compares.)"""
import ctypes as C
import math

import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import project_cases as P
import project_ref as R
import synthetic as S
from parity_util import assert_bit_identical, info_tuple

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_project_alone(gpu_mod, oracle, case):
    cfg = P.config(case)
    gpu, orc = gpu_mod.GpuFilter(cfg), O.OracleFilter(cfg, O.SUM_CONTRACT)
    mw, count, got = P.run_project(gpu, lambda f: f.sync(), case)
    mw_o, count_o, want = P.run_project(orc, lambda f: f.info(), case)
    assert (mw, count) == (mw_o, count_o) and mw == P.warm_max_weight(case.n, case.rough)
    assert_bit_identical(got, want, f"{case.name} project")
    pa, st = P.particles(case), P.step_input(case)
    idx = P.sample_indices(case.n)
    for mode in ("contract", "exact"):
        _, res = R.project(cfg, pa, st, mw, count, idx, mode=mode)
        R.check(res, got, f"{case.name} device ({mode})")
    zs = [R.zsigma_expected(float(v), 2.0 * case.pez) for v in pa.zsigma]       # every particle, not the sample
    assert P.same_bits(got.zsigma, np.array(zs)), f"{case.name}: zsigma is not the exactly rounded root everywhere"
    gpu.close()


def run_steps(f, info_fn, case, scan=None):
    """the warm update, the case's particles, two steps that update and resample: the second
    step's kernel gathers the first one's resample.  Returns what every stage left."""
    out = []
    P.warm_up(f, info_fn, case)
    f.upload(P.particles(case))
    st = P.step_input(case)
    for k in range(2):
        assert f.step(st)
        i = info_fn(f)
        out.append((info_tuple(i), f.download(), f.ancestors() if i.resampled else None))
        if scan is not None:
            f.map_update(scan)
    return out


def assert_same_steps(got, want, label):
    for k, ((gi, gp, ga), (wi, wp, wa)) in enumerate(zip(got, want)):
        assert_bit_identical(gp, wp, f"{label} step {k}")
        assert repr(gi) == repr(wi), f"{label} step {k}: info {gi} != {wi}"
        assert (ga is None) == (wa is None) and (ga is None or np.array_equal(ga, wa)), f"{label} step {k}: ancestors differ"
    assert got[1][0][6], f"{label}: the second step did not resample"


@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_step_with_pending_resample(gpu_mod, oracle, case):
    cfg = P.config(case, step=True)
    gpu, orc = gpu_mod.GpuFilter(cfg), O.OracleFilter(cfg, O.SUM_CONTRACT)
    got = run_steps(gpu, lambda f: f.sync(), case)
    assert_same_steps(got, run_steps(orc, lambda f: f.info(), case), case.name)
    assert got[0][0][6], f"{case.name}: the first step did not resample"
    gpu.close()


@pytest.mark.parametrize("name", P.MAPS_CASES)
def test_with_particle_maps(gpu_mod, oracle, name):
    """per-particle maps: the project alone, then the two steps with a scan merged after each"""
    case = P.CASE_BY_NAME[name]
    cfg = P.config(case)
    cfg.flags |= A.FLAG_PARTICLE_MAPS
    gpu, orc = gpu_mod.GpuFilter(cfg), O.OracleFilter(cfg, O.SUM_CONTRACT)
    a = P.run_project(gpu, lambda f: f.sync(), case)
    b = P.run_project(orc, lambda f: f.info(), case)
    assert a[:2] == b[:2]
    assert_bit_identical(a[2], b[2], f"{name} maps project")
    gpu.close()
    cfg = P.config(case, step=True)
    cfg.flags |= A.FLAG_PARTICLE_MAPS
    cfg.local_map_pages = 48
    gpu, orc = gpu_mod.GpuFilter(cfg), O.OracleFilter(cfg, O.SUM_CONTRACT)
    got = run_steps(gpu, lambda f: f.sync(), case, S.scan_patches())
    assert_same_steps(got, run_steps(orc, lambda f: f.info(), case, S.scan_patches()), f"{name} maps")
    gpu.close()


@pytest.mark.parametrize("what", ["nan_mean", "inf_cov", "nan_cov_offdiag", "negative_diagonal"])
def test_rejects_inputs_outside_the_domain(gpu_mod, oracle, what):
    """ESLAM_ERR_INVALID_ARG from project, update and step, before any launch: the particles and
    the project counter are unchanged and the filter goes on working"""
    from test_project_ref import bad_input
    case = P.CASE_BY_NAME["cov_full"]
    gpu = gpu_mod.GpuFilter(P.config(case))
    P.warm_up(gpu, lambda f: f.sync(), case)
    before, count = gpu.download(), gpu.rng_state().project_count
    st = bad_input(case, what)
    for call in (gpu.project, gpu.update, gpu.step):
        with pytest.raises(gpu_mod.EslamError) as e:
            call(st)
        assert e.value.code == A.ERR_INVALID_ARG
    after = gpu.download()
    for fld in P.FIELDS:
        assert P.same_bits(getattr(after, fld), getattr(before, fld)), fld
    assert gpu.rng_state().project_count == count
    gpu.project(P.step_input(case))
    gpu.close()
