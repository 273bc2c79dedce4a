"""The predict step of the CPU oracle (or_project / or_prepare) against project_ref.py, the mpmath
restatement of PoseEstimator::project, on every case of project_cases.py: x, y, orientation and
zpos within the derived bounds (the contract's normals: the tight bound; Box-Muller in mpmath: plus
2^-22 of the radius per normal), zsigma and the penalised weight exactly; and the moments of the
sampled motion against the mean and covariance that went in."""
import math

import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import project_cases as P
import project_ref as R
import synthetic as S

WORST = {"contract": {}, "exact": {}}


def oracle_run(case):
    f = O.OracleFilter(P.config(case), O.SUM_CONTRACT)
    return f, P.run_project(f, lambda g: g.info(), case)


@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_oracle_project_against_reference(oracle, case):
    f, (mw, count, got) = oracle_run(case)
    cfg, pa, st = P.config(case), P.particles(case), P.step_input(case)
    assert mw == P.warm_max_weight(case.n, case.rough)
    idx = P.sample_indices(case.n)
    for mode in ("contract", "exact"):
        prep, res = R.project(cfg, pa, st, mw, count, idx, mode=mode)
        R.check(res, got, f"{case.name} ({mode})", WORST[mode])
    # what the case is there for does happen
    L = [[float(prep.L[i][j].v) for j in range(3)] for i in range(3)]
    assert prep.do_spread == (case.name == "spread_below")
    if case.particles == "yaw_edges":
        want = [False, True, False, False, True, False] if case.mdev > 0 else [False] * 6
        assert [r.penalised for r in res[:len(want)]] == want[:case.n]
    if case.particles == "unwrapped":
        assert all(res[i].penalised for i in range(0, 64, 2))
    if case.name == "slip_0":
        assert not any(r.slipped for r in res)
    if case.name == "slip_1":
        assert all(r.slipped for r in res)
    if case.name == "slip_at_the_draw":
        assert count == 0 and not res[0].slipped and any(r.slipped for r in res)
    if case.name == "cov_full_spd":
        assert all(L[i][j] != 0.0 for i in range(3) for j in range(i + 1))
    if case.name == "cov_full":
        assert L[1][0] != 0.0 and L[2][0] != 0.0 and L[2][1] != 0.0 and L[2][2] == 0.0     # indefinite: see project_cases.RHO
        assert any(r.slipped for r in res) and not all(r.slipped for r in res)
        assert any(r.penalised for r in res) and not all(r.penalised for r in res)
    if case.cov in ("rank1", "tiny_negative"):
        assert L[1][0] != 0.0 and L[2][0] != 0.0 and L[1][1] == 0.0 and L[2][1] == 0.0
    if case.cov == "zero_first_pivot":
        assert L[0][0] == L[1][0] == L[2][0] == 0.0 and L[2][1] != 0.0
    # every other field is untouched
    for fld in ("mprob", "floating", "n_contact_points"):
        assert P.same_bits(getattr(got, fld), getattr(pa, fld))


def test_worst_case_table(oracle):
    """prints the worst error over the cases in units of the bound (the table of project_ref.py);
    runs the cases itself when it is run alone"""
    if not WORST["contract"]:
        for case in P.CASES:
            test_oracle_project_against_reference(oracle, case)
    for mode in ("contract", "exact"):
        print(mode, {f: round(v, 3) for f, v in sorted(WORST[mode].items())})
        assert all(v <= 1.0 for v in WORST[mode].values())


def test_sqrt_rn_is_the_correctly_rounded_root():
    """project_ref.sqrt_rn (integers) on squares, their neighbours and the device's switch point"""
    for v in (0.0, 5e-324, 2.0 ** -767, math.nextafter(2.0 ** -767, 0.0), 2.0, 0.0625, 1e-300, 1.7976931348623157e308):
        r = R.sqrt_rn(v)
        lo, hi = math.nextafter(r, 0.0), math.nextafter(r, math.inf)
        from fractions import Fraction as F
        assert ((F(lo) + F(r)) / 2) ** 2 <= F(v) <= ((F(r) + F(hi)) / 2) ** 2 or v == 0.0
    assert R.sqrt_rn(4.0) == 2.0 and R.sqrt_rn(2.0 ** -1074) == 2.0 ** -537 and R.sqrt_rn(math.inf) == math.inf
    assert R.zsigma_expected(1e200, 0.0) == math.inf and R.zsigma_expected(0.0, 0.0) == 0.0


def moments_run(slip):
    n = 65536
    case = P.Case("moments", n=n, cov="full_spd", slip=slip, mdev=0.0)
    cfg = P.base_config(case)
    cfg.spread_threshold = 0.0                    # max_weight = 0 >= the threshold: no spread
    f = O.OracleFilter(cfg, O.SUM_CONTRACT)
    f.set_threads(min(8, __import__("os").cpu_count() or 1))
    pa = A.ParticleArrays(n)
    x0, y0, th0 = 0.3, -0.2, 0.7
    pa.x[:], pa.y[:], pa.orientation[:] = x0, y0, th0
    pa.zsigma[:], pa.weight[:] = 0.25, 1.0 / n
    f.upload(pa)
    st = P.step_input(case)
    assert f.project(st) == 0
    got = f.download()
    ex, ey = got.x - x0, got.y - y0
    c, s_ = math.cos(th0), math.sin(th0)
    return n, st, np.stack([c * ex + s_ * ey, -s_ * ex + c * ey, got.orientation - th0])


def test_moments_of_the_sampled_motion(oracle):
    """identical start poses, no slip, no spread, the full covariance: the body-frame deltas have
    sample mean and covariance within 5 standard errors of mu and Sigma (the positive definite
    matrix of project_cases.py: the indefinite one is no sample's covariance).  The contract's normals are
    within 2^-22 max(1, r) of exact ones, r <= sqrt(-2 log 2^-33) < 6.8: a delta moves by at most
    e_i = 6.8 2^-22 sum_j |L_ij|, a mean by e_i, a covariance by 2 (e_i s_j + e_j s_i) + e_i e_j"""
    n, st, d = moments_run(0.0)
    mu, Sg = np.array(list(st.sample_mean)), np.array(list(st.sample_cov)).reshape(3, 3)
    Sg = np.tril(Sg) + np.tril(Sg, -1).T
    L = np.linalg.cholesky(Sg)
    e = 6.8 * 2.0 ** -22 * np.abs(L).sum(axis=1)
    sd = np.sqrt(np.diag(Sg))
    mean, cov = d.mean(axis=1), np.cov(d, bias=True)
    for i in range(3):
        assert abs(mean[i] - mu[i]) <= 5 * math.sqrt(Sg[i, i] / n) + e[i], (i, mean[i], mu[i])
        for j in range(3):
            tol = 5 * math.sqrt((Sg[i, i] * Sg[j, j] + Sg[i, j] ** 2) / n) + 2 * (e[i] * sd[j] + e[j] * sd[i]) + e[i] * e[j]
            assert abs(cov[i, j] - Sg[i, j]) <= tol, (i, j, cov[i, j], Sg[i, j])


def test_slip_halves_the_mean_of_dy(oracle):
    """slipFactor 1: dy is multiplied by an independent uniform, E = mu1 / 2, Var = (S11 + mu1^2) / 3
    - mu1^2 / 4; dx and dth keep their means"""
    n, st, d = moments_run(1.0)
    mu, S11 = list(st.sample_mean), st.sample_cov[4]
    var = (S11 + mu[1] ** 2) / 3 - mu[1] ** 2 / 4
    assert abs(d[1].mean() - mu[1] / 2) <= 5 * math.sqrt(var / n) + 1e-7
    assert abs(d[0].mean() - mu[0]) <= 5 * math.sqrt(st.sample_cov[0] / n) + 1e-7
    assert abs(d[2].mean() - mu[2]) <= 5 * math.sqrt(st.sample_cov[8] / n) + 1e-7


@pytest.mark.parametrize("what", ["nan_mean", "inf_cov", "nan_cov_offdiag", "negative_diagonal"])
def test_oracle_rejects_inputs_outside_the_domain(oracle, what):
    """a non-finite sample_mean or sample_cov entry or a negative diagonal: ESLAM_ERR_INVALID_ARG
    from project, update and step alike, the particles unchanged (include/eslam_gpu.h)"""
    case = P.CASE_BY_NAME["cov_full"]
    f = O.OracleFilter(P.config(case), O.SUM_CONTRACT)
    P.warm_up(f, lambda g: g.info(), case)
    before = f.download()
    st = bad_input(case, what)
    import ctypes as C
    assert f.project(st) == A.ERR_INVALID_ARG and f.update(st) == A.ERR_INVALID_ARG
    assert f.L.or_step(f.h, C.byref(st), C.byref(C.c_int(0))) == A.ERR_INVALID_ARG
    after = f.download()
    for fld in P.FIELDS:
        assert P.same_bits(getattr(after, fld), getattr(before, fld)), fld
    assert f.rng_state().project_count == 0


def bad_input(case, what):
    st = P.step_input(case)
    if what == "nan_mean":
        st.sample_mean[1] = math.nan
    elif what == "inf_cov":
        st.sample_cov[0] = math.inf
    elif what == "nan_cov_offdiag":
        st.sample_cov[2] = math.nan               # above the diagonal: unread by the factor, rejected all the same
    else:
        st.sample_cov[4] = -1e-12
    return st
