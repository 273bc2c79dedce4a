"""The CPU restatement of the pose estimate's moments (tests/c/moments_ref.c, the rule of DESIGN.md
5i) against an independent numpy float64 computation (np.arctan2 of the weighted sine and cosine
sums, deviations wrapped with np.angle, np.cov with aweights) and exact cases.  The device is
compared with the restatement bit for bit in tests/test_gpu_pose_moments.py."""
import numpy as np
import pytest

import eslam_abi as A
import moments_cases as M
import moments_ref as R

# Largest disagreement of the restatement and numpy on CLOUDS and the gated case, in the units of
# `disagreement` below, measured with this file (printed by the tests): 1.6e-13, the means of the
# blobs at (1000, -2000) -- two ulps of 2000 over a cloud 2.9 m across; every other term is below
# 3e-16.  The two differ by the ulps of their sin, cos and atan2 and by the order of their sums;
# 16 x the measured value leaves room for another libm, and the bound is never below 1e-12 (the
# GMM test's margin for the same kind of comparison).
MEASURED = 1.6e-13
BOUND = max(16.0 * MEASURED, 1e-12)
N = 3000


def disagreement(m, want, c):
    """largest difference: means relative to the cloud's extent, covariances to its square, every
    yaw term (the mean's and the covariance's yaw row and column), R, the weight share and
    z_within absolute, the effective count relative to itself"""
    ext = max(np.ptp(c["x"][np.isfinite(c["x"])]), np.ptp(c["y"][np.isfinite(c["y"])]), np.ptp(c["z"][np.isfinite(c["z"])]), 1.0)
    s = np.array([ext, ext, ext, 1.0])
    mean, cov = np.array(list(m.mean)), np.array(list(m.cov)).reshape(4, 4)
    dm = np.abs(mean - want["mean"])
    dm[3] = min(dm[3], abs(dm[3] - 2.0 * np.pi))                  # a mean on the cut may come out at either end
    s2 = np.outer(s, s)
    s2[3, :] = s2[:, 3] = 1.0
    return max((dm / s).max(), (np.abs(cov - want["cov"]) / s2).max(), abs(m.z_within - want["z_within"]),
               abs(m.yaw_resultant - want["yaw_resultant"]), abs(m.weight_share - want["weight_share"]),
               abs(m.effective - want["effective"]) / want["effective"])


def ref(c, gate=None, rows=0):
    rc, m = R.moments(*[c[f] for f in M.FIELDS], gate=gate, sum_chunk_rows=rows)
    assert rc == 0
    return m


CLOUDS = {
    "blob": lambda: M.blob(N, seed=1),
    "across the cut": lambda: M.across_the_cut(N, seed=2),
    "whole turns": lambda: M.whole_turns(M.across_the_cut(N, seed=2), seed=3),
    "correlated": lambda: M.correlated(N, seed=4),
}


@pytest.mark.parametrize("name", list(CLOUDS))
def test_restatement_equals_numpy(name):
    c = CLOUDS[name]()
    m = ref(c)
    want = M.numpy_moments(c)
    assert (m.particles_counted, m.particles_gated_out, m.particles_skipped) == (N, 0, 0)
    d = disagreement(m, want, c)
    print(f"moments restatement vs numpy, {name}: {d:.3e} (bound {BOUND:.3e})")
    assert d <= BOUND, (name, d)
    cov = np.array(list(m.cov)).reshape(4, 4)
    assert np.array_equal(cov, cov.T) and -np.pi < m.mean[3] <= np.pi
    assert m.weight_share == 1.0


def test_blob_is_where_it_was_planted():
    m = ref(M.blob(N, seed=1))
    assert abs(m.mean[0] - 1000.0) < 0.05 and abs(m.mean[1] + 2000.0) < 0.05 and abs(m.mean[2] - 0.2) < 0.005
    assert abs(m.mean[3] - 0.3) < 0.01 and 0.99 < m.yaw_resultant <= 1.0 and 0.5 * N < m.effective <= N


@pytest.mark.parametrize("name", ["across the cut", "whole turns"])
def test_circular_mean_holds_across_the_cut(name):
    """the yaw mean is at +-pi (within 0.05 + the sample's own error); the linear mean of theta is not"""
    c = CLOUDS[name]()
    m = ref(c)
    assert np.pi - abs(m.mean[3]) <= 0.05 + 0.02
    linear = float((c["w"] * c["theta"]).sum() / c["w"].sum())
    assert np.pi - abs(linear) > 0.5
    assert abs(m.cov[15] - 0.09) < 0.015                          # sigma 0.3 survives the wrap


def test_whole_turns_change_the_result_by_rounding_only():
    a = M.across_the_cut(N, seed=2)
    b = M.whole_turns(a, seed=3)
    ma, mb = ref(a), ref(b)
    d = disagreement(mb, {"mean": np.array(list(ma.mean)), "cov": np.array(list(ma.cov)).reshape(4, 4), "z_within": ma.z_within,
                          "yaw_resultant": ma.yaw_resultant, "effective": ma.effective, "weight_share": ma.weight_share}, a)
    assert d <= 1e-13, d                                          # theta + 6 pi carries 8 more ulps than theta


def test_planted_x_yaw_correlation_is_recovered():
    m = ref(M.correlated(N, seed=4))
    cov = np.array(list(m.cov)).reshape(4, 4)
    rho = cov[0, 3] / np.sqrt(cov[0, 0] * cov[3, 3])
    assert abs(rho - 0.8) <= 0.05, rho


def test_gate_selects_one_cluster():
    c, gate, member = M.two_clusters(N, seed=5)
    m = ref(c, gate)
    ins = M.inside(c, gate)
    assert not (ins & ~member).any() and (ins & member).sum() >= 0.99 * member.sum()
    want = M.numpy_moments(c, ins)
    assert (m.particles_counted, m.particles_gated_out, m.particles_skipped) == (int(ins.sum()), int((~ins).sum()), 0)
    d = disagreement(m, want, c)
    print(f"moments restatement vs numpy, gated: {d:.3e} (bound {BOUND:.3e})")
    assert d <= BOUND, d
    assert abs(m.mean[0] - 20.0) < 0.05 and abs(m.mean[3] - 3.0) < 0.02 and 0.0 < m.weight_share < 1.0
    # the gate never moves the scale: the exponent is that of the ungated call
    assert m.weight_exp == ref(c).weight_exp
    # a circle around the other cluster
    other = ref(c, A.PoseGate((26.0, -7.5), (1.0, 0.0, 1.0), 4.0))
    assert other.particles_counted == int((~member).sum()) and abs(other.mean[3] + 2.0) < 0.03


def all_bits(m):
    return m.as_tuple()


def test_weight_scaling_moves_weight_exp_and_no_other_bit():
    c, gate, _ = M.two_clusters(1000, seed=6)
    for g in (None, gate):
        base = all_bits(ref(c, g))
        for k in (-900, 900):
            d = dict(c, w=np.ldexp(c["w"], k))
            got = all_bits(ref(d, g))
            assert got[:-2] == base[:-2] and got[-2] == base[-2] + k, (k, g is not None)


def test_no_valid_particle():
    c = M.blob(70, seed=7)
    c["w"][:] = 0.0
    m = ref(c)
    assert (m.particles_counted, m.particles_gated_out, m.particles_skipped) == (0, 0, 70)
    assert not any(m.doubles()) and m.weight_exp == 0


def test_every_particle_gated_out():
    c = M.blob(70, seed=7)
    m = ref(c, A.PoseGate((0.0, 0.0), (1.0, 0.0, 1.0), 1.0))
    assert (m.particles_counted, m.particles_gated_out, m.particles_skipped) == (0, 70, 0)
    assert not any(m.doubles()) and m.weight_exp == ref(c).weight_exp


def test_each_kind_of_skipped_particle_is_counted_once():
    base = M.blob(200, seed=8)
    for f, v in [("x", np.nan), ("theta", np.inf), ("zsigma", np.nan), ("w", 0.0), ("w", -1e-7), ("w", np.nan)] + M.SKIP_KINDS:
        c = {k: a.copy() for k, a in base.items()}
        c[f][57] = v
        m = ref(c)
        assert (m.particles_counted, m.particles_skipped) == (199, 1), (f, v)
        ok = np.ones(200, bool)
        ok[57] = False
        assert disagreement(m, M.numpy_moments({k: a[ok] for k, a in base.items()}), base) <= BOUND, (f, v)
    c, cnt = M.with_skipped(base, seed=9)
    m = ref(c)
    assert m.particles_skipped == cnt and m.particles_counted == 200 - cnt
    assert disagreement(m, M.numpy_moments(c), base) <= BOUND


def test_identical_particles():
    n = 300
    c = {"x": np.full(n, 12.5), "y": np.full(n, -3.25), "z": np.full(n, 0.2), "theta": np.full(n, 2.5), "zsigma": np.full(n, 0.01),
         "w": np.full(n, 0.01)}
    m = ref(c)
    assert np.abs(np.array(list(m.cov))).max() <= BOUND and abs(m.yaw_resultant - 1.0) <= BOUND
    assert abs(m.mean[0] - 12.5) <= BOUND * 12.5 and abs(m.mean[3] - 2.5) <= BOUND and abs(m.z_within - 1e-4) <= BOUND
    assert abs(m.effective - n) <= 1e-9


def test_refused_arguments():
    c = M.blob(10, seed=1)
    bad = [A.PoseGate((0, 0), (1.0, 1.0, 1.0), 9.0), A.PoseGate((0, 0), (1.0, 2.0, 1.0), 9.0), A.PoseGate((0, 0), (-1.0, 0.0, -1.0), 9.0),
           A.PoseGate((0, 0), (0.0, 0.0, 1.0), 9.0), A.PoseGate((0, 0), (1.0, 0.0, 1.0), -1.0), A.PoseGate((0, 0), (1.0, 0.0, 1.0), np.inf),
           A.PoseGate((0, 0), (1.0, 0.0, 1.0), np.nan), A.PoseGate((np.nan, 0), (1.0, 0.0, 1.0), 9.0),
           A.PoseGate((0, np.inf), (1.0, 0.0, 1.0), 9.0), A.PoseGate((0, 0), (np.inf, 0.0, 1.0), 9.0),
           A.PoseGate((0, 0), (1e200, 0.0, 1e200), 9.0), A.PoseGate((0, 0), (np.nan, 0.0, 1.0), 9.0)]
    for g in bad:
        assert R.moments(*[c[f] for f in M.FIELDS], gate=g)[0] == A.ERR_INVALID_ARG, (list(g.cov), g.chi2, list(g.centre))
    assert R.moments(*[c[f] for f in M.FIELDS], gate=A.PoseGate((0, 0), (1.0, 0.0, 1.0), 0.0))[0] == 0
    assert R.moments(*[c[f][:0] for f in M.FIELDS])[0] == A.ERR_NOT_INITIALISED
