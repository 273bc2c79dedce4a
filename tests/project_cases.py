"""The predict-step cases shared by test_project_ref.py (CPU oracle) and test_gpu_project.py
(device): odometry covariances with every off-diagonal term, the Cholesky's pivot rules, body
orientations and pose deltas with every component, the yaw penalty at its edge, the slip compare,
the spread on either side of its threshold and zsigma at the edges of the device's square root
(test infrastructure).

A case is a configuration, the particles to upload, one step input and a way to the previous
update's max_weight: `run_project` runs one real update on a warm particle set first (the update
does not read the spread threshold), takes max_weight from it, uploads the case's particles and
projects.  The spread cases put the threshold at, above and below that max_weight."""
import functools
import math

import numpy as np

import eslam_abi as A
import oracle_ffi as O
import synthetic as S

FIELDS = ("x", "y", "orientation", "zpos", "zsigma", "weight", "mprob", "floating", "n_contact_points")
N_ONE, N_RAGGED, N_LARGE = 1, 4099, 8192          # 4099: a ragged last row, several rows per chunk
SEED = 977
MDEV = 15 * math.pi / 180.0                       # the default maxYawDeviation

SIGMA = (0.02, 0.01, 0.004)
RHO = dict(xy=0.8, xth=-0.6, yth=0.3)             # distinct magnitudes: no two L entries exchange unnoticed
# These three correlations are no covariance's: 1 + 2 (0.8)(-0.6)(0.3) - 0.64 - 0.36 - 0.09 < 0, the
# matrix is indefinite and its third pivot negative (L22 = 0, L10, L20 and L21 all non-zero).  It
# stays a case as it is (the sampler must take what an odometry hands it); with rho_y_theta = -0.3
# the determinant is 0.198 and the matrix positive definite: the case whose L has all six entries
# and the one whose sample moments can be compared with mu and Sigma.
RHO_SPD = dict(xy=0.8, xth=-0.6, yth=-0.3)


def cov_of(sigma, xy=0.0, xth=0.0, yth=0.0):
    sx, sy, st = sigma
    a, b, c = xy * sx * sy, xth * sx * st, yth * sy * st
    return [sx * sx, a, b, a, sy * sy, c, b, c, st * st]


def rank1_cov():
    """sigma = (2^-6, 2^-7, 2^-8), every correlation 1: every entry and every step of the
    factorisation is exact, the second and third pivots are exactly 0"""
    s = (2.0 ** -6, 2.0 ** -7, 2.0 ** -8)
    return [s[i] * s[j] for i in range(3) for j in range(3)]


def tiny_negative_cov():
    """S11 eight ulps below fl(L10^2): the second pivot is about -1e-19 in doubles, and negative
    in exact arithmetic too (fl(L10^2) is within 3 ulps of S10^2 / S00)"""
    c = cov_of(SIGMA, xy=0.85, xth=-0.6, yth=0.3)
    l10 = c[3] / math.sqrt(c[0])
    s11 = l10 * l10
    for _ in range(8):
        s11 = math.nextafter(s11, 0.0)
    c[4] = s11
    assert c[4] - l10 * l10 < 0.0
    return c


def upper_differs_cov():
    """the lower triangle of the full matrix, something else above the diagonal"""
    c = cov_of(SIGMA, **RHO)
    c[1], c[2], c[5] = 7.0, -3.0, 11.0
    return c


COVS = {
    "full": cov_of(SIGMA, **RHO),
    "full_spd": cov_of(SIGMA, **RHO_SPD),
    "only_xy": cov_of(SIGMA, xy=RHO["xy"]),
    "only_xth": cov_of(SIGMA, xth=RHO["xth"]),
    "only_yth": cov_of(SIGMA, yth=RHO["yth"]),
    "zero": [0.0] * 9,
    "rank1": rank1_cov(),
    "zero_first_pivot": [0.0, 0, 0, 1e-5, 1e-4, 0, -2e-6, 1.2e-5, 1.6e-5],
    "tiny_negative": tiny_negative_cov(),
    "upper_differs": upper_differs_cov(),
    "large": cov_of((0.3, 0.2, 0.004), xy=0.9),
    "no_theta": [1e-4, 0, 0, 2e-5, 1e-4, 0, 0, 0, 0],      # third row of L zero: dth = mu2
}
for _c in COVS.values():
    assert all(math.isfinite(v) for v in _c) and min(_c[0], _c[4], _c[8]) >= 0.0


class Case:
    def __init__(self, name, n=N_RAGGED, cov="full", yaw=0.2, mean=(0.02, 0.005, 0.002), slip=0.05, mdev=MDEV,
                 spread=0.5, hash_use=0, pez=1e-4, particles="random", rough=False, roll=0.3, pitch=-0.25):
        self.name, self.n, self.cov, self.yaw, self.mean, self.slip, self.mdev = name, n, cov, yaw, mean, slip, mdev
        self.spread, self.hash_use, self.pez, self.particles, self.rough = spread, hash_use, pez, particles, rough
        self.roll, self.pitch = roll, pitch

    def __repr__(self):
        return self.name


CASES = [
    Case("cov_full"),
    Case("cov_full_spd", cov="full_spd"),
    Case("cov_only_xy", cov="only_xy"),
    Case("cov_only_xth", cov="only_xth"),
    Case("cov_only_yth", cov="only_yth"),
    Case("cov_zero", cov="zero"),
    Case("cov_rank1", cov="rank1"),
    Case("cov_zero_first_pivot", cov="zero_first_pivot"),
    Case("cov_tiny_negative_pivot", cov="tiny_negative"),
    Case("cov_upper_differs", cov="upper_differs"),
    Case("cov_large", n=N_LARGE, cov="large", rough=True, yaw=0.0),
    Case("one_particle", n=N_ONE),
    Case("yaw_0", yaw=0.0, n=N_ONE),
    Case("yaw_2.5", yaw=2.5),
    Case("yaw_near_pi", yaw=math.pi - 1e-9),
    Case("yaw_near_minus_pi", yaw=-math.pi + 1e-9),
    Case("penalty_edges", cov="no_theta", mean=(0.02, 0.005, 0.0), yaw=0.0, roll=0.0, pitch=0.0, particles="yaw_edges"),
    Case("penalty_unwrapped", cov="no_theta", mean=(0.02, 0.005, 0.0), yaw=-math.pi + 0.01, particles="unwrapped"),
    Case("penalty_off_zero", mdev=0.0, particles="yaw_edges"),
    Case("penalty_off_negative", mdev=-0.1, particles="yaw_edges"),
    Case("slip_0", slip=0.0),
    Case("slip_1", slip=1.0),
    Case("slip_at_the_draw", slip="draw"),                 # slipFactor = particle 0's slip uniform: u < u is false
    Case("spread_above", spread=0.5),                      # threshold = max_weight / 2: no spread
    Case("spread_at", spread=1.0),                         # threshold = max_weight: x >= beta, no spread
    Case("spread_below", spread=2.0),                      # threshold = 2 max_weight: spread 1/2
    Case("spread_below_hash", spread=2.0, hash_use=1),     # a hash: no spread
    Case("zsigma_zvar_0", pez=0.0, particles="zsigma"),
    Case("zsigma_zvar_2e-4", pez=1e-4, particles="zsigma"),
    Case("zsigma_zvar_2^-767", pez=2.0 ** -768, particles="zsigma"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
MAPS_CASES = ("cov_full", "cov_full_spd", "cov_rank1", "cov_large")       # the set run with per-particle maps


def zsigma_edges():
    """0, the smallest denormal, 2^-384 and sqrt(2^-767) with their neighbours (zs^2 + z_var on both
    sides of the 2^-767 at which the device's square root changes path), ordinary values, squares
    near DBL_MAX, squares that overflow"""
    r = 2.0 ** -383.5
    out = [0.0, 5e-324, 2.0 ** -384, math.nextafter(2.0 ** -384, 0.0), math.nextafter(2.0 ** -384, 1.0)]
    v = r
    for _ in range(3):
        v = math.nextafter(v, 0.0)
    for _ in range(7):
        out.append(v)
        v = math.nextafter(v, 1.0)
    return out + [2.0 ** -383, 2.0 ** -400, 2.0 ** -511, 1e-3, 1.0, 1e150, 1.3e154, 1.3407807929942596e154, 1e200]


def yaw_edges():
    """theta - yaw at exactly maxYawDeviation, one ulp above and below it, on both signs (the
    case has yaw = 0 and delta.theta = 0)"""
    up, dn = math.nextafter(MDEV, 4.0), math.nextafter(MDEV, 0.0)
    return [MDEV, up, dn, -MDEV, -up, -dn]


def particles(case):
    """the particles a case uploads: seeded poses on the map, positive weights of many scales"""
    n = case.n
    rng = np.random.default_rng(3000 + n)
    pa = A.ParticleArrays(n)
    pa.x[:] = rng.normal(0, 0.2, n)
    pa.y[:] = rng.normal(0, 0.2, n)
    pa.orientation[:] = rng.normal(0, 0.3, n)
    pa.zpos[:] = 0.18 + rng.normal(0, 0.01, n)
    pa.zsigma[:] = 0.25
    pa.weight[:] = np.ldexp(0.5 + rng.integers(0, 1 << 52, n) * 2.0 ** -53, rng.integers(-20, 1, n))
    pa.mprob[:] = 1.0
    pa.floating[:] = 1
    if case.particles == "yaw_edges":
        e = yaw_edges()
        pa.orientation[:len(e)] = e[:n]
    elif case.particles == "unwrapped":
        pa.orientation[:min(n, 64):2] = math.pi - 0.01          # against yaw = -pi + 0.01: 2 pi - 0.02 apart
    elif case.particles == "zsigma":
        e = zsigma_edges()
        k = np.arange(n)
        pa.zsigma[:] = np.where((k >= 64) & (k < 128), 0.25, np.array(e)[k % len(e)])   # one row of ordinary values
    return pa


def step_input(case):
    st = S.step_stream(1)[0]
    st.body2odometry_rot[:] = S.quat_from_rpy(case.roll, case.pitch, case.yaw)
    st.pose_delta_trans[:] = [0.02, 0.013, -0.007]
    st.position_error_zz = case.pez
    st.sample_mean[:] = list(case.mean)
    st.sample_cov[:] = COVS[case.cov]
    return st


def full_covariance(st, k):
    """a full covariance (even k: the positive definite one, odd k: the indefinite one), a mean
    and a pose delta with every component, put into step k of another stream
    (dist_scenarios.py's full_cov)"""
    st.pose_delta_trans[:] = [st.pose_delta_trans[0], 0.013, -0.007]
    st.sample_mean[1] = 0.005
    st.sample_cov[:] = COVS["full" if k % 2 else "full_spd"]
    return st


@functools.lru_cache(maxsize=None)
def grid(rough):
    return S.rough_map(cells=120) if rough else S.flat_map(cells=120)


def warm_particles(n):
    """the particles of the update that precedes the step: standing on the map"""
    rng = np.random.default_rng(4000 + n)
    pa = A.ParticleArrays(n)
    pa.x[:] = rng.normal(0, 0.1, n)
    pa.y[:] = rng.normal(0, 0.1, n)
    pa.orientation[:] = rng.normal(0, 0.05, n)
    pa.zpos[:] = 0.18
    pa.zsigma[:] = 0.05
    pa.weight[:] = 1.0 / n
    pa.mprob[:] = 1.0
    pa.floating[:] = 1
    return pa


def slip_uniform(project_count, gi):
    """the slip test's uniform of global particle gi: (word + 1/2) 2^-32 of word 0 of call 1"""
    import ctypes as C
    w = (C.c_uint32 * 4)()
    O.lib().or_dm_philox(SEED, 1, project_count, gi, 1, w)
    return (int(w[0]) + 0.5) * 2.0 ** -32


def base_config(case, step=False):
    cfg = A.default_config()
    cfg.seed = SEED
    cfg.particle_count = case.n
    cfg.min_effective = 0                         # the warm update does not resample
    cfg.slip_factor = slip_uniform(0, 0) if case.slip == "draw" else case.slip
    cfg.max_yaw_deviation = case.mdev
    cfg.hash_use = case.hash_use
    cfg.flags |= A.FLAG_RECORD_ANCESTORS
    if step:
        S.bench_config(cfg, case.n)               # every step updates and resamples
    return cfg


@functools.lru_cache(maxsize=None)
def warm_max_weight(n, rough):
    """max_weight after the warm update, from the CPU oracle (the update reads neither the spread
    threshold nor anything else a case changes)"""
    case = Case("warm", n=n, rough=rough)
    f = O.OracleFilter(base_config(case), O.SUM_CONTRACT)
    return warm_up(f, lambda g: g.info(), case)


def warm_up(f, info_fn, case):
    f.set_map(grid(case.rough))
    f.upload(warm_particles(case.n))
    rc = f.update(S.step_stream(1)[0])
    assert not rc, rc
    return float(info_fn(f).max_weight)


def config(case, step=False):
    cfg = base_config(case, step)
    mw = warm_max_weight(case.n, case.rough)
    assert 0.0 < mw < 1e300
    cfg.spread_threshold = mw * case.spread       # a power of two: exact (1/2 unless the case says: no spread)
    return cfg


def run_project(f, info_fn, case):
    """one real update, then the case's particles uploaded and projected.  Returns (the previous
    max_weight, the project counter the draws are keyed by, the particles after the step)"""
    mw = warm_up(f, info_fn, case)
    f.upload(particles(case))
    count = int(f.rng_state().project_count)
    rc = f.project(step_input(case))
    assert not rc, rc
    return mw, count, f.download()


def sample_indices(n):
    """the particles compared with project_ref (mpmath is slow; the draws are keyed by index and
    every particle runs the same code): both ends whole, a stride between them"""
    if n <= 320:
        return list(range(n))
    return sorted(set(range(160)) | set(range(n - 160, n)) | set(range(160, n - 160, 13)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return bool(np.array_equal(a, b))
