"""PoseEstimator::project restated in mpmath (test infrastructure).

Written from src/PoseEstimator.cpp:184-242 and DESIGN.md 2 (the draw layout), not from the oracle's
or the kernel's code, and with nothing of eslam_detmath.h in it.  What it takes from the build is
the raw Philox words of a particle (`or_dm_philox`, pinned by the Random123 vectors) and, in
`contract` mode, the two normals the contract makes of a pair of words (`or_dm` 18 / 19, tied to
mpmath by test_detmath.py::test_box_muller32_normals).

The step, per PoseEstimator.cpp:

  yaw       = atan2(R10, R00) of R(q) (base::getYaw; 0 when sqrt(R22^2 + R21^2) <= 1e-12)
  z_delta   = (R(q) pose_delta)_z,  z_var = 2 position_error_zz
  L         = lower Cholesky factor of sample_cov, read from the LOWER triangle S[i*3+j], i >= j;
              a pivot d <= 0 gives a zero column (the rule the code states)
  spread    = weightingFunction(max_weight, 0, spreadThreshold, 0): 1 below 0, 1 - x / beta below
              beta, 0 from beta on
  per particle, with the draws of DESIGN.md 2 -- call 0: Box-Muller pairs (z0, z1), (z2, sn0);
  call 1: slip test, slip factor, pair (sn1, sn2); a uniform is (word + 1/2) 2^-32, a pair of
  words (a, b) gives r = sqrt(-2 log u(a)), (r cos 2 pi u(b), r sin 2 pi u(b)):
    delta   = mu + L (z0, z1, z2);   u_slip < slipFactor (strict): delta.y *= u_factor
    (x, y) += Rot(theta) (delta.x, delta.y);   theta += delta.theta
    maxYawDeviation > 0 and fabs(theta - yaw) > maxYawDeviation (strict, not wrapped): w *= 0.7
    zPos   += z_delta;   zSigma = sqrt(zSigma^2 + z_var)
    spread > 0 and no hash: x += sn0 tf, y += sn1 tf, theta += sn2 rf,
                            tf = spreadTranslationFactor spread, rf = spreadRotationFactor spread

The bounds.  Every value is carried as (v, e): v the exact-arithmetic value at 160 bits, e a bound
on |double result - v|.  An input double has e = 0.  One IEEE operation on (a, ea), (b, eb) gives

  a + b : e = ea + eb                 + u (|v| + e)
  a * b : e = |a| eb + |b| ea + ea eb + u (|v| + e)
  a / b : e = (ea + |v| eb) / (|b| - eb) + u (|v| + e)
  sqrt a: e = sqrt(a) - sqrt(a - ea)  + u (|v| + e)

with u = 2^-53 (the last term is the operation's own rounding; 2^-1075 is added below 2^-1022).
The rounding term is dropped when both operands are exact and v is itself a double: then the
operation is exact (a zero covariance makes delta = mu exactly, dyadic matrices factor exactly).
The expressions are evaluated in the association the contract uses, so the count of roundings is
that of each expression.  Further terms, none fitted to an output of the oracle or the kernel:

  sin, cos of theta   4.5e-16 absolute each (the dm_sincos error test_detmath.py asserts)
  a normal            contract mode: 0 (the contract's normal is a double, taken as it is);
                      exact mode: 2^-22 max(1, r) (test_box_muller32_normals), which the carried
                      errors propagate through |L| and tf / rf
  Cholesky            the carried errors of its own operations on the given matrix; a pivot whose
                      sign the carried error cannot decide is refused (the cases avoid it)
  yaw                 the carried error of R10, R00 through atan2 plus 2 u |yaw| for atan2 itself;
                      it matters only for the penalty: the decision is *ambiguous* (either weight
                      accepted) when | |theta - yaw| - maxYawDeviation | is within the carried
                      error of the difference, exact otherwise -- with yaw = 0 and delta.theta = 0
                      the error is 0 and the compare is decided at one ulp
  zsigma              compared with == against sqrt_rn(fl(fl(zs zs) + z_var)), integers only
  weight              compared exactly: w or fl(0.7 w)

Every bound is multiplied by 1 + 2^-40 (the second-order terms are carried, the slack covers the
160-bit arithmetic).

Worst error on the CPU oracle over project_cases.CASES, in units of the bound (printed by
tests/test_project_ref.py::test_worst_case_table):

  field         contract   exact
  x             0.78       0.78
  y             0.72       0.69
  orientation   0.98       0.97
  zpos          0.51       0.51
  zsigma        ==         ==
  weight        ==         ==

(orientation comes close to 1 where theta + delta.theta is one rounding of exact operands: half an
ulp of a value just above a power of two is u |v| itself.  The exact column is not larger: its
bound grows with the 2^-22 term.)
"""
import ctypes as C
import math
from fractions import Fraction

import mpmath as mp

import oracle_ffi as O

PREC = 160
U = mp.mpf(2) ** -53
SLACK = 1 + mp.mpf(2) ** -40
SINCOS_ERR = mp.mpf("4.5e-16")
NORMAL_ERR = mp.mpf(2) ** -22
STREAM_PROJECT = 1
FIELDS = ("x", "y", "orientation", "zpos")


def _ctx():
    mp.mp.prec = PREC


class V:
    """a value and the bound on the double computation's distance from it"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v, self.e = mp.mpf(v), mp.mpf(e)


def is_double(v):
    try:
        return mp.isfinite(v) and mp.mpf(float(v)) == v
    except OverflowError:
        return False


def _rnd(v, e, exact_in):
    if exact_in and e == 0 and is_double(v):
        return V(v, 0)
    r = U * (abs(v) + e)
    if v != 0 and abs(v) < mp.mpf(2) ** -1022:
        r += mp.mpf(2) ** -1075
    return V(v, e + r)


def add(a, b):
    return _rnd(a.v + b.v, a.e + b.e, a.e == 0 and b.e == 0)


def sub(a, b):
    return _rnd(a.v - b.v, a.e + b.e, a.e == 0 and b.e == 0)


def mul(a, b):
    return _rnd(a.v * b.v, abs(a.v) * b.e + abs(b.v) * a.e + a.e * b.e, a.e == 0 and b.e == 0)


def div(a, b):
    v = a.v / b.v
    assert abs(b.v) > b.e
    return _rnd(v, (a.e + abs(v) * b.e) / (abs(b.v) - b.e), a.e == 0 and b.e == 0)


def sqrt(a):
    v = mp.sqrt(a.v)
    lo = a.v - a.e
    e = v - mp.sqrt(lo) if lo > 0 else v
    return _rnd(v, e, a.e == 0)


def lift(x):
    return V(mp.mpf(float(x)), 0)


# ---- the preamble ------------------------------------------------------------------------------
def rotation(q):
    """Eigen's toRotationMatrix of q = (w, x, y, z), entries R[r][c] as V"""
    w, x, y, z = (lift(c) for c in q)
    two = lift(2.0)
    tx, ty, tz = mul(two, x), mul(two, y), mul(two, z)
    twx, twy, twz = mul(tx, w), mul(ty, w), mul(tz, w)
    txx, txy, txz = mul(tx, x), mul(ty, x), mul(tz, x)
    tyy, tyz, tzz = mul(ty, y), mul(tz, y), mul(tz, z)
    one = lift(1.0)
    return [[sub(one, add(tyy, tzz)), sub(txy, twz), add(txz, twy)],
            [add(txy, twz), sub(one, add(txx, tzz)), sub(tyz, twx)],
            [sub(txz, twy), add(tyz, twx), sub(one, add(txx, tyy))]]


def yaw_of(R):
    g = sqrt(add(mul(R[2][2], R[2][2]), mul(R[2][1], R[2][1])))
    assert abs(g.v - mp.mpf("1e-12")) > g.e, "gimbal test undecided"
    if not g.v > mp.mpf("1e-12"):
        return V(0, 0)
    a, b = R[1][0], R[0][0]
    if a.e == 0 and a.v == 0 and b.e == 0 and b.v > 0:
        return V(0, 0)
    v = mp.atan2(a.v, b.v)
    h2 = a.v * a.v + b.v * b.v
    e = (abs(b.v) * a.e + abs(a.v) * b.e) / (h2 - 2 * (abs(a.v) * a.e + abs(b.v) * b.e)) + 2 * U * abs(v)
    return V(v, e)


def cholesky(S):
    """lower factor of the lower triangle of the 9 doubles S; a pivot <= 0 gives a zero column"""
    zero = V(0, 0)
    L = [[zero] * 3 for _ in range(3)]
    for j in range(3):
        d = lift(S[j * 3 + j])
        for k in range(j):
            d = sub(d, mul(L[j][k], L[j][k]))
        assert d.e == 0 or abs(d.v) > d.e, f"pivot {j}: sign undecided ({d.v} +- {d.e})"
        if d.v > 0:
            ljj = sqrt(d)
            L[j][j] = ljj
            for i in range(j + 1, 3):
                s = lift(S[i * 3 + j])
                for k in range(j):
                    s = sub(s, mul(L[i][k], L[j][k]))
                L[i][j] = div(s, ljj)
    return L


def spread_of(max_weight, threshold):
    """weightingFunction(x, 0, beta, 0)"""
    x, beta = lift(max_weight), lift(threshold)
    if x.v < 0:
        return V(1, 0)
    if x.v < beta.v:
        a = div(lift(1.0), sub(lift(0.0), beta))
        s = add(mul(a, x), lift(1.0))
        assert s.v > s.e, "spread's sign undecided"
        return s
    return V(0, 0)


class Prep:
    pass


def preamble(cfg, st, max_weight):
    _ctx()
    p = Prep()
    R = rotation(list(st.body2odometry_rot))
    p.yaw = yaw_of(R)
    t = [lift(c) for c in st.pose_delta_trans]
    p.z_delta = add(add(mul(R[2][0], t[0]), mul(R[2][1], t[1])), mul(R[2][2], t[2]))
    p.z_var = float(Fraction(st.position_error_zz) * 2)
    p.mu = [lift(c) for c in st.sample_mean]
    p.L = cholesky(list(st.sample_cov))
    p.spread = spread_of(max_weight, cfg.spread_threshold)
    p.do_spread = p.spread.v > 0 and not cfg.hash_use
    p.tf = mul(lift(cfg.spread_translation_factor), p.spread)
    p.rf = mul(lift(cfg.spread_rotation_factor), p.spread)
    return p


# ---- the draws ---------------------------------------------------------------------------------
def words(seed, project_count, gi):
    """the 8 raw Philox words of global particle gi: call 0 then call 1"""
    out = []
    for call in (0, 1):
        w = (C.c_uint32 * 4)()
        O.lib().or_dm_philox(int(seed), STREAM_PROJECT, int(project_count), int(gi), call, w)
        out += list(w)
    return out


def uniform(word):
    return (mp.mpf(int(word)) + mp.mpf(0.5)) / 2 ** 32          # exact, and a double


def normal_pair(a, b, mode):
    """(r cos t, r sin t) of the words (a, b) as V"""
    if mode == "contract":
        return lift(O.dm(18, float(a), float(b))), lift(O.dm(19, float(a), float(b)))
    r = mp.sqrt(-2 * mp.log(uniform(a)))
    t = 2 * mp.pi * uniform(b)
    e = NORMAL_ERR * max(mp.mpf(1), r)
    return V(r * mp.cos(t), e), V(r * mp.sin(t), e)


# ---- zsigma, exactly ---------------------------------------------------------------------------
def fl(q):
    """the Fraction q rounded to the nearest double (ties to even), inf on overflow"""
    try:
        return q.numerator / q.denominator
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def sqrt_rn(v):
    """the correctly rounded square root of the double v >= 0, by integers"""
    if v == 0 or v == math.inf:
        return v
    q = Fraction(v)
    t = q.denominator.bit_length() - 1                           # denominator 2^t
    s = (t + 1) // 2 + 64
    N = q.numerator << (2 * s - t)
    r = math.isqrt(N)
    sticky = 0 if r * r == N else 1                              # r has > 64 bits: a sticky bit suffices
    return (2 * r + sticky) / (1 << (s + 1))


def zsigma_expected(zs, z_var):
    """the correctly rounded sqrt of fl(fl(zs zs) + z_var), zs and z_var >= 0"""
    sq = fl(Fraction(zs) * Fraction(zs)) if math.isfinite(zs) else math.inf
    if math.isinf(sq) or math.isinf(z_var):
        return math.inf
    return sqrt_rn(fl(Fraction(sq) + Fraction(z_var)))


# ---- the step ----------------------------------------------------------------------------------
class Result:
    """per checked particle: index, the fields as V, the expected zsigma double, the accepted
    weights (one, or two when the penalty is ambiguous)"""
    __slots__ = ("i", "x", "y", "orientation", "zpos", "zsigma", "zsigma_double", "weights", "penalised", "slipped")


def project(cfg, pa, st, max_weight, project_count, indices, mode="contract", gbase=0):
    p = preamble(cfg, st, max_weight)
    slip, mdev = float(cfg.slip_factor), float(cfg.max_yaw_deviation)
    out = []
    for i in indices:
        w8 = words(cfg.seed, project_count, gbase + i)
        z0, z1 = normal_pair(w8[0], w8[1], mode)
        z2, sn0 = normal_pair(w8[2], w8[3], mode)
        L = p.L
        dx = add(p.mu[0], mul(L[0][0], z0))
        dy = add(p.mu[1], add(mul(L[1][0], z0), mul(L[1][1], z1)))
        dth = add(p.mu[2], add(add(mul(L[2][0], z0), mul(L[2][1], z1)), mul(L[2][2], z2)))
        r = Result()
        r.i = i
        r.slipped = uniform(w8[4]) < mp.mpf(slip)
        if r.slipped:
            dy = mul(dy, V(uniform(w8[5]), 0))
        th0 = mp.mpf(float(pa.orientation[i]))
        s, c = V(mp.sin(th0), SINCOS_ERR), V(mp.cos(th0), SINCOS_ERR)
        x = add(lift(pa.x[i]), sub(mul(c, dx), mul(s, dy)))
        y = add(lift(pa.y[i]), add(mul(s, dx), mul(c, dy)))
        th = add(lift(pa.orientation[i]), dth)
        w = float(pa.weight[i])
        r.weights, r.penalised = (w,), False
        if mdev > 0.0:
            d = sub(th, p.yaw)
            gap = abs(d.v) - mp.mpf(mdev)
            if abs(gap) <= d.e * SLACK and d.e > 0:
                r.weights, r.penalised = (w, 0.7 * w), None
            elif gap > 0:
                r.weights, r.penalised = (0.7 * w,), True
        r.zpos = add(lift(pa.zpos[i]), p.z_delta)
        zs = float(pa.zsigma[i])
        r.zsigma_double = zsigma_expected(zs, p.z_var)
        r.zsigma = None
        if math.isfinite(r.zsigma_double):
            r.zsigma = sqrt(add(mul(lift(zs), lift(zs)), lift(p.z_var)))
        if p.do_spread:
            sn1, sn2 = normal_pair(w8[6], w8[7], mode)
            x = add(x, mul(sn0, p.tf))
            y = add(y, mul(sn1, p.tf))
            th = add(th, mul(sn2, p.rf))
        r.x, r.y, r.orientation = x, y, th
        out.append(r)
    return p, out


def bound(value):
    """the allowed absolute error of one field of a Result"""
    return value.e * SLACK


def check(res, got, label, worst=None):
    """`got` (ParticleArrays after the step) against the Results: the fields within their bounds,
    zsigma and the weight exactly.  worst: dict field -> largest error / bound seen"""
    for r in res:
        i = r.i
        for f in FIELDS:
            want, g = getattr(r, f), float(getattr(got, f)[i])
            assert math.isfinite(g), f"{label}: {f}[{i}] = {g}"
            err, b = abs(mp.mpf(g) - want.v), bound(want)
            if worst is not None and b > 0:
                worst[f] = max(worst.get(f, 0.0), float(err / b))
            assert err <= b, f"{label}: {f}[{i}] = {g!r}, want {mp.nstr(want.v, 25)} +- {mp.nstr(b, 5)} (off by {mp.nstr(err, 5)})"
        zs = float(got.zsigma[i])
        assert zs == r.zsigma_double, f"{label}: zsigma[{i}] = {zs!r}, want exactly {r.zsigma_double!r}"
        if r.zsigma is not None:
            assert abs(mp.mpf(zs) - r.zsigma.v) <= bound(r.zsigma) + mp.mpf(2) ** -1074, f"{label}: zsigma[{i}] off its mpmath value"
        wg = float(got.weight[i])
        assert any(wg == w and math.copysign(1, wg) == math.copysign(1, w) for w in r.weights), \
            f"{label}: weight[{i}] = {wg!r}, want one of {r.weights!r} (penalised: {r.penalised})"
