"""dm_atan2 and dm_wrap_pi of include/eslam_detmath.h (host build, exported by the pose-moment
restatement tests/c/moments_ref.c) against mpmath at 40 digits."""
import math

import mpmath as mp
import numpy as np
import pytest

import moments_ref as R

mp.mp.dps = 40

# the worst cases this file measures (printed by the tests); the header and DESIGN.md 5i quote them
ATAN2_WORST_ULP = 1.0
# half an ulp of a result in [2, 4) -- the last subtraction's rounding; the two before it are exact or
# far below it -- measured 2.0e-16
WRAP_WORST_ABS = 2.3e-16


def ulp_err(got, want):
    want = float(want)
    if want == 0.0:
        return abs(got)
    return abs(got - want) / math.ulp(abs(want))


def atan2_inputs():
    rng = np.random.default_rng(20240)
    n = 4400
    # all four quadrants, |y / x| from 1e-300 to 1e300 (log-uniform), magnitudes over 1e+-3
    ratio = 10.0 ** rng.uniform(-300, 300, n)
    x = 10.0 ** rng.uniform(-3, 3, n)
    y = x * ratio
    big = ~np.isfinite(y) | (y > 1e305)
    y[big], x[big] = x[big], x[big] / ratio[big]
    x, y = x * rng.choice([-1.0, 1.0], n), y * rng.choice([-1.0, 1.0], n)
    # ratios near 1 and the segment boundaries 7/16 and 11/16, either way round
    m = 1200
    t = np.concatenate([rng.uniform(0.0, 1.0, m // 2), 0.4375 + 1e-3 * rng.standard_normal(m // 4), 0.6875 + 1e-3 * rng.standard_normal(m // 4)])
    b = 10.0 ** rng.uniform(-2, 2, m)
    a = t * b
    swap = rng.random(m) < 0.5
    y2, x2 = np.where(swap, b, a) * rng.choice([-1.0, 1.0], m), np.where(swap, a, b) * rng.choice([-1.0, 1.0], m)
    pts = list(zip(y.tolist(), x.tolist())) + list(zip(y2.tolist(), x2.tolist()))
    # the axes, |y| = |x|, arguments at 2^+-900 and the largest and smallest doubles
    v = [1.0, 3.5, 1e-200, 2.0 ** 900, 2.0 ** -900, 1.7976931348623157e308, 5e-324, 2.2250738585072014e-308]
    for p in v:
        for s in (1.0, -1.0):
            pts += [(s * p, 0.0), (s * p, -0.0), (0.0, s * p), (-0.0, s * p), (s * p, p), (s * p, -p)]
    for p in (2.0 ** 900, 2.0 ** -900):
        for q in (2.0 ** 900, 2.0 ** -900, 1.0, 3.0):
            for sy in (1.0, -1.0):
                for sx in (1.0, -1.0):
                    pts += [(sy * p, sx * q), (sy * q * 0.7, sx * p)]
    return pts


def test_atan2_against_mpmath():
    pts = atan2_inputs()
    assert len(pts) >= 4000
    y, x = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    got = R.atan2(y, x)
    worst, at = 0.0, None
    for g, yy, xx in zip(got.tolist(), y.tolist(), x.tolist()):
        # mpmath has no -0: the angle of |y|, then y's sign
        want = mp.atan2(mp.mpf(abs(yy)), mp.mpf(xx)) * int(math.copysign(1.0, yy))
        if abs(want) < mp.mpf(2) ** -1022:            # a result below the normal range: the correctly rounded one
            assert g == float(want), (yy, xx, g)
            continue
        e = ulp_err(g, want)
        if e > worst:
            worst, at = e, (yy, xx)
    print(f"dm_atan2: worst error {worst:.3f} ulp at {at} over {len(pts)} points")
    assert worst <= 2.0                               # the bar of dm_exp and dm_log (tests/test_detmath.py)
    assert worst <= ATAN2_WORST_ULP + 0.005, "the figure the header quotes"
    assert np.all(np.abs(got) <= math.pi)


def test_atan2_signed_zeros_and_axes():
    """as C's atan2: +-0 on the positive x axis, +-pi on the negative one and at (+-0, -0), +-pi/2 on the y axis"""
    def a(y, x):
        return float(R.atan2([y], [x])[0])
    for x in (0.0, 1.0, 1e-300, 1e300):
        assert math.copysign(1.0, a(0.0, x)) == 1.0 and a(0.0, x) == 0.0
        assert math.copysign(1.0, a(-0.0, x)) == -1.0 and a(-0.0, x) == 0.0
    for x in (-0.0, -1.0, -1e-300, -1e300):
        assert a(0.0, x) == math.pi and a(-0.0, x) == -math.pi
    for y in (1.0, 1e-300, 1e300, 5e-324):
        for x in (0.0, -0.0):
            assert a(y, x) == math.pi / 2 and a(-y, x) == -math.pi / 2
    for p in (1.0, 2.0 ** 900, 2.0 ** -900, 5e-324, 1.7976931348623157e308):
        assert a(p, p) == math.pi / 4 and a(-p, p) == -math.pi / 4
        assert a(p, -p) == 3 * math.pi / 4 and a(-p, -p) == -3 * math.pi / 4
    for y, x in ((1.0, 2.0), (-3.0, 0.5), (1e-5, -7.0), (-2.0, -2.5), (0.45, 1.0), (0.7, 1.0)):
        assert a(y, x) == pytest.approx(math.atan2(y, x), rel=4e-16)


def test_wrap_pi_against_mpmath():
    """On the cut itself -- d within 1e-15 of an odd multiple of pi -- rounding may send d to
    either end, a whole turn apart; both ends are the deviation's wrap, so there the comparison is
    taken on the circle and the result must be at +-pi.  Everywhere else it is direct."""
    rng = np.random.default_rng(77)
    d = np.concatenate([rng.uniform(-50.0, 50.0, 6000), np.linspace(-50.0, 50.0, 2001)])
    near = []
    for k in range(-8, 8):
        c = float((2 * k + 1) * mp.pi)
        v = c
        for _ in range(4):
            v = math.nextafter(v, math.inf)
            near.append(v)
        v = c
        for _ in range(4):
            v = math.nextafter(v, -math.inf)
            near.append(v)
        near += [c, c + 1e-9, c - 1e-9, c + 1e-12, c - 1e-12]
    d = np.concatenate([d, np.array(near), [0.0, -0.0, 1e-300, 2 * math.pi, -2 * math.pi]])
    got = R.wrap_pi(d)
    assert np.all(got >= -math.pi - 1e-15) and np.all(got <= math.pi + 1e-15)
    two_pi = 2 * mp.pi
    worst, on_cut = 0.0, 0
    for g, dd in zip(got.tolist(), d.tolist()):
        turns = mp.mpf(dd) / two_pi
        want = mp.mpf(dd) - two_pi * mp.nint(turns)
        err = abs(mp.mpf(g) - want)
        if abs(abs(turns - mp.nint(turns)) - mp.mpf(1) / 2) * two_pi < mp.mpf("1e-15"):
            on_cut += 1
            err = min(err, abs(err - two_pi))
            assert abs(abs(g) - math.pi) <= 2e-15
        worst = max(worst, float(err))
    print(f"dm_wrap_pi: worst |error| {worst:.3e} over {len(d)} points, {on_cut} on the cut")
    assert on_cut >= 8
    assert worst <= WRAP_WORST_ABS
