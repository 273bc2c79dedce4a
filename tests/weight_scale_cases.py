"""The weight-scale cases shared by test_weights_ref.py (CPU oracle) and test_gpu_weight_scales.py
(device): particle sets whose weights are one seeded base set times a power of two or a decimal
scale, weights outside (0, finite), the runs through a filter, and the comparisons with
weights_ref.py (test infrastructure).

The bounds (u = 2^-53, J rows per canonical chunk, every weight positive):

  chunk total  each lane adds J rows from +0.0 (J - 1 roundings), the butterfly adds 6 times:
               J + 5 roundings of non-negative terms, relative error <= (J + 5) u
  fixed point  trunc(total 2^(DM_FX_SCALE - e)), 2^(e-1) <= max w < 2^e: loses < 2^(e-112) per chunk,
               against S >= 2^(e-1) a relative 2^-111 per chunk (at most 65 chunks here); the
               integer sum is exact; one rounding out of fixed point
  S            (J + 6) u
  w_i / S      one more rounding: (J + 7) u
  Q'           sum of (w 2^-e)^2: the scaling is exact, the square rounds once, then the chunk total
               and the rounding out: (J + 7) u  (the largest term is >= 1/4, no square underflows
               below 2^-1022 while the weights span less than 2^480)
  effective    1 / (Q' / (S' S')): S' S' 2 (J + 6) + 1, Q' J + 7, the division and the reciprocal
               one each: (3 J + 22) u
  centroid     a sum of c_i v_i over the normalised weights v_i ((J + 7) u each): the product
               rounds once, the chunk total J + 5 times, the pairwise tree over the chunks
               L = ceil(log2(chunks)) times: |error| <= (2 J + 13 + L) u A, A = sum |c_i| w_i / S.
               sum v_i likewise without the product: (2 J + 12 + L) u.  A coordinate is the quotient
               p = (sum c v) / (sum v), |p| <= A, one more rounding:
               |error| <= ((2 J + 13 + L) + (2 J + 12 + L) + 1) u A = (4 J + 26 + 2 L) u A

Every bound is multiplied by 1 + 2^-40 for the second-order terms (at most (3 J + 22)^2 u^2) and
the fixed-point truncation.  The worst cases measured on the CPU oracle over the whole table are
printed by the tests and recorded in test_weights_ref.py."""
import functools
import math
from fractions import Fraction

import numpy as np

import eslam_abi as A
import synthetic as S
import weights_ref as R

U = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -40
SIZES = (1, 63, 64, 65, 193, 4097)
ROWS = (0, 3, 31)                                  # eslam_config.sum_chunk_rows (0: the default, J = 1 here)
POW2 = (-960, -511, -510, -200, -112, -111, -56, -1, 0, 1, 14, 15, 511, 512, 960)
DECIMAL = (1e-300, 1e-40, 1e-33, 1e-20, 1e-10, 1e10, 1e100, 1e200)
SCALES = [("p", k) for k in POW2] + [("d", s) for s in DECIMAL]
OUTSIDE_SIZES = (65, 193, 4097)
OUTSIDE_ROWS = (0, 3)
STEP_K = (-400, -111, -1, 0, 1, 400)
# indices whose base weight is small (below 2^-20): with them every chunking of the table has a
# chunk of small weights only -- J = 1: [64, 128); J = 3: {192} at n = 193, [2112, 2304) at 4097;
# J = 31: [1984, 3968)
SMALL = sorted(set(range(64, 128)) | {192} | set(range(1984, 3968)))
FIELDS = ("x", "y", "orientation", "zpos", "zsigma", "weight", "mprob", "floating", "n_contact_points")


def rows_of(rows, n):
    return A.chunk_rows(n, rows)


def bound_sum(J):
    return (J + 6) * U * SLACK


def bound_weight(J):
    return (J + 7) * U * SLACK


def bound_effective(J):
    return (3 * J + 22) * U * SLACK


def bound_centroid(J, n):
    chunks = -(-n // (64 * J))
    L = max(chunks - 1, 0).bit_length()            # ceil(log2(chunks))
    return (4 * J + 26 + 2 * L) * U * SLACK


def config(n, rows):
    cfg = A.default_config()
    cfg.seed = 1234
    cfg.particle_count = n
    cfg.min_effective = n // 2
    cfg.sum_chunk_rows = rows
    cfg.flags |= A.FLAG_RECORD_ANCESTORS
    return cfg


def is_normal(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return bool(np.all(np.isfinite(a) & (a >= 2.0 ** -1022)))


@functools.lru_cache(maxsize=None)
def base_weights(n):
    """seeded normal doubles in [2^-30, 1) with full mantissas; the SMALL indices in [2^-30, 2^-20)"""
    rng = np.random.default_rng(1000 + n)
    m = 0.5 + rng.integers(0, 1 << 52, n).astype(np.float64) * 2.0 ** -53          # [0.5, 1), 53 bits
    e = rng.integers(-29, 1, n)
    small = np.array([i for i in SMALL if i < n], dtype=np.int64)
    e[small] = rng.integers(-29, -20, len(small))
    w = np.ldexp(m, e)
    assert np.all((w >= 2.0 ** -30) & (w < 1.0)) and np.all(w[small] < 2.0 ** -20)
    w.setflags(write=False)
    return w


def poses(n, step=False):
    """x, y, theta, z of mixed signs (step=True: on the map, for an update)"""
    rng = np.random.default_rng(2000 + n)
    pa = A.ParticleArrays(n)
    pa.x[:] = rng.normal(0, 0.2 if step else 0.5, n)
    pa.y[:] = rng.normal(0, 0.2 if step else 0.5, n)
    pa.orientation[:] = rng.normal(0, 0.1 if step else 0.3, n)
    pa.zpos[:] = 0.18 + rng.normal(0, 0.01, n) if step else rng.normal(0, 0.2, n)
    pa.zsigma[:] = 0.5 if step else 0.25
    pa.mprob[:] = 1.0
    pa.floating[:] = 1 if step else 0
    return pa


def scaled(n, scale):
    """the base weights times a scale: ("p", k) 2^k (exact), ("d", s) the decimal s (rounded)"""
    kind, v = scale
    w = np.ldexp(base_weights(n), v) if kind == "p" else base_weights(n) * v
    if kind == "p":                                # the table's promise: nothing leaves the normal doubles
        assert is_normal(w) and np.array_equal(np.ldexp(w, -v), base_weights(n))
    return w


def particles(n, weights, step=False):
    pa = poses(n, step)
    pa.weight[:] = weights
    return pa


def scale_id(scale):
    return f"2^{scale[1]}" if scale[0] == "p" else f"{scale[1]:g}"


# ---- the Fraction reference of a case, computed once -------------------------------------------
def _split(fr):
    """(hi, lo) doubles of exact values: hi = the nearest double, lo = the rest"""
    hi = np.array([float(f) for f in fr])
    lo = np.array([float(f - Fraction(h)) for f, h in zip(fr, hi)])
    return hi, lo


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def reference(n, scale):
    """weights_ref over the case's doubles.  A power-of-two scale is exact on normal doubles, so its
    reference is the k = 0 one with S times 2^k."""
    if scale[0] == "p" and scale[1] != 0:
        r0, r = reference(n, ("p", 0)), Ref()
        r.__dict__.update(r0.__dict__)
        r.S = r0.S * Fraction(2) ** scale[1]
        assert is_normal([float(r.S)])
        return r
    w = scaled(n, scale)
    pa = poses(n)
    r = Ref()
    r.S, v, r.effective, r.uniform = R.normalize(w.tolist())
    r.w_hi, r.w_lo = _split(v)
    r.position, r.yaw, _, mags = R.centroid(pa.x.tolist(), pa.y.tolist(), pa.orientation.tolist(), pa.zpos.tolist(),
                                            w.tolist())
    r.mag = [mags[0], mags[1], mags[3]]
    r.mag_yaw = mags[2]
    r.best = R.best_index(w.tolist())
    return r


# ---- one run through a filter --------------------------------------------------------------------
def snapshot(pa):
    return {f: np.array(getattr(pa, f)) for f in FIELDS}


def run_case(f, info_fn, n, weights, full=True):
    """upload; sum, best, normalise (weights, effective, uniform reset); full: resample (ancestors,
    particles), upload again, centroid (which normalises first).  The cases outside the domain
    stop after normalise: what a resample or a centroid of NaN weights gives is declared nowhere."""
    out = {}
    if not hasattr(f, "rng0"):                     # every run of one filter draws the same stream
        f.rng0 = f.rng_state()
    f.set_rng_state(f.rng0)
    f.upload(particles(n, weights))
    out["sum"] = f.weights_sum()
    out["best"] = int(f.best_index())
    out["effective"] = f.normalize()
    out["uniform"] = int(info_fn(f).uniform_reset)
    out["weights"] = np.array(f.download().weight)
    if not full:
        return out
    f.resample()
    out["ancestors"] = np.array(f.ancestors())
    out["resampled"] = snapshot(f.download())
    f.upload(particles(n, weights))
    pos, quat = f.centroid()
    out["position"], out["quat"] = np.array(pos), np.array(quat)
    out["centroid_weights"] = np.array(f.download().weight)
    return out


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b, nan_equal=False):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    eq = bits(a) == bits(b)
    if nan_equal:
        eq |= np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(eq))


def assert_same_run(got, want, label, k=0, nan_equal=False):
    """two runs equal bit for bit; k: got's weights are want's times 2^k (only the sum moves)"""
    assert same_bits(got["sum"], math.ldexp(want["sum"], k), nan_equal), \
        f"{label}: sum {got['sum']!r}, expected {math.ldexp(want['sum'], k)!r}"
    assert same_bits(got["effective"], want["effective"], nan_equal), \
        f"{label}: effective {got['effective']!r} != {want['effective']!r}"
    assert got["uniform"] == want["uniform"], f"{label}: uniform reset {got['uniform']} != {want['uniform']}"
    assert got["best"] == want["best"], f"{label}: best index {got['best']} != {want['best']}"
    for key in ("weights", "position", "quat", "centroid_weights"):
        if key not in want:
            continue
        bad = np.nonzero(~((bits(got[key]) == bits(want[key])) | (nan_equal & np.isnan(got[key]) & np.isnan(want[key]))))[0]
        assert bad.size == 0, (f"{label}: {key} differs at {bad.size} entries; first {bad[0]}: "
                               f"{got[key][bad[0]]!r} != {want[key][bad[0]]!r}")
    if "ancestors" not in want:
        return
    assert np.array_equal(got["ancestors"], want["ancestors"]), f"{label}: ancestors differ"
    for fld in FIELDS:
        g, w = got["resampled"][fld], want["resampled"][fld]
        ok = same_bits(g, w, nan_equal) if g.dtype == np.float64 else np.array_equal(g, w)
        assert ok, f"{label}: resampled {fld} differs"


def rel_err(got, exact):
    return abs(float((Fraction(float(got)) - exact) / exact))


def check_accuracy(got, ref, n, J, label, worst=None):
    """one run of positive weights against the Fraction reference, within the derived bounds;
    worst: a dict that keeps the largest error per quantity in units of u"""
    assert math.isfinite(got["sum"]) and math.isfinite(got["effective"]), \
        f"{label}: sum {got['sum']!r} effective {got['effective']!r}"
    e = {"sum": rel_err(got["sum"], ref.S), "effective": rel_err(got["effective"], ref.effective)}
    for key in ("weights", "centroid_weights"):
        w = got[key]
        e[key] = float(np.max(np.abs(((w - ref.w_hi) - ref.w_lo) / ref.w_hi)))
    cen = []
    for q in range(3):
        cen.append(abs(float((Fraction(float(got["position"][q])) - ref.position[q]) / ref.mag[q])))
    # the quaternion is q_from_yaw(mean yaw) (identity z compensation): yaw = 2 atan2(z, w); each
    # component within an ulp of a value <= 1 (<= u), atan2 within an ulp and sensitivity <= 1 in
    # either component: 3 u on the half angle, 6 u on the yaw, rounded up to 8 u absolute
    qw, qx, qy, qz = got["quat"]
    assert qx == 0.0 and qy == 0.0, f"{label}: quaternion {got['quat']}"
    yaw = 2.0 * math.atan2(qz, qw)
    e_yaw = abs(float(Fraction(yaw) - ref.yaw))
    e["centroid"] = max(cen)
    if worst is not None:
        for key, v in e.items():
            worst[key] = max(worst.get(key, 0.0), v / U)
        worst["yaw"] = max(worst.get("yaw", 0.0), max(e_yaw - 8 * U, 0.0) / float(ref.mag_yaw) / U)
    assert got["uniform"] == int(ref.uniform) and got["best"] == ref.best, label
    assert e["sum"] <= bound_sum(J), f"{label}: sum off by {e['sum'] / U:.2f} u, bound {J + 6} u"
    assert e["weights"] <= bound_weight(J), f"{label}: a weight off by {e['weights'] / U:.2f} u, bound {J + 7} u"
    assert e["centroid_weights"] <= bound_weight(J), f"{label}: a weight (getCentroid) off by {e['centroid_weights'] / U:.2f} u"
    assert e["effective"] <= bound_effective(J), \
        f"{label}: effective {got['effective']!r} off by {e['effective'] / U:.2f} u, bound {3 * J + 22} u"
    bc = bound_centroid(J, n)
    assert e["centroid"] <= bc, f"{label}: position off by {e['centroid'] / U:.2f} u A, bound {bc / U:.1f} u A"
    assert e_yaw <= bc * float(ref.mag_yaw) + 8 * U, f"{label}: yaw off by {e_yaw / U:.2f} u"


# ---- weights outside (0, finite) -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dyadic_weights(n):
    """multiples of 2^-20 in (0, 1): every sum of them is exact in a double"""
    w = np.random.default_rng(3000 + n).integers(1, 1 << 20, n).astype(np.float64) * 2.0 ** -20
    w.setflags(write=False)
    return w


def outside_cases(n, rows):
    """(name, weights): the cases of the declared rule at n particles, J = rows_of(rows, n)"""
    J = rows_of(rows, n)
    chunk, base = 64 * J, dyadic_weights(n)
    chunks = -(-n // chunk)
    out = []
    for at in sorted({0, 63, 64, n - 1}):
        if at < n:
            w = base.copy()
            w[at] = np.nan
            out.append((f"nan_at_{at}", w))
    for name, v in (("pos_inf", np.inf), ("neg_inf", -np.inf)):
        w = base.copy()
        w[n // 2] = v
        out.append((name, w))
    if chunks >= 2:
        for name, a, b in (("nan_then_inf", np.nan, np.inf), ("inf_then_nan", np.inf, np.nan)):
            w = base.copy()
            w[1], w[chunk + 0] = a, b              # chunks 0 and 1
            out.append((name, w))
        w = base.copy()
        w[chunk:2 * chunk] *= -1.0                 # chunk 1 has a negative total, the others count
        out.append(("negative_chunk", w))
    w = np.ones(n)
    w[n // 3] = 1e200
    out.append(("1e200_among_ones", w))
    out.append(("all_negative", -base))
    out.append(("all_neg_zero", np.full(n, -0.0)))
    out.append(("all_pos_zero", np.zeros(n)))
    return out


def check_rule(got, rule, n, J, label):
    """one run against weights_ref.declared_rule: sum and effective as bit patterns (NaN as "is
    NaN"; an effective count the rule gives as a plain quotient, within bound_effective), every
    weight after normalize() (the cases' finite weights are dyadic or 1 and 1e200, so S is exact
    and w / S rounds once: bit patterns), the uniform-reset flag"""
    def one(g, want, what, bound=None):
        if want is R.NAN or (isinstance(want, float) and want != want):
            assert g != g, f"{label}: {what} {g!r}, the rule says NaN"
        elif want is R.INF:
            assert g == math.inf, f"{label}: {what} {g!r}, the rule says +inf"
        elif isinstance(want, float) or bound is None:
            assert same_bits(g, float(want)), f"{label}: {what} {g!r}, the rule says {float(want)!r}"
        else:
            assert math.isfinite(g) and rel_err(g, want) <= bound, f"{label}: {what} {g!r}, the rule says {float(want)!r}"
    one(got["sum"], rule["S"], "sum")
    assert got["uniform"] == int(rule["uniform_reset"]), f"{label}: uniform reset {got['uniform']}"
    one(got["effective"], rule["effective"], "effective", None if rule["uniform_reset"] else bound_effective(J))
    for i, (g, want) in enumerate(zip(got["weights"].tolist(), rule["weights"])):
        one(g, want, f"weight {i}")


# ---- upload, then forced-update steps ----------------------------------------------------------------
STEP_SIZES = ((193, 3), (4097, 0))


def step_config(n, rows):
    cfg = config(n, rows)
    cfg.measurement_threshold_distance = -1.0                      # every step updates
    cfg.measurement_threshold_angle = -1.0
    return cfg


def run_steps(f, info_fn, n, k):
    """upload base weights 2^k, three forced-update steps; everything after each step"""
    f.set_map(S.rough_map(cells=200))
    f.upload(particles(n, scaled(n, ("p", k)), step=True))
    out = []
    for st in S.step_stream(3, tilt=True):
        assert f.step(st)
        i = info_fn(f)
        out.append((snapshot(f.download()), i.effective, int(i.resampled), int(i.uniform_reset), i.weight_sum))
    return out


def assert_same_steps(got, want, label, k=0):
    for s, (g, w) in enumerate(zip(got, want)):
        for fld in FIELDS:
            ok = same_bits(g[0][fld], w[0][fld]) if g[0][fld].dtype == np.float64 else np.array_equal(g[0][fld], w[0][fld])
            assert ok, f"{label} step {s}: {fld} differs"
        assert same_bits(g[1], w[1]) and g[2:4] == w[2:4], f"{label} step {s}: effective {g[1]!r} {w[1]!r}, flags {g[2:4]} {w[2:4]}"
        assert same_bits(g[4], math.ldexp(w[4], k if s == 0 else 0)), f"{label} step {s}: weight sum {g[4]!r} {w[4]!r}"


# ---- a written sub-range ----------------------------------------------------------------------------
def check_normalized(w_in, total, effective, w_out, J, label):
    """a sum, an effective count and normalised weights of the positive weights w_in against
    weights_ref, within the bounds above"""
    S, v, eff, uniform = R.normalize([float(a) for a in w_in])
    hi, lo = _split(v)
    assert not uniform
    assert rel_err(total, S) <= bound_sum(J), f"{label}: sum {total!r}"
    assert rel_err(effective, eff) <= bound_effective(J), f"{label}: effective {effective!r}, exact {float(eff)!r}"
    e = float(np.max(np.abs(((np.asarray(w_out) - hi) - lo) / hi)))
    assert e <= bound_weight(J), f"{label}: a weight off by {e / U:.2f} u"
