"""A plain restatement of the weight statistics in exact rational arithmetic (test infrastructure).

No ctypes, none of the build's headers: only the reference's definitions, evaluated with
fractions.Fraction on the doubles as they are given.

  getWeightsSum / normalizeWeights  src/ParticleFilter.hpp:34-70
      S = sum w;  w_i <- w_i / S;  effective = 1 / sum (w_i / S)^2;
      S <= 0: every weight becomes 1 / N (the uniform reset), effective = N
  getBestParticleIndex              src/ParticleFilter.hpp:160-173  (first maximum, strict >)
  getCentroid                       src/PoseEstimator.cpp:354-383
      normalises, then sums x w, y w, theta w, z w and w over the normalised weights;
      position = (sum x w, sum y w, sum z w) / sum w, mean yaw = sum theta w / sum w

`declared_rule` states what the build's sum contract declares for weights outside (0, finite),
where the reference itself has no defined answer ("outside the domain")."""
import math
from fractions import Fraction


def weights_sum(w):
    """S = sum w, exact"""
    return sum((Fraction(float(v)) for v in w), Fraction(0))


def normalize(w, n_global=None):
    """(S, normalised weights, effective, uniform_reset), all exact"""
    n = len(w) if n_global is None else n_global
    S = weights_sum(w)
    if S <= 0:
        return S, [Fraction(1, n)] * len(w), Fraction(n), True
    v = [Fraction(float(a)) / S for a in w]
    return S, v, 1 / sum((a * a for a in v), Fraction(0)), False


def best_index(w):
    """the first maximum (strict >, from -inf: NaN is never the best)"""
    index, weight = 0, -math.inf
    for i, v in enumerate(w):
        if v > weight:
            index, weight = i, v
    return index


def centroid(x, y, theta, z, w):
    """getCentroid: (position [x, y, z], mean yaw, the five sums, the four sums of |.| w), exact;
    w: the weights as given (normalised here)"""
    _, v, _, _ = normalize(w)
    cols = [[Fraction(float(a)) for a in c] for c in (x, y, theta, z)]
    sums = [sum((a * b for a, b in zip(c, v)), Fraction(0)) for c in cols] + [sum(v, Fraction(0))]
    mags = [sum((abs(a) * b for a, b in zip(c, v)), Fraction(0)) for c in cols]
    sw = sums[4]
    return [sums[0] / sw, sums[1] / sw, sums[3] / sw], sums[2] / sw, sums, mags


# ---- the contract's declared rule outside (0, finite) -----------------------------------------
NAN, INF = "nan", "inf"


def _chunk_total(vals):
    """the total of one canonical chunk in IEEE terms: NAN, +-inf (as a float) or the exact sum"""
    if any(v != v for v in vals) or (math.inf in vals and -math.inf in vals):
        return NAN
    for v in vals:
        if math.isinf(v):
            return v
    return sum((Fraction(v) for v in vals), Fraction(0))


def rule_sum(vals, chunk):
    """The declared rule, per canonical chunk of `chunk` = 64 J consecutive particles: a NaN total
    makes the sum NaN; else a +-inf total makes it +inf; a total <= 0 adds 0."""
    totals = [_chunk_total([float(v) for v in vals[c:c + chunk]]) for c in range(0, len(vals), chunk)]
    if any(t is NAN for t in totals):
        return NAN
    if any(not isinstance(t, Fraction) for t in totals):
        return INF
    return sum((t for t in totals if t > 0), Fraction(0))


def _div(a, S):
    """a / S as IEEE division decides it where it is not a plain quotient; S: NAN, INF or a
    positive Fraction.  Returns a float (NaN, +-inf, +-0) or the exact Fraction."""
    if a != a or S is NAN:
        return math.nan
    if S is INF:
        return math.nan if math.isinf(a) else math.copysign(0.0, a)
    if math.isinf(a):
        return a
    if a == 0.0:
        return a                                   # keeps the zero's sign
    return Fraction(a) / S


def declared_rule(w, rows, n_global=None):
    """normalizeWeights under the declared rule, `rows` = J.  Returns a dict: S and Q (the rule
    applied to the weights and to their squares), uniform_reset, effective and the weights after
    the call; each value NAN, INF, a float (a signed zero or infinity) or an exact Fraction."""
    n = len(w) if n_global is None else n_global
    w = [float(v) for v in w]
    chunk = 64 * rows
    S = rule_sum(w, chunk)
    # the squares are never negative and (+-inf)^2 = +inf, so over them the rule is: NaN if any
    # weight is NaN, else +inf if any is infinite, else the exact sum
    if any(v != v for v in w):
        Q = NAN
    elif any(math.isinf(v) for v in w):
        Q = INF
    else:
        Q = sum((Fraction(v) ** 2 for v in w), Fraction(0))
    if isinstance(S, Fraction) and S <= 0:
        return dict(S=S, Q=Q, uniform_reset=True, effective=Fraction(n), weights=[Fraction(1, n)] * len(w))
    if S is NAN or Q is NAN or S is INF:           # inf / (inf inf) as well: NaN
        eff = NAN
    else:
        eff = S * S / Q
    return dict(S=S, Q=Q, uniform_reset=False, effective=eff, weights=[_div(v, S) for v in w])
