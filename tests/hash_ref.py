"""An independent restatement of the SurfaceHash respawn and of getBestParticleIndex, in plain
Python and numpy (test infrastructure, no GPU, no oracle).

It restates what the reference does (src/PoseEstimator.cpp:75-86 and 130-182,
src/SurfaceHash.hpp:25-29, 60-92 and 128-153, src/ContactModel.cpp:48-79,
src/ParticleFilter.hpp:160-173) together with the build's own rules where the reference leaves
the result open: replace_count is clamped to N, nothing is drawn when
nothing can be replaced, and a NaN weight sorts after +inf.  The inputs are the hash poses and
each pose's bucket (hash creation has its own numpy reference, test_hash.py::numpy_hash).

The plane through the lowest points is solved exactly (fractions.Fraction on the normal
equations); callers assert that the slopes sit away from a bin edge (HashRef.select_bucket
returns the margin), so an exact solve and the LDL^T of the build cannot choose different bins.
The sum of the weights is math.fsum, the correctly rounded exact sum.  The build's sum contract
 equals it bit for bit where every weight is a multiple of one power of two, the
whole sum fits 53 bits and no 64-particle chunk has a negative total (the contract's fixed-point
accumulators hold totals >= 0): the test families are built that way, or bound the difference."""
import math
from collections import deque
from fractions import Fraction

import numpy as np


class GlibcRand:
    """glibc's rand() after srand(seed): the TYPE_3 additive feedback generator.  r_0 = seed,
    r_i = 16807 r_{i-1} mod (2^31 - 1) for i < 31, r_i = r_{i-31} for i < 34, then
    r_i = r_{i-31} + r_{i-3} mod 2^32; the first 310 of those are discarded and every later one
    gives r_i >> 1.  One object is one stream (no process-global state)."""

    def __init__(self, seed=1):
        r = [seed if seed else 1]
        for i in range(1, 31):
            r.append(16807 * r[i - 1] % 2147483647)
        for i in range(31, 34):
            r.append(r[i - 31])
        for i in range(34, 344):
            r.append((r[i - 31] + r[i - 3]) & 0xFFFFFFFF)
        self.last = deque(r[-34:], maxlen=34)          # the last 34 raw values, oldest first
        self.draws = 0

    def __call__(self):
        v = (self.last[-31] + self.last[-3]) & 0xFFFFFFFF
        self.last.append(v)
        self.draws += 1
        return v >> 1

    def ring(self):
        """(slots, pos): the last 34 raw values laid out as a ring whose slot `pos` holds the
        oldest (the layout of eslam_rng_state::libc_rand / libc_rand_pos)."""
        pos = self.draws % 34
        slots = [0] * 34
        for j, v in enumerate(self.last):
            slots[(pos + j) % 34] = v
        return slots, pos


def lowest_points(feet, groups):
    """ContactModel::lowestPointHeuristic: a run of consecutive contacts with one group id >= 0
    gives its lowest point (the first of equally low ones); an ungrouped contact is its own."""
    out, i, m = [], 0, len(feet)
    while i < m:
        if groups[i] < 0:
            out.append(feet[i])
            i += 1
            continue
        j = i
        while j + 1 < m and groups[j + 1] == groups[i]:
            j += 1
        out.append(feet[min(range(i, j + 1), key=lambda q: (feet[q][2], q))])
        i = j + 1
    return out


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def plane_slopes(points):
    """SurfaceParam::fromPoints: the least-squares plane z = a x + b y + c through the points,
    (a, b) as exact fractions (Cramer's rule on the normal equations)."""
    P = [[Fraction(float(v)) for v in p] for p in points]
    s = lambda f: sum((f(p) for p in P), Fraction(0))
    x, y, z = s(lambda p: p[0]), s(lambda p: p[1]), s(lambda p: p[2])
    xx, yy, xy = s(lambda p: p[0] * p[0]), s(lambda p: p[1] * p[1]), s(lambda p: p[0] * p[1])
    xz, yz = s(lambda p: p[0] * p[2]), s(lambda p: p[1] * p[2])
    A = [[xx, xy, x], [xy, yy, y], [x, y, Fraction(len(P))]]
    b = [xz, yz, z]
    det = _det3(A)
    assert det != 0, "degenerate foot layout"
    col = lambda k: [[b[r] if c == k else A[r][c] for c in range(3)] for r in range(3)]
    return _det3(col(0)) / det, _det3(col(1)) / det


def bin_position(slope, bins):
    """the real number whose integer part Buckets::bucketIndex takes, for the range [-1, 1]"""
    return (slope + 1) / 2 * bins


def bucket_index(slope, bins):
    """Buckets::bucketIndex: truncation towards zero, clamped to [0, bins - 1]"""
    return min(bins - 1, max(0, math.trunc(bin_position(slope, bins))))


def sort_key(w):
    """the respawn order's key of a weight: its float, the zero's sign dropped; NaN after +inf"""
    if w != w:
        return (1, 0.0)
    with np.errstate(over="ignore"):
        return (0, float(np.float32(w)) + 0.0)


def respawn_order(weights):
    return sorted(range(len(weights)), key=lambda i: (sort_key(float(weights[i])), i))


class Respawn:
    """what one sampleFromHash does: the particles replaced, in order (`order`), the hash pose
    each takes (`src`), the weight they get, and k / rel / the bucket behind them"""

    def __init__(self, bucket, bsize, rel, k):
        self.bucket, self.bsize, self.rel, self.k = bucket, bsize, rel, k
        self.order, self.src, self.weight = [], [], None


class HashRef:
    def __init__(self, poses, bucket, bins, rand=None):
        """poses: (x, y, theta, z) arrays in creation order; bucket: each pose's bucket"""
        self.x, self.y, self.th, self.z = (np.asarray(a, dtype=np.float64) for a in poses)
        self.bins = bins
        self.n = len(self.x)
        self.members = {}
        for i, b in enumerate(np.asarray(bucket).tolist()):          # creation order within a bucket
            self.members.setdefault(b, []).append(i)
        self.rand = rand if rand is not None else GlibcRand(1)

    def init(self, n):
        """PoseEstimator::init(N, hash): the pose index of every particle"""
        return [self.rand() % self.n for _ in range(n)]

    def select_bucket(self, feet, groups):
        """(bucket, margin): the bucket of the plane through the lowest points of the
        yaw-compensated feet, and the distance of the nearer slope from a bin edge, in bins"""
        sx, sy = plane_slopes(lowest_points([tuple(float(v) for v in f) for f in feet], list(groups)))
        px, py = bin_position(sx, self.bins), bin_position(sy, self.bins)
        margin = min(abs(p - round(p)) for p in (px, py))
        return bucket_index(sx, self.bins) * self.bins + bucket_index(sy, self.bins), float(margin)

    def relevance(self, bucket):
        """(size of the bucket, getRelevance^3): (1 - size / poses)^3, cubed exactly, rounded once"""
        bsize = len(self.members.get(bucket, []))
        return bsize, float(Fraction(1.0 - 1.0 * bsize / self.n) ** 3)

    def replace_count(self, N, bucket, percentage):
        """replace_count: int(N percentage rel), 0 below a relevance of 0.8 or with an empty
        bucket (nothing to sample), clamped to N"""
        bsize, rel = self.relevance(bucket)
        k = int(N * percentage * rel)
        if rel < 0.8 or bsize == 0:
            k = 0
        return min(k, N)

    def respawn(self, weights, bucket, percentage, avg_factor):
        """PoseEstimator::sampleFromHash on the given weights; draws from self.rand"""
        N = len(weights)
        members = self.members.get(bucket, [])
        bsize, rel = self.relevance(bucket)
        k = self.replace_count(N, bucket, percentage)
        if k == 0:                                                     # nothing replaced, nothing drawn
            return Respawn(bucket, bsize, rel, 0)
        out = Respawn(bucket, bsize, rel, k)
        w = [float(v) for v in weights]
        S = math.fsum(w) if all(v == v for v in w) else float("nan")
        out.weight = ((S / N) * avg_factor) * rel
        out.order = respawn_order(w)[:k]
        out.src = [members[self.rand() % bsize] for _ in range(k)]
        return out


def best_index(weights):
    """ParticleFilter::getBestParticleIndex: the first strictly greater weight wins, starting
    from -inf at index 0 (so -0 before +0 wins, and a NaN never does)"""
    index, best = 0, -math.inf
    for i, w in enumerate(weights):
        if w > best:
            index, best = i, w
    return index
