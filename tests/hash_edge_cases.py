"""The hash-respawn and best-particle edge cases shared by test_hash_ref.py (CPU oracle) and
test_gpu_hash_edges.py (device): weight families at the edges of the (float weight, index) sort
key, the sizes, percentages and buckets, and the comparison of one filter with hash_ref.py
(test infrastructure)."""
import functools

import numpy as np

import eslam_abi as A
import hash_ref as H
import synthetic as S
from contact_layouts import yaw_free_feet
from hash_util import SLOPE_FEET, hash_config, hash_grid

CELLS, STEPS, BINS = 60, 8, 20
N3 = 2048 * 2 + 17                       # 4113: three sort tiles of 2048, the last ragged
FX_SCALE = 112                           # DM_FX_SCALE (include/eslam_detmath.h)
ZS0 = 0.25                               # the uploaded zSigma


# ---- feet ------------------------------------------------------------------------------------
def _on_plane(a, b, c=-0.2):
    return lambda x, y, up=0.0: (x, y, c + a * x + b * y + up)


_g = _on_plane(-0.13, 0.33)
# six feet in three groups of two with distinct z: the lowest of each group lies on the plane
# z = -0.13 x + 0.33 y - 0.2, its partner 5 to 9 cm above it, first in two groups, second in one
GROUPED_FEET = [_g(0.3, 0.05, 0.07), _g(0.25, 0.0), _g(-0.25, 0.0), _g(-0.3, 0.05, 0.09), _g(0.05, -0.45, 0.05),
                _g(0.0, -0.5)]
GROUPED_IDS = [0, 0, 1, 1, 2, 2]
_e = _on_plane(0.85, 0.04)               # a slope no pose of the map has: an empty bucket
EMPTY_FEET = [_e(0.25, 0.0), _e(-0.25, 0.0), _e(0.25, -0.5), _e(-0.25, -0.5)]
_l = _on_plane(0.03, 0.04)               # nearly level: the flat map's one bucket (10, 10)
LEVEL_FEET = [_l(0.25, 0.0), _l(-0.25, 0.0), _l(0.25, -0.5), _l(-0.25, -0.5)]


def bucket_steps(kind, steps=1):
    """(grid, step inputs) of a bucket kind"""
    if kind == "slope":                  # hash_util's slope feet under the tilted body
        return hash_grid(cells=CELLS), S.step_stream(steps, feet=SLOPE_FEET, tilt=True)
    if kind == "grouped":
        return hash_grid(cells=CELLS), S.step_stream(steps, feet=GROUPED_FEET, groups=GROUPED_IDS)
    if kind == "empty":
        return hash_grid(cells=CELLS), S.step_stream(steps, feet=EMPTY_FEET)
    if kind == "flat":
        return S.flat_map(cells=CELLS), S.step_stream(steps, feet=LEVEL_FEET)
    raise KeyError(kind)


# ---- weight families ---------------------------------------------------------------------------
def _scatter(n, seed):
    return np.random.default_rng(seed).permutation(n)


def family(name, n, k=0):
    """n weights of the family; k: the replace count of the case (the boundary family)"""
    j = np.arange(n, dtype=np.float64)
    if name == "zeros":
        return np.zeros(n)
    if name == "signed_zeros":           # -0, +0, -0, ...
        return np.where(np.arange(n) % 2 == 0, -0.0, 0.0)
    if name == "one_float":              # 1 + j 2^-40 < 1 + 2^-24: every float is 1, the index decides
        return 1.0 + j[_scatter(n, 1)] * 2.0 ** -40
    if name == "round_tie":
        # 1 + 2^-24 lies halfway between the floats 1 and 1 + 2^-23 and goes to the even one, 1;
        # 1 + 3 2^-24 halfway between 1 + 2^-23 and 1 + 2^-22 and goes to 1 + 2^-22; their
        # neighbours 2^-40 to either side go to the nearer float
        u, e = 2.0 ** -24, 2.0 ** -40
        # (so does 1 - 2^-25, the tie between 1 - 2^-24 and 1, which goes to 1).  Five of the
        # eleven values are the float 1, the lowest key: the index decides among them, not the double
        vals = np.array([1 + u, 1 + 3 * u, 1 + u - e, 1 + u + e, 1 + 3 * u - e, 1 + 3 * u + e, 1.0, 1 + 2 * u, 1 + 4 * u,
                         1 - u / 2, 1 - u / 2 + e])
        return vals[_scatter(n, 2) % len(vals)]
    if name == "denormal":
        # float denormals j 2^-140 (exact in float), with values that round to a float zero
        # (2^-151; 2^-150, the tie that goes to the even 0), true zeros of both signs and
        # 3 2^-150 (the tie between 2^-149 and 2^-148, which goes to 2^-148)
        w = (j % 4000) * 2.0 ** -140
        p = _scatter(n, 3)
        for q, v in enumerate((2.0 ** -151, 2.0 ** -150, 0.0, -0.0, 3 * 2.0 ** -150, 2.0 ** -148, 2.0 ** -149)):
            w[p[q::23][:40]] = v
        return w[_scatter(n, 4)]
    if name == "overflow":
        # multiples of 2^100 below FLT_MAX, and six weights at or above 2^128, which are inf as floats
        w = (1.0 + j[_scatter(n, 5)]) * 2.0 ** 100
        big = (2.0 ** 128, 1.5 * 2.0 ** 128, 2.0 ** 129, 2.0 ** 128, 1.25 * 2.0 ** 129, 2.0 ** 129)
        w[_scatter(n, 6)[:len(big)]] = big[:min(len(big), n)]
        return w
    if name == "negative":
        # negative among positive; every run of 64 keeps a positive total (see hash_ref.py)
        w = ((np.arange(n) * 7) % 13 + 1) * 2.0 ** -8
        neg = np.arange(n) % 3 == 1
        w[neg] = -(((np.arange(n) * 5) % 11)[neg].astype(np.float64)) * 2.0 ** -10     # includes -0.0
        return w
    if name == "boundary_tie":
        # k - 3 low weights, then six weights of one float (1) at scattered indices, the rest 2:
        # the k-th and (k + 1)-th keys are equal, the boundary falls inside the tie
        assert 3 <= k <= n - 3
        p = _scatter(n, 7)
        w = np.full(n, 2.0)
        w[p[:k - 3]] = 0.5 - (np.arange(k - 3) % 5) * 2.0 ** -10
        w[p[k - 3:k + 3]] = 1.0 + np.arange(6) * 2.0 ** -40
        return w
    if name == "dyadic":                 # random multiples of 2^-30 below 2^-10, many repeated
        rng = np.random.default_rng(8)
        return rng.integers(0, 1 << 20, n).astype(np.float64)[rng.integers(0, n, n)] * 2.0 ** -30
    if name == "nan":
        # a quarter NaN, of both signs and several payloads, among dyadic weights and +inf
        rng = np.random.default_rng(9)
        w = rng.integers(0, 1 << 20, n).astype(np.float64) * 2.0 ** -30
        p = _scatter(n, 10)
        nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,
                         0x7FF8000000000123], dtype=np.uint64).view(np.float64)
        q = p[:max(n // 4, 1)]
        w[q] = nans[np.arange(len(q)) % len(nans)]
        w[p[len(q):len(q) + 3]] = np.inf
        return w
    raise KeyError(name)


TINY = ()                                # families whose sum the contract truncates (weight_bound): none, see check_respawn
FAMILIES = ("zeros", "signed_zeros", "one_float", "round_tie", "denormal", "overflow", "negative", "boundary_tie",
            "dyadic", "nan")


# (id, n, family, percentage, bucket kind); a percentage ("k", K) is the one that makes
# replace_count K (resolve_percentage).  The NaN family replaces 90 %, so the boundary falls among
# the NaN; the overflow family all but three, so it falls among the six float infinities
CASES = [(f"family-{fam}", N3, fam, {"nan": 0.9, "overflow": ("k", N3 - 3)}.get(fam, 0.05), "slope") for fam in FAMILIES]
CASES += [(f"n-{n}", n, "dyadic", 2.0 if n == 1 else 0.05, "slope") for n in (1, 255, 2048, 2049)]
CASES += [("pct-0.9", N3, "dyadic", 0.9, "slope"), ("pct-2.0", N3, "dyadic", 2.0, "slope"),
          ("pct-k1", N3, "dyadic", ("k", 1), "slope")]
CASES += [("bucket-grouped", N3, "dyadic", 0.05, "grouped"), ("bucket-empty", N3, "dyadic", 0.05, "empty"),
          ("bucket-flat", N3, "dyadic", 0.05, "flat")]
CASE_IDS = [c[0] for c in CASES]


# ---- one case ----------------------------------------------------------------------------------
def edge_config(n, percentage):
    cfg = hash_config(n, steps=STEPS, bins=BINS, period=1, percentage=percentage)
    cfg.max_yaw_deviation = 0.0          # project leaves the weights alone
    return cfg


def particles(weights):
    n = len(weights)
    rng = np.random.default_rng(n)
    pa = A.ParticleArrays(n)
    pa.x[:] = rng.normal(0, 0.2, n)
    pa.y[:] = rng.normal(0, 0.2, n)
    pa.orientation[:] = rng.normal(0, 0.1, n)
    pa.zpos[:] = 0.18
    pa.zsigma[:] = ZS0
    pa.weight[:] = weights
    pa.mprob[:] = 1.0
    pa.floating[:] = 0
    return pa


@functools.lru_cache(maxsize=None)
def hash_tables(kind):
    """the hash poses and buckets of a bucket kind's map (the CPU oracle's SurfaceHash::create,
    which test_hash.py checks against numpy), computed once"""
    import oracle_ffi as O
    f = O.OracleFilter(edge_config(1, 0.05), O.SUM_CONTRACT)
    f.set_map(bucket_steps(kind)[0])
    f.hash_create()
    return tuple(f.hash_poses())


def resolve_percentage(pct, n, rel):
    """("k", K): the percentage at which int(n * pct * rel) is K (the middle of its interval)"""
    if not isinstance(pct, tuple):
        return pct
    p = (pct[1] + 0.5) / n / rel
    assert int(n * p * rel) == pct[1]
    return p


def make_ref(f, draws=0):
    """hash_ref over the filter's hash poses, its rand() advanced by `draws`"""
    x, y, th, z, bucket = f.hash_poses()
    ref = H.HashRef((x, y, th, z), bucket, BINS)
    for _ in range(draws):
        ref.rand()
    return ref


def assert_rand_state(f, ref, label=""):
    """the filter's rand() stands exactly where the reference's does (position and ring)"""
    st = f.rng_state()
    slots, pos = ref.rand.ring()
    assert int(st.libc_rand_pos) == pos, f"{label}: rand() position {st.libc_rand_pos} != {pos}"
    assert [int(v) for v in st.libc_rand] == slots, f"{label}: rand() state differs"


def weight_bound(wexp, avg, rel):
    """see check_respawn: the truncation bound of the tiny-weight family on the assigned weight"""
    return (2.0 ** -(FX_SCALE - wexp)) * avg * rel * (1.0 + 2.0 ** -40)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_respawn(before, after, r, ref, avg, tiny=False, label=""):
    """One project + respawn against hash_ref.  before: the uploaded particles; after: the
    filter's download; r: hash_ref's Respawn for the uploaded weights.

    The weight the replaced particles get is ((S / N) avgFactor) rel.  Where every uploaded
    weight is a multiple of 2^-40 (of 2^100 in the overflow family) the contract's fixed-point sum
    S is exact and the weight equals hash_ref's (math.fsum) bit for bit.  So it does in the
    denormal family (float denormals, multiples of 2^-151 with a sum below 2^-120): the fixed
    point follows the largest weight (dm_stat_exp: e = -127, scale 239), so no chunk total is
    truncated.  While the statistics' exponent was clamped at 1 the contract truncated there and
    the family was compared within a bound (tiny=True, kept for a family that would need it):
    the double sum of each chunk of 64 particles is exact (30 significant bits), and
    each chunk total is converted to fixed point as trunc(total 2^(DM_FX_SCALE - wexp)), losing
    less than 2^-(DM_FX_SCALE - wexp); there are at most N chunks, so
    0 <= fsum - S < N 2^-(DM_FX_SCALE - wexp).  Dividing by N, times avgFactor, times rel (three
    roundings of 2^-53 relative each, far below the bound's slack of 2^-40) gives
    |weight - ref| <= 2^-(DM_FX_SCALE - wexp) avgFactor rel (1 + 2^-40), wexp the exponent of the
    largest weight."""
    n = before.n
    replaced = np.zeros(n, bool)
    replaced[r.order] = True
    assert len(set(r.order)) == r.k == len(r.src)
    got = after.zsigma == 0.5
    assert np.array_equal(got, replaced), (f"{label}: replaced set differs: {np.count_nonzero(got)} particles, "
                                           f"reference {r.k}; first difference at {np.nonzero(got != replaced)[0][:5]}")
    o, s = np.array(r.order, dtype=np.int64), np.array(r.src, dtype=np.int64)
    for fld, pose in (("x", ref.x), ("y", ref.y), ("orientation", ref.th), ("zpos", ref.z)):
        bad = np.nonzero(bits(getattr(after, fld)[o]) != bits(pose[s]))[0]
        assert bad.size == 0, f"{label}: {fld} of replaced particle {o[bad[0]]} is not hash pose {s[bad[0]]}"
    # zSigma and floating: 0.5 and set where replaced; elsewhere project's sqrt(zs^2 + 2 err_zz), untouched
    keep = ~replaced
    assert np.all(after.floating[replaced] == 1) and np.all(after.floating[keep] == 0), label
    zs = np.sqrt(ZS0 * ZS0 + 1e-4 * 2.0)
    assert np.all(bits(after.zsigma[keep]) == bits(np.full(np.count_nonzero(keep), zs))), label
    # every other weight unchanged, bit for bit (project left them alone)
    assert np.array_equal(bits(after.weight[keep]), bits(before.weight[keep])), f"{label}: a kept weight changed"
    if r.k == 0:
        return
    w = after.weight[replaced]
    assert np.all(bits(w) == bits(w[:1])), f"{label}: the replaced particles' weights differ"
    w = float(w[0])
    if r.weight != r.weight:
        assert w != w, f"{label}: weight {w!r}, reference NaN"
    elif tiny:
        bound = weight_bound(1, avg, r.rel)
        print(f"{label}: weight {w!r} reference {r.weight!r} bound {bound!r}")
        assert abs(w - r.weight) <= bound, f"{label}: weight {w!r} reference {r.weight!r} bound {bound!r}"
    else:
        assert bits([w])[0] == bits([r.weight])[0], f"{label}: weight {w!r} reference {r.weight!r}"


def run_case(make_filter, case, then=()):
    """Run one case on a fresh filter: init_pose on the case's map, the upload, one project;
    then one more upload and project per family named in `then`, with the following steps (the
    rand() stream goes on).  Returns [(before, after, respawn, ref, label)], the filter and its
    config, and checks the rand() state after every call."""
    cid, n, fam, pct, kind = case
    fams = (fam,) + tuple(then)
    grid, steps = bucket_steps(kind, len(fams))
    tables = hash_tables(kind)
    ref = H.HashRef(tables[:4], tables[4], BINS)
    if isinstance(pct, tuple):                                    # the relevance of the first step's bucket
        st0 = steps[0]
        b0, _ = ref.select_bucket(yaw_free_feet(st0), [int(st0.contacts[i].group_id) for i in range(int(st0.n_contacts))])
        pct = resolve_percentage(pct, n, ref.relevance(b0)[1])
    cfg = edge_config(n, pct)
    f = make_filter(cfg)
    f.set_map(grid)
    f.init_pose([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])          # SurfaceHash::create + init(N, hash): n draws
    for a, b in zip(f.hash_poses(), tables):                      # the filter's hash is the reference's input
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    for _ in range(n):
        ref.rand()
    assert_rand_state(f, ref, f"{cid} init")
    out = []
    for s, (st, fam_s) in enumerate(zip(steps, fams)):
        groups = [int(st.contacts[i].group_id) for i in range(int(st.n_contacts))]
        bucket, margin = ref.select_bucket(yaw_free_feet(st), groups)
        assert margin > 1e-9, f"{cid}: a slope sits {margin} bins from a bin edge"
        pa = particles(family(fam_s, n, ref.replace_count(n, bucket, pct)))
        f.upload(pa)
        r = ref.respawn(pa.weight, bucket, pct, cfg.hash_avg_factor)
        f.project(st)
        after = f.download()
        assert_rand_state(f, ref, f"{cid} project {s}")
        out.append((pa, after, r, ref, f"{cid} project {s}"))
    return out, f, cfg


def check_init(pa, ref, idx):
    """init(N, hash): particle i holds hash pose idx[i]; zSigma 0, weight 0, floating"""
    i = np.array(idx, dtype=np.int64)
    for fld, pose in (("x", ref.x), ("y", ref.y), ("orientation", ref.th), ("zpos", ref.z)):
        assert np.array_equal(bits(getattr(pa, fld)), bits(pose[i])), fld
    zero = np.zeros(pa.n, np.uint64)
    assert np.array_equal(bits(pa.zsigma), zero) and np.array_equal(bits(pa.weight), zero) and np.all(pa.floating == 1)


def check_case(case, runs, cfg):
    """what the case is there for holds in the reference, then every run against it"""
    cid, n, fam, pct, kind = case
    for step, (before, after, r, ref, label) in enumerate(runs):
        if kind == "empty":
            assert r.bsize == 0 and r.rel == 1.0 and r.k == 0
        elif kind == "flat":
            assert r.bsize == ref.n and r.rel == 0.0 and r.k == 0
        else:
            assert 0 < r.bsize and r.rel >= 0.8 and 0 < r.k <= n
        if pct == 2.0:
            assert r.k == n
        if isinstance(pct, tuple) and step == 0:
            assert r.k == pct[1]
        if cid == "pct-0.9":
            assert n // 2 < r.k < n
        if step == 0 and fam == "boundary_tie":
            order = H.respawn_order(before.weight.tolist())
            a, b = order[r.k - 1], order[r.k]
            assert H.sort_key(float(before.weight[a])) == H.sort_key(float(before.weight[b])) and a < b
        if step == 0 and fam == "overflow":                        # the boundary falls among the float infinities
            with np.errstate(over="ignore"):
                inf = np.isinf(before.weight.astype(np.float32))
            hit = np.zeros(n, bool)
            hit[r.order] = True
            assert np.all(hit[~inf]) and 0 < np.count_nonzero(hit & inf) < np.count_nonzero(inf)
        if step == 0 and fam == "nan":                             # ... among the NaN
            nan = np.isnan(before.weight)
            hit = np.zeros(n, bool)
            hit[r.order] = True
            assert np.all(hit[~nan]) and 0 < np.count_nonzero(hit & nan) < np.count_nonzero(nan)
        check_respawn(before, after, r, ref, cfg.hash_avg_factor, tiny=step == 0 and fam in TINY, label=label)


# ---- best particle -------------------------------------------------------------------------------
BEST_SIZES = (1, 63, 64, 65, 256, 257, 524288 + 257)     # the last: more than 2048 blocks of 256


def best_cases(n):
    """(name, weights) for getBestParticleIndex at n particles"""
    rng = np.random.default_rng(n)
    base = rng.integers(1, 1 << 20, n).astype(np.float64) * 2.0 ** -21          # in (0, 0.5)
    out = []
    for at in sorted({0, n - 1, 63, 64, 255, 256} & set(range(n))):
        w = base.copy()
        w[at] = 0.75
        out.append((f"max_at_{at}", w))
    w = base.copy()                                        # the maximum in the first and in the last block
    w[[min(3, n - 1), n - 1]] = 0.75
    out.append(("max_twice", w))
    stride = 2048 * 256                                    # the grid stride of the 2048-block launch
    if n > stride + 300:                                   # two maxima one thread visits; one it visits second
        for name, at in (("max_twice_one_thread", [100, stride + 100]), ("max_second_pass_first", [stride + 100, 300])):
            w = base.copy()
            w[at] = 0.75
            out.append((name, w))
    neg = -base
    for name, a, b in (("neg_zero_first", -0.0, 0.0), ("pos_zero_first", 0.0, -0.0)):
        w = neg.copy()
        w[0], w[n - 1] = a, b                              # n == 1: the one weight is b
        out.append((name, w))
    out.append(("all_neg_inf", np.full(n, -np.inf)))
    out.append(("all_nan", np.full(n, np.nan)))
    w = base.copy()                                        # NaN before and after the maximum
    w[n // 2] = 0.75
    w[0] = np.nan
    w[n - 1] = -np.nan if n > 2 else w[n - 1]
    if n > 2:
        w[n // 2 - 1] = np.nan
    out.append(("nan_around_max", w))
    w = base.copy()
    w[n // 3] = np.inf
    w[n - 1] = np.inf if n > 1 else w[n - 1]
    out.append(("pos_inf", w))
    w = rng.integers(1, 1 << 20, n).astype(np.float64) * 2.0 ** -1074          # denormal doubles
    w[(2 * n) // 3] = ((1 << 20) + 5) * 2.0 ** -1074
    out.append(("denormal", w))
    return out
