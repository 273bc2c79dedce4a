"""The CPU oracle's SurfaceHash respawn (PoseEstimator::sampleFromHash) and init(N, hash) against
hash_ref.py, an independent restatement in plain Python, at the edges of the respawn order's key
(float(weight), then index): signed zeros, doubles that collapse to one float, round-to-even at a
float boundary, float denormals, overflow to inf, negative weights, a tie across the
replace_count boundary and NaN (the build's rule: after +inf); at replace_count 0, 1 and N; at an
empty bucket and at the flat map's single bucket; and at particle counts around the sort tile of
2048.  test_gpu_hash_edges.py runs the same cases on the device."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import hash_edge_cases as E
import hash_ref as H
import oracle_ffi as O


def oracle_filter(cfg):
    return O.OracleFilter(cfg, O.SUM_CONTRACT)


def test_glibc_rand_restatement():
    """hash_ref's pure-Python rand() == this system's rand() after srand(1), 5000 draws"""
    libc = C.CDLL(ctypes.util.find_library("c"))
    libc.srand(1)
    want = [libc.rand() for _ in range(5000)]
    r = H.GlibcRand(1)
    assert [r() for _ in range(5000)] == want


def test_families_hit_their_edges():
    """the weight families hold what their names say (as floats)"""
    n = E.N3
    f32 = lambda w: w.astype(np.float32)
    with np.errstate(over="ignore"):
        z = E.family("signed_zeros", n)
        assert np.all(z == 0) and np.signbit(z[0]) and not np.signbit(z[1])
        one = E.family("one_float", n)
        assert len(np.unique(one)) == n and np.all(f32(one) == np.float32(1))
        t = E.family("round_tie", n)
        assert np.float32(1 + 2.0 ** -24) == np.float32(1) and np.float32(1 + 3 * 2.0 ** -24) == np.float32(1 + 2.0 ** -22)
        assert {1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24} <= set(t.tolist())
        d = E.family("denormal", n)
        tiny = np.float32(2.0 ** -126)
        assert np.all(f32(d) < tiny) and np.count_nonzero(f32(d) > 0) > 3000 and d.max() < 2.0 ** -127
        assert np.count_nonzero((d > 0) & (f32(d) == 0)) >= 40 and np.any(np.signbit(d) & (d == 0))
        assert np.all(np.floor(d * 2.0 ** 151) == d * 2.0 ** 151)
        o = E.family("overflow", n)
        assert np.count_nonzero(np.isinf(f32(o))) == 6 and np.all(np.isfinite(o)) and len(np.unique(o[np.isinf(f32(o))])) > 1
        g = E.family("negative", n)
        assert np.any(g < 0) and np.any(np.signbit(g) & (g == 0))
        pad = np.r_[g, np.zeros(-n % 64)].reshape(-1, 64)
        assert np.all(pad.sum(axis=1) > 0)
        x = E.family("nan", n)
        assert np.count_nonzero(np.isnan(x) & np.signbit(x)) > 100 and np.count_nonzero(np.isnan(x) & ~np.signbit(x)) > 100
        for fam in E.FAMILIES:
            if fam not in ("nan", "denormal", "overflow"):
                w = E.family(fam, n, 200)
                assert np.all(np.floor(w * 2.0 ** 40) == w * 2.0 ** 40), fam       # multiples of 2^-40


@pytest.mark.parametrize("n", [1, 2049])
def test_init_hash_against_ref(oracle, n):
    cfg = E.edge_config(n, 0.05)
    f = oracle_filter(cfg)
    f.set_map(E.hash_grid(cells=E.CELLS))
    f.hash_create()
    ref = E.make_ref(f)
    E.assert_rand_state(f, ref, "fresh")
    f.init_hash(n)
    E.check_init(f.download(), ref, ref.init(n))
    E.assert_rand_state(f, ref, "init")


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_respawn_against_ref(oracle, case):
    runs, f, cfg = E.run_case(oracle_filter, case)
    E.check_case(case, runs, cfg)


def test_two_respawns_in_a_row(oracle):
    """period 1: the second project respawns again and rand() goes on where the first stopped"""
    case = ("twice", E.N3, "dyadic", 0.05, "slope")
    runs, f, cfg = E.run_case(oracle_filter, case, then=("one_float",))
    assert len(runs) == 2 and all(r.k > 0 for _, _, r, _, _ in runs)
    E.check_case(case, runs, cfg)
    assert runs[0][3].rand.draws == E.N3 + runs[0][2].k + runs[1][2].k
