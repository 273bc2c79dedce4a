"""The CPU restatement of the pose distribution's Gaussian mixture (tests/c/gmm_ref.c, the rule of
DESIGN.md 5g) against an independent numpy float64 EM, closed forms and planted mixtures.  The
device is compared with the restatement bit for bit in tests/test_gpu_gmm.py."""
import numpy as np
import pytest

import gmm_cases as G
import gmm_ref as R

# Largest disagreement of the restatement and the numpy EM after 10 passes on EM_CASES, in the
# units of `disagreement` below, measured with this file (printed by the test): 1.3e-15.  The two
# differ by the ulps of their exp and log and by the order of their sums, carried through at most
# 10 contracting iterations; 16 x the measured value leaves room for another libm, and the bound
# is never below 1e-12.
MEASURED = 1.3e-15
BOUND = max(16.0 * MEASURED, 1e-12)

EM_CASES = {
    "three along x": dict(centres=[(-6.0, 0.5), (0.0, 0.0), (7.0, -0.5)], K=3),
    "two along y": dict(centres=[(100.0, -3.0), (100.5, 4.0)], K=2),
    "triangle": dict(centres=[(0.0, 0.0), (6.0, 0.0), (3.0, 5.0)], K=3),
    "five on one blob": dict(centres=[(2.0, 3.0)], K=5),
}


def disagreement(got, want, x, y):
    """largest difference relative to each quantity's scale: weights to 1, means to the cloud's
    extent, covariances to its square, the log-likelihood to max(1, |L|)"""
    gw, gm, gc, gl = got
    ww, wm, wc, wl = want
    ext = max(np.ptp(x), np.ptp(y), 1.0)
    return max(np.abs(gw - ww).max(), np.abs(gm - wm).max() / ext, np.abs(gc - wc).max() / ext ** 2,
               abs(gl - wl) / max(1.0, abs(wl)))


@pytest.mark.parametrize("name", list(EM_CASES))
def test_restatement_equals_numpy_em(name):
    case = EM_CASES[name]
    x, y, w = G.clusters(case["centres"], 400, 1.5, seed=11)   # overlapping: no pass repeats L exactly
    rc, gw, gm, gc, info = R.fit(x, y, w, case["K"], 10, 0.0, 1e-6)
    assert rc == 0 and info.iterations == 10 and info.particles_used == x.shape[0]
    want = G.numpy_em(x, y, w, case["K"], 10, 1e-6)
    d = disagreement((gw, gm, gc, info.log_likelihood), want, x, y)
    print(f"gmm restatement vs numpy EM, {name}: {d:.3e} (bound {BOUND:.3e})")
    assert d <= BOUND, (name, d)


def test_one_component_is_the_weighted_mean_and_covariance():
    rng = np.random.default_rng(5)
    n = 700
    x = 1000.0 + 2.0 * rng.standard_normal(n)
    y = -998.0 + 0.7 * rng.standard_normal(n)
    w = rng.uniform(0.2, 1.0, n) * 3e-7
    lx, ly, lw = (a.astype(np.longdouble) for a in (x, y, w))
    sw = lw.sum()
    mx, my = (lw * lx).sum() / sw, (lw * ly).sum() / sw
    cov = [(lw * (lx - mx) ** 2).sum() / sw, (lw * (lx - mx) * (ly - my)).sum() / sw, (lw * (ly - my) ** 2).sum() / sw]
    big = max(np.abs(x).max(), np.abs(y).max())
    first = None
    for iters in (0, 1, 10):
        rc, gw, gm, gc, info = R.fit(x, y, w, 1, iters, 0.0, 1e-6)
        assert rc == 0 and gw[0] == 1.0 and info.components_live == 1
        assert abs(gm[0, 0] - float(mx)) <= n * 2.0 ** -53 * big and abs(gm[0, 1] - float(my)) <= n * 2.0 ** -53 * big
        assert np.abs(gc[0] - np.array(cov, dtype=np.float64)).max() <= n * 2.0 ** -53 * big ** 2
        # every later pass reproduces the bits of the hard assignment's parameters
        bits = np.concatenate([gw, gm.ravel(), gc.ravel()]).view(np.uint64)
        first = bits if first is None else first
        assert np.array_equal(bits, first), iters
    assert np.isnan(R.fit(x, y, w, 1, 0, 0.0, 1e-6)[4].log_likelihood)


@pytest.mark.parametrize("centres", [[(3.0, -2.0), (8.0, 1.0)], [(0.0, 0.0), (6.0, 0.0), (3.0, 5.0)]],
                         ids=["two", "three"])
def test_planted_mixtures_are_recovered(centres):
    x, y, w = G.clusters(centres, 320, 0.3, seed=23)          # centres >= 16 sigma apart
    rc, gw, gm, gc, info = R.fit(x, y, w, len(centres))       # the default parameters
    assert rc == 0 and info.converged == 1 and info.iterations <= 10 and info.components_live == len(centres)
    for c in centres:
        assert np.abs(gm - np.array(c)).max(axis=1).min() <= 0.1, (c, gm)
    assert abs(gw.sum() - 1.0) <= 1e-12


def test_weight_scaling_changes_no_output_bit():
    x, y, w = G.clusters([(0.0, 0.0), (6.0, 0.0), (3.0, 5.0)], 300, 0.3, seed=3)
    base = R.fit(x, y, w, 3)
    for k in (-900, 900):
        got = R.fit(x, y, np.ldexp(w, k), 3)
        for a, b in zip(base[1:4], got[1:4]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), k
        ti, tb = list(R.info_tuple(got[4])), list(R.info_tuple(base[4]))
        assert ti[-1] == tb[-1] + k and ti[:-1] == tb[:-1], k


def test_identical_particles():
    n = 200
    rc, gw, gm, gc, info = R.fit(np.full(n, 12.5), np.full(n, -3.25), np.full(n, 0.01), 3)
    assert rc == 0 and info.components_live == 1 and info.converged == 1 and info.iterations == 2
    assert gw.tolist() == [1.0, 0.0, 0.0] and gm[0].tolist() == [12.5, -3.25] and not gc.any() and not gm[1:].any()


def test_more_components_than_modes():
    x, y, w = G.clusters([(2.0, 3.0)], 500, 0.4, seed=9)
    rc, gw, gm, gc, info = R.fit(x, y, w, 5)
    assert rc == 0 and abs(gw.sum() - 1.0) <= 1e-12
    assert np.isfinite(gw).all() and np.isfinite(gm).all() and np.isfinite(gc).all() and np.isfinite(info.log_likelihood)


def test_skipped_particles_are_counted_and_change_nothing():
    x, y, w = G.cloud(500, seed=4)
    base = R.fit(x, y, w, 3, sum_chunk_rows=1)
    # skipped particles behind the fitted ones leave every fitted particle in its lane: same bits
    bad = np.array([np.nan, 1.0, 2.0, 3.0, np.inf])
    got = R.fit(np.concatenate([x, bad]), np.concatenate([y, np.full(5, 1.0)]),
                np.concatenate([w, [1e-7, 0.0, -1e-7, np.inf, 1e-7]]), 3, sum_chunk_rows=1)
    assert got[4].particles_skipped == 5 and got[4].particles_used == 500
    for a, b in zip(base[1:4], got[1:4]):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert R.info_tuple(got[4])[6:] == R.info_tuple(base[4])[6:] and R.info_tuple(got[4])[:4] == R.info_tuple(base[4])[:4]
    # spread through the cloud they move the others to other lanes: the same fit up to rounding
    xs, ys, ws, cnt = G.with_skipped(x, y, w, seed=8)
    ok = np.isfinite(xs) & np.isfinite(ys) & np.isfinite(ws) & (ws > 0)
    assert cnt == (~ok).sum()
    a = R.fit(xs, ys, ws, 3)
    b = R.fit(xs[ok], ys[ok], ws[ok], 3)
    assert a[4].particles_skipped == cnt and a[4].particles_used == ok.sum() and b[4].particles_skipped == 0
    assert disagreement((a[1], a[2], a[3], a[4].log_likelihood), (b[1], b[2], b[3], b[4].log_likelihood), x, y) <= 1e-9
    assert a[4].iterations == b[4].iterations


def test_no_valid_particle():
    n = 70
    rc, gw, gm, gc, info = R.fit(np.arange(n, dtype=np.float64), np.zeros(n), np.zeros(n), 3)
    assert rc == 0 and info.components_live == 0 and info.particles_used == 0 and info.particles_skipped == n
    assert not gw.any() and not gm.any() and not gc.any() and info.iterations == 0


def test_negative_zero_is_zero():
    x, y, w = G.cloud(130, seed=6)
    x[:40], y[5:70] = 0.0, 0.0
    a = R.fit(x, y, w, 2, sum_chunk_rows=1)
    x[:40:2], y[5:70:3] = -0.0, -0.0
    b = R.fit(x, y, w, 2, sum_chunk_rows=1)
    for u, v in zip(a[1:4], b[1:4]):
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
    assert R.info_tuple(a[4]) == R.info_tuple(b[4])


def test_ctypes_mirrors_have_the_header_layouts(tmp_path):
    import ctypes as C
    import os
    import subprocess
    import eslam_abi as A
    structs = {"eslam_gmm_params": A.GmmParams, "eslam_gmm_component": A.GmmComponent, "eslam_gmm_info": A.GmmInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eslam_gpu.h"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("max %d\\n", ESLAM_GMM_MAX_COMPONENTS);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{os.path.join(R.ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l)
    for cname, py in structs.items():
        assert int(out[cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, f"{cname}.{f}"
    assert int(out["max"]) == A.GMM_MAX_COMPONENTS == 8


def test_arguments():
    x, y, w = G.cloud(10, seed=1)
    for kw in (dict(components=0), dict(components=9), dict(tolerance=-1.0), dict(tolerance=float("nan")),
               dict(min_variance=0.0), dict(min_variance=float("inf")), dict(min_variance=float("nan"))):
        assert R.fit(x, y, w, **kw)[0] == -1, kw
