"""eslam_gpu_fit_pose_gmm on the device (eslam_gmm.hip) against the CPU restatement
(tests/c/gmm_ref.c), bit for bit: every output double and every info field.  Sizes cover the
partial wave, the block boundary of 4 waves and odd chunk counts (the tree's tail); then skipped
particles, weights at 1e-290 and 1e+290, a pending resample gather, the unchanged filter, the
error codes, and a filter sharded over 2 and 3 ranks (tests/gmm_dist_worker.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eslam_abi as A
import gmm_cases as G
import gmm_ref as R
from parity_util import assert_bit_identical

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KS = (1, 2, 3, 5, 8)
ITERS = (0, 1, 10)
# (n, eslam_config.sum_chunk_rows): one row per chunk, two rows, the default rule
SIZES = [(n, 1) for n in (1, 2, 63, 64, 65, 127, 129, 256, 257, 320, 1000)] + [(130, 2), (4096, 0)]


def config(rows):
    cfg = A.default_config()
    cfg.sum_chunk_rows = rows
    return cfg


def particles(x, y, w):
    pa = A.ParticleArrays(x.shape[0])
    pa.x[:], pa.y[:], pa.weight[:] = x, y, w
    pa.orientation[:] = 0.01 * np.arange(x.shape[0])
    pa.zpos[:], pa.zsigma[:] = 0.18, 0.01
    return pa


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_fit(got, want, label):
    """got: GpuFilter.fit_pose_gmm's tuple; want: gmm_ref.fit's (rc first)"""
    assert want[0] == 0, label
    for name, a, b in zip(("weights", "means", "covs"), got[:3], want[1:4]):
        assert np.array_equal(bits(a), bits(b)), (label, name, a, b)
    assert R.info_tuple(got[3]) == R.info_tuple(want[4]), (label, got[3].as_dict(), want[4].as_dict())


def check_all(g, x, y, w, rows, label, ks=KS, iters=ITERS):
    for k in ks:
        for it in iters:
            tol = 0.0 if it == 1 else 1e-5
            got = g.fit_pose_gmm(k, it, tol, 1e-6)
            assert_same_fit(got, R.fit(x, y, w, k, it, tol, 1e-6, sum_chunk_rows=rows), f"{label} K={k} iterations={it}")


@pytest.mark.parametrize("n,rows", SIZES)
def test_fit_equals_restatement(gpu_mod, n, rows):
    x, y, w = G.cloud(n, seed=100 + n)
    g = gpu_mod.GpuFilter(config(rows))
    g.upload(particles(x, y, w))
    check_all(g, x, y, w, rows, f"n={n} rows={rows}")
    g.close()


@pytest.mark.parametrize("n,rows", [(257, 1), (130, 2), (4096, 0)])
def test_skipped_particles(gpu_mod, n, rows):
    x, y, w, cnt = G.with_skipped(*G.cloud(n, seed=7), seed=n)
    g = gpu_mod.GpuFilter(config(rows))
    g.upload(particles(x, y, w))
    check_all(g, x, y, w, rows, f"skipped n={n}", ks=(1, 3, 8))
    info = g.fit_pose_gmm(3)[3]
    assert info.particles_skipped == cnt and info.particles_used == n - cnt
    # no fitted particle at all: 0 live components, zeros
    w[:] = 0.0
    g.upload(particles(x, y, w))
    got = g.fit_pose_gmm(3)
    assert_same_fit(got, R.fit(x, y, w, 3, sum_chunk_rows=rows), "no valid particle")
    assert got[3].components_live == 0 and got[3].particles_skipped == n and not got[0].any() and not got[1].any()
    g.close()


@pytest.mark.parametrize("scale", [1e-290, 1e290])
def test_weight_extremes(gpu_mod, scale):
    n = 320
    x, y, w = G.cloud(n, seed=12)
    w = w / 3e-7 * scale
    g = gpu_mod.GpuFilter(config(1))
    g.upload(particles(x, y, w))
    check_all(g, x, y, w, 1, f"weights at {scale}", ks=(1, 3, 8), iters=(10,))
    # a power of two moves weight_exp and nothing else
    base = g.fit_pose_gmm(3)
    g.upload(particles(x, y, np.ldexp(w, 40 if scale < 1 else -40)))
    moved = g.fit_pose_gmm(3)
    for a, b in zip(base[:3], moved[:3]):
        assert np.array_equal(bits(a), bits(b))
    ta, tb = R.info_tuple(base[3]), R.info_tuple(moved[3])
    assert ta[:-1] == tb[:-1] and tb[-1] - ta[-1] == (40 if scale < 1 else -40)
    g.close()


def test_identical_particles_and_negative_zero(gpu_mod):
    n = 200
    g = gpu_mod.GpuFilter(config(1))
    x, y, w = np.full(n, -0.0), np.full(n, 3.5), np.full(n, 0.25)
    x[::3] = 0.0
    g.upload(particles(x, y, w))
    got = g.fit_pose_gmm(3)
    assert_same_fit(got, R.fit(x, y, w, 3, sum_chunk_rows=1), "identical particles")
    assert got[3].components_live == 1 and got[3].converged == 1 and got[0].tolist() == [1.0, 0.0, 0.0]
    assert bits(got[1][0]).tolist() == bits(np.array([0.0, 3.5])).tolist() and not got[2].any()
    g.close()


def test_after_a_resample_with_its_gather_pending(gpu_mod):
    n = 1000
    x, y, w = G.cloud(n, seed=31)
    w = w ** 3                                        # concentrated: many particles are dropped, others copied
    g = gpu_mod.GpuFilter(config(1))
    g.upload(particles(x, y, w / w.sum()))
    g.resample()                                      # the gather is left to the next reader
    got = g.fit_pose_gmm(3)
    pa = g.download()
    assert not np.array_equal(pa.x, x)
    assert_same_fit(got, R.fit(pa.x, pa.y, pa.weight, 3, sum_chunk_rows=1), "after resample()")
    g.close()


def test_filter_unchanged(gpu_mod):
    """a fit between two steps changes no later step (the twin never fits), and particles, weights
    and RNG state around a fit are bit-identical"""
    import synthetic as S
    n = 2048
    cfg = S.bench_config(A.default_config(), n)
    grid = S.rough_map(cells=120)
    stream = S.step_stream(4, tilt=True)
    a, b = gpu_mod.GpuFilter(cfg), gpu_mod.GpuFilter(cfg)
    for f in (a, b):
        f.set_map(grid)
        f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)
        for st in stream[:3]:
            f.step(st)
    fit = a.fit_pose_gmm(3)                           # with whatever the third step left pending
    assert fit[3].particles_used == n and fit[3].components_live >= 1
    for f in (a, b):
        f.step(stream[3])
    pa, pb = a.download(), b.download()
    assert_bit_identical(pa, pb, "a step after a fit")
    assert bytes(a.rng_state()) == bytes(b.rng_state())
    ia, ib = a.sync(), b.sync()
    assert (ia.effective, ia.weight_sum, ia.resampled) == (ib.effective, ib.weight_sum, ib.resampled)
    r0 = bytes(a.rng_state())
    got = a.fit_pose_gmm(5)
    assert_bit_identical(a.download(), pa, "particles around a fit")
    assert bytes(a.rng_state()) == r0
    assert_same_fit(got, R.fit(pa.x, pa.y, pa.weight, 5, sum_chunk_rows=cfg.sum_chunk_rows), "the fit of the stepped filter")
    a.close()
    b.close()


def test_error_codes_leave_the_filter_usable(gpu_mod):
    """ESLAM_ERR_NOT_INITIALISED and every ESLAM_ERR_INVALID_ARG.  Not covered: a poisoned filter
    returning its fault (check_poisoned, the line every entry point shares); poisoning a context
    means making a device wait give up, which this file does not do."""
    n = 257
    x, y, w = G.cloud(n, seed=2)
    g = gpu_mod.GpuFilter(config(1))
    with pytest.raises(gpu_mod.EslamError) as e:
        g.fit_pose_gmm()
    assert e.value.code == A.ERR_NOT_INITIALISED
    g.upload(particles(x, y, w))
    want = R.fit(x, y, w, 3, sum_chunk_rows=1)
    before = g.download()
    bad = (dict(components=0), dict(components=9), dict(tolerance=-1e-9), dict(tolerance=float("nan")),
           dict(min_variance=0.0), dict(min_variance=-1.0), dict(min_variance=float("inf")), dict(min_variance=float("nan")))
    for kw in bad:
        with pytest.raises(gpu_mod.EslamError) as e:
            g.fit_pose_gmm(**kw)
        assert e.value.code == A.ERR_INVALID_ARG, kw
        assert_same_fit(g.fit_pose_gmm(3), want, f"after {kw}")
    import ctypes as C
    p = A.GmmParams(3, 10, 1e-5, 1e-6)
    out = (A.GmmComponent * 3)()
    assert g.L.eslam_gpu_fit_pose_gmm(g.h, None, out, None) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_fit_pose_gmm(g.h, C.byref(p), None, None) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_fit_pose_gmm(None, C.byref(p), out, None) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_fit_pose_gmm(g.h, C.byref(p), out, None) == 0          # a null info is allowed
    assert np.array_equal(bits([out[k].weight for k in range(3)]), bits(want[1]))
    d = A.GmmParams()
    g.L.eslam_gmm_params_default(C.byref(d))
    assert (d.components, d.max_iterations, d.tolerance, d.min_variance) == (3, 10, 1e-5, 1e-6)
    assert_bit_identical(g.download(), before, "the refused calls")
    g.close()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_fit_equals_one_gpu(gpu_mod, tmp_path, world):
    """gloo ranks sharing the GPU (tests/gmm_dist_worker.py), shards of unequal chunk counts:
    every rank's result is the single context's bit for bit; bad arguments are refused before
    any collective and differing parameters on every rank, nobody hanging"""
    import gmm_dist_worker as W
    n_global = 1050                                   # 17 chunks of 64: 8 + 9, or 5 + 6 + 6
    store = str(tmp_path / "store")
    procs, outs = [], []
    for r in range(world):
        out = str(tmp_path / f"rank{r}.npz")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), ESLAM_DIST_STORE=store, OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "gmm_dist_worker.py"), str(n_global), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        outs.append(out)
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    bad = [f"--- rank {r} (exit {p.returncode}) ---\n{log[-2500:]}" for r, (p, log) in enumerate(zip(procs, logs)) if p.returncode]
    assert not bad, "\n".join(bad)
    parts = [dict(np.load(o)) for o in outs]
    assert len(set(int(p["chunks"][0]) for p in parts)) > 1
    x, y, w = W.global_cloud(n_global)
    one = gpu_mod.GpuFilter(A.default_config())
    one.upload(particles(x, y, w))
    for p in parts:
        assert p["codes"].tolist() == [A.ERR_INVALID_ARG] * (len(W.BAD) + 1)
    for i, (k, iters, tol) in enumerate(W.FITS):
        wts, means, covs, info = one.fit_pose_gmm(k, iters, tol)
        want = np.concatenate([wts, means.ravel(), covs.ravel()])
        want_info = [v & (2 ** 64 - 1) for v in R.info_tuple(info)]
        assert_same_fit((wts, means, covs, info), R.fit(x, y, w, k, iters, tol), f"one GPU, fit {i}")
        for r, p in enumerate(parts):
            assert np.array_equal(bits(p[f"fit{i}"]), bits(want)), (i, r)
            assert p[f"info{i}"].tolist() == want_info, (i, r)
    one.close()
