"""eslam_gpu_pose_moments on the device (eslam_moments.hip) against the CPU restatement
(tests/c/moments_ref.c), bit for bit: every double and every count.  Sizes cover the partial wave,
the block boundary of 4 waves and odd chunk counts (the tree's tail), each ungated and gated; then
skipped particles, weights at 1e-290 and 1e+290, a yaw cloud across the cut, a pending resample
gather, the unchanged filter, the error codes, and a filter sharded over 2 and 3 ranks
(tests/pose_moments_dist_worker.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import eslam_abi as A
import moments_cases as M
import moments_ref as R
from parity_util import assert_bit_identical

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# (n, eslam_config.sum_chunk_rows): one row per chunk, two rows, the default rule
SIZES = [(n, 1) for n in (1, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097, 12289)] + [(4097, 2), (12289, 0)]


def config(rows):
    cfg = A.default_config()
    cfg.sum_chunk_rows = rows
    return cfg


def assert_same(got, want, label):
    """got: GpuFilter.pose_moments' PoseMoments; want: moments_ref's (rc, PoseMoments)"""
    assert want[0] == 0, label
    assert got.as_tuple() == want[1].as_tuple(), (label, got.as_dict(), want[1].as_dict())


def check(g, c, rows, gate, label):
    """ungated and gated, each twice in a row (the kept scratch)"""
    for gt, what in ((None, "ungated"), (gate, "gated"), (None, "ungated again")):
        want = R.moments(*[c[f] for f in M.FIELDS], gate=gt, sum_chunk_rows=rows)
        for call in (1, 2):
            assert_same(g.pose_moments(gt), want, f"{label} {what} call {call}")


@pytest.mark.parametrize("n,rows", SIZES)
def test_moments_equal_restatement(gpu_mod, n, rows):
    c, gate = M.cloud(n, seed=100 + n)
    g = gpu_mod.GpuFilter(config(rows))
    g.upload(M.particles(c))
    check(g, c, rows, gate, f"n={n} rows={rows}")
    m = g.pose_moments(gate)
    assert m.particles_counted + m.particles_gated_out == n and m.particles_skipped == 0
    assert n < 64 or 0 < m.particles_counted < n
    g.close()


@pytest.mark.parametrize("n,rows", [(257, 1), (4097, 2), (12289, 0)])
def test_skipped_particles(gpu_mod, n, rows):
    c, gate = M.cloud(n, seed=7)
    c, cnt = M.with_skipped(c, seed=n)
    g = gpu_mod.GpuFilter(config(rows))
    g.upload(M.particles(c))
    check(g, c, rows, gate, f"skipped n={n}")
    m = g.pose_moments()
    assert m.particles_skipped == cnt == len(M.SKIP_KINDS) * 2 and m.particles_counted == n - cnt
    # no valid particle at all: the counts, every double zero
    c["w"][:] = 0.0
    g.upload(M.particles(c))
    for gt in (None, gate):
        m = g.pose_moments(gt)
        assert_same(m, R.moments(*[c[f] for f in M.FIELDS], gate=gt, sum_chunk_rows=rows), "no valid particle")
        assert (m.particles_counted, m.particles_gated_out, m.particles_skipped) == (0, 0, n) and not any(m.doubles())
    g.close()


def test_every_particle_gated_out(gpu_mod):
    c, _ = M.cloud(1000, seed=3)
    far = A.PoseGate((-500.0, 500.0), (1.0, 0.0, 1.0), 1.0)
    g = gpu_mod.GpuFilter(config(1))
    g.upload(M.particles(c))
    m = g.pose_moments(far)
    assert_same(m, R.moments(*[c[f] for f in M.FIELDS], gate=far, sum_chunk_rows=1), "all gated out")
    assert (m.particles_counted, m.particles_gated_out) == (0, 1000) and not any(m.doubles())
    assert m.weight_exp == g.pose_moments().weight_exp
    g.close()


@pytest.mark.parametrize("scale", [1e-290, 1e290])
def test_weight_extremes(gpu_mod, scale):
    n = 1000
    c, gate = M.cloud(n, seed=12)
    c["w"] = c["w"] / 3e-7 * scale
    g = gpu_mod.GpuFilter(config(1))
    g.upload(M.particles(c))
    check(g, c, 1, gate, f"weights at {scale}")
    # a power of two moves weight_exp and nothing else
    k = 40 if scale < 1 else -40
    base = [g.pose_moments(gt).as_tuple() for gt in (None, gate)]
    g.upload(M.particles(dict(c, w=np.ldexp(c["w"], k))))
    for b, gt in zip(base, (None, gate)):
        t = g.pose_moments(gt).as_tuple()
        assert t[:-2] == b[:-2] and t[-2] == b[-2] + k
    g.close()


@pytest.mark.parametrize("turns", [False, True], ids=["in one turn", "whole turns apart"])
def test_yaw_cloud_across_the_cut(gpu_mod, turns):
    n = 4097
    c = M.across_the_cut(n, seed=21)
    if turns:
        c = M.whole_turns(c, seed=22)
    gate = A.PoseGate((1000.0, -2000.0), (0.16, 0.02, 0.0625), 2.0)
    g = gpu_mod.GpuFilter(config(1))
    g.upload(M.particles(c))
    check(g, c, 1, gate, "across the cut")
    m = g.pose_moments()
    assert np.pi - abs(m.mean[3]) <= 0.07 and abs(m.cov[15] - 0.09) < 0.015
    g.close()


def test_after_a_resample_with_its_gather_pending(gpu_mod):
    n = 1000
    c, gate = M.cloud(n, seed=31)
    c["w"] = c["w"] ** 3                              # concentrated: many particles are dropped, others copied
    c["w"] = c["w"] / c["w"].sum()
    g = gpu_mod.GpuFilter(config(1))
    g.upload(M.particles(c))
    g.resample()                                      # the gather is left to the next reader
    got = g.pose_moments(gate)
    pa = g.download()
    assert not np.array_equal(pa.x, c["x"])
    assert_same(got, R.of_particles(pa, gate, 1), "after resample()")
    assert_same(g.pose_moments(), R.of_particles(pa, None, 1), "after resample(), ungated")
    g.close()


def test_filter_unchanged(gpu_mod):
    """a call between two steps changes no later step (the twin never calls), and particles, weights
    and RNG state around a call are bit-identical"""
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
    m = a.pose_moments()                              # with whatever the third step left pending
    assert m.particles_counted == n and m.particles_skipped == 0
    a.pose_moments(A.PoseGate((m.mean[0], m.mean[1]), (m.cov[0] + 1e-6, m.cov[1], m.cov[5] + 1e-6), 4.0))
    for f in (a, b):
        f.step(stream[3])
    pa, pb = a.download(), b.download()
    assert_bit_identical(pa, pb, "a step after a call")
    assert bytes(a.rng_state()) == bytes(b.rng_state())
    ia, ib = a.sync(), b.sync()
    assert (ia.effective, ia.weight_sum, ia.resampled) == (ib.effective, ib.weight_sum, ib.resampled)
    r0 = bytes(a.rng_state())
    gate = A.PoseGate((0.0, 0.0), (0.01, 0.0, 0.01), 9.0)
    got = [a.pose_moments(), a.pose_moments(gate)]
    assert_bit_identical(a.download(), pa, "particles around a call")
    assert bytes(a.rng_state()) == r0
    assert_same(got[0], R.of_particles(pa, None, cfg.sum_chunk_rows), "the stepped filter")
    assert_same(got[1], R.of_particles(pa, gate, cfg.sum_chunk_rows), "the stepped filter, gated")
    a.close()
    b.close()


BAD_GATES = [dict(cov=(1.0, 1.0, 1.0)), dict(cov=(1.0, 2.0, 1.0)), dict(cov=(-1.0, 0.0, -1.0)), dict(cov=(0.0, 0.0, 1.0)),
             dict(cov=(np.nan, 0.0, 1.0)), dict(cov=(np.inf, 0.0, 1.0)), dict(cov=(1e200, 0.0, 1e200)), dict(chi2=-1.0),
             dict(chi2=np.inf), dict(chi2=np.nan), dict(centre=(np.nan, 0.0)), dict(centre=(0.0, -np.inf))]


def test_error_codes_leave_the_filter_usable(gpu_mod):
    """ESLAM_ERR_NOT_INITIALISED and every ESLAM_ERR_INVALID_ARG.  Not covered: a poisoned filter
    returning its fault (check_poisoned, the line every entry point shares); poisoning a context
    means making a device wait give up, which this file does not do."""
    n = 257
    c, gate = M.cloud(n, seed=2)
    g = gpu_mod.GpuFilter(config(1))
    with pytest.raises(gpu_mod.EslamError) as e:
        g.pose_moments()
    assert e.value.code == A.ERR_NOT_INITIALISED
    g.upload(M.particles(c))
    want = R.moments(*[c[f] for f in M.FIELDS], gate=gate, sum_chunk_rows=1)
    before = g.download()
    for kw in BAD_GATES:
        with pytest.raises(gpu_mod.EslamError) as e:
            g.pose_moments(A.PoseGate(**kw))
        assert e.value.code == A.ERR_INVALID_ARG, kw
        assert R.moments(*[c[f] for f in M.FIELDS], gate=A.PoseGate(**kw))[0] == A.ERR_INVALID_ARG, kw
        assert_same(g.pose_moments(gate), want, f"after {kw}")
    out = A.PoseMoments()
    assert g.L.eslam_gpu_pose_moments(g.h, None, None) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_pose_moments(None, None, C.byref(out)) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_pose_moments(g.h, C.byref(A.PoseGate(chi2=0.0)), C.byref(out)) == 0      # chi2 = 0 is a gate
    assert out.particles_gated_out == n
    assert_bit_identical(g.download(), before, "the refused calls")
    g.close()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_moments_equal_one_gpu(gpu_mod, tmp_path, world):
    """gloo ranks sharing the GPU (tests/pose_moments_dist_worker.py), shards of unequal chunk
    counts: every rank's result is the single context's bit for bit, gated and ungated; a refused
    gate is refused before any collective and differing gates on every rank, nobody hanging"""
    import pose_moments_dist_worker as W
    n_global = 1050                                   # 17 chunks of 64: 8 + 9, or 5 + 6 + 6
    store = str(tmp_path / "store")
    procs, outs = [], []
    for r in range(world):
        out = str(tmp_path / f"rank{r}.npz")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), ESLAM_DIST_STORE=store, OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "pose_moments_dist_worker.py"), str(n_global), out], env=env,
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
    c, gates = W.global_cloud(n_global)
    one = gpu_mod.GpuFilter(A.default_config())
    one.upload(M.particles(c))
    for p in parts:
        assert p["codes"].tolist() == [A.ERR_INVALID_ARG] * (len(W.BAD) + 2)
    for i, gt in enumerate(gates):
        m = one.pose_moments(gt)
        assert_same(m, R.moments(*[c[f] for f in M.FIELDS], gate=gt), f"one GPU, call {i}")
        want = [v & (2 ** 64 - 1) for v in m.as_tuple()]
        for r, p in enumerate(parts):
            assert p[f"m{i}"].tolist() == want, (i, r)
    one.close()
