"""eslam_gpu_kld_count and eslam_gpu_resample_kld on the device (eslam_kld.hip).
The count against the CPU restatement (tests/c/kld_ref.c): every info field equal, the bound by
its bits, on every shared case of tests/kld_cases.py -- sizes around the wave, the block and
several blocks, one contended bin, the 64 bits of one word and a 65th, coordinates on bin edges,
yaw edge values, every kind of skipped particle, no counted particle, a cloud too spread.  Then a
pending resample gather, the unchanged filter, every refused argument; resample_kld against a twin
given eslam_gpu_resample_stratified / _multinomial(info.samples); and a filter sharded over 2 and
3 ranks (tests/kld_dist_worker.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import eslam_abi as A
import kld_cases as K
import kld_ref as R
from parity_util import assert_bit_identical

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = K.cases()


def config(n=250, flags=0, rows=1):
    cfg = A.default_config()
    cfg.sum_chunk_rows = rows
    cfg.particle_count = n
    cfg.flags |= flags
    return cfg


def particles(x, y, th, w):
    pa = A.ParticleArrays(x.shape[0])
    pa.x[:], pa.y[:], pa.orientation[:], pa.weight[:] = x, y, th, w
    pa.zpos[:], pa.zsigma[:] = 0.18, 0.01
    return pa


def count_or_error(g, gpu_mod, **params):
    """(rc, KldInfo) of GpuFilter.kld_count, as kld_ref.count returns it"""
    try:
        return 0, g.kld_count(**params)
    except gpu_mod.EslamError as e:
        return e.code, e.info


def assert_same_count(got, want, label):
    assert got[0] == want[0], (label, got[0], want[0])
    assert got[1].as_tuple() == want[1].as_tuple(), (label, got[1].as_dict(), want[1].as_dict())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_count_equals_restatement(gpu_mod, case):
    name, x, y, th, w, params = case
    params = dict(dict(n_min=1), **params)
    g = gpu_mod.GpuFilter(config())
    g.upload(particles(x, y, th, w))
    want = R.count(x, y, th, w, **params)
    assert_same_count(count_or_error(g, gpu_mod, **params), want, name)
    # again: the kept scratch, a bitmap that is zeroed every call
    assert_same_count(count_or_error(g, gpu_mod, **params), want, name + " again")
    g.close()


def test_one_filter_through_many_boxes(gpu_mod):
    """the scratch grows and shrinks with the box; counts in between stay right"""
    x, y, th, w = K.cloud(4096, seed=3, sigma=1.5)
    g = gpu_mod.GpuFilter(config())
    g.upload(particles(x, y, th, w))
    for params in (dict(bin_xy=1.0, theta_bins=1), dict(bin_xy=0.01, theta_bins=360), dict(bin_xy=0.1), dict(bin_xy=0.003, theta_bins=4),
                   dict(bin_xy=0.1), dict(bin_xy=0.01, theta_bins=4096, max_bins=2 ** 20), dict(bin_xy=5.0, theta_bins=2)):
        params["n_min"] = 1
        assert_same_count(count_or_error(g, gpu_mod, **params), R.count(x, y, th, w, **params), str(params))
    g.close()


def test_default_n_min_is_the_configured_count(gpu_mod):
    g = gpu_mod.GpuFilter(config(n=777))
    g.upload(particles(*K.one_bin(100)))
    info = g.kld_count()
    assert (info.bins_occupied, info.samples, info.clamped) == (1, 777, 1)
    assert g.kld_params().n_min == 777
    g.close()


def test_after_a_resample_with_its_gather_pending(gpu_mod):
    n = 1000
    x, y, th, w = K.cloud(n, seed=31)
    w = w ** 3                                        # concentrated: many particles are dropped, others copied
    g = gpu_mod.GpuFilter(config())
    g.upload(particles(x, y, th, w / w.sum()))
    g.resample()                                      # the gather is left to the next reader
    got = g.kld_count(n_min=1)
    pa = g.download()
    assert not np.array_equal(pa.x, x)
    rc, want = R.count(pa.x, pa.y, pa.orientation, pa.weight, n_min=1)
    assert rc == 0 and got.as_tuple() == want.as_tuple()
    assert got.bins_occupied < R.count(x, y, th, w, n_min=1)[1].bins_occupied
    g.close()


def test_filter_unchanged(gpu_mod):
    """a snapshot taken before a count equals one taken after; and a count between two steps, with
    whatever the step left pending, changes no later step (the twin never counts)"""
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
    info = a.kld_count(n_min=1)                       # with whatever the third step left pending
    assert info.particles_counted == n and info.bins_occupied > 1
    for f in (a, b):
        f.step(stream[3])
    pa, pb = a.download(), b.download()
    assert_bit_identical(pa, pb, "a step after a count")
    assert bytes(a.rng_state()) == bytes(b.rng_state())
    blob = a.save_state()
    got = a.kld_count(n_min=1, bin_xy=0.02)
    assert np.array_equal(a.save_state(), blob)
    assert bytes(a.rng_state()) == bytes(b.rng_state())
    rc, want = R.count(pa.x, pa.y, pa.orientation, pa.weight, n_min=1, bin_xy=0.02)
    assert rc == 0 and got.as_tuple() == want.as_tuple()
    with pytest.raises(gpu_mod.EslamError):
        a.kld_count(n_min=1, bin_xy=1e-4, max_bins=64)            # too spread: refused ...
    assert np.array_equal(a.save_state(), blob)                   # ... with nothing changed
    a.close()
    b.close()


BAD = (dict(bin_xy=0.0), dict(bin_xy=-0.1), dict(bin_xy=float("inf")), dict(bin_xy=float("nan")), dict(theta_bins=0),
       dict(theta_bins=4097), dict(multinomial=2), dict(epsilon=0.0), dict(epsilon=-1.0), dict(epsilon=float("inf")),
       dict(epsilon=float("nan")), dict(z_quantile=-1e-9), dict(z_quantile=float("inf")), dict(z_quantile=float("nan")),
       dict(n_min=0), dict(n_min=10, n_max=9), dict(min_change=-1e-9), dict(min_change=float("nan")))


def test_refused_arguments_leave_the_filter_usable(gpu_mod):
    """ESLAM_ERR_NOT_INITIALISED and every ESLAM_ERR_INVALID_ARG, for both calls"""
    n = 257
    x, y, th, w = K.cloud(n, seed=2)
    g = gpu_mod.GpuFilter(config())
    for call in (g.kld_count, g.resample_kld):
        with pytest.raises(gpu_mod.EslamError) as e:
            call()
        assert e.value.code == A.ERR_NOT_INITIALISED
    g.upload(particles(x, y, th, w / w.sum()))
    want = R.count(x, y, th, w / w.sum(), n_min=1)[1]
    before = g.download()
    for kw in BAD:
        for call in (g.kld_count, g.resample_kld):
            with pytest.raises(gpu_mod.EslamError) as e:
                call(**kw)
            assert e.value.code == A.ERR_INVALID_ARG, kw
            assert g.L.eslam_gpu_last_error(g.h).decode().startswith("kld: "), kw
        assert g.kld_count(n_min=1).as_tuple() == want.as_tuple(), kw
    p, info = g.kld_params(n_min=1), A.KldInfo()
    assert g.L.eslam_gpu_kld_count(g.h, None, C.byref(info)) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_kld_count(g.h, C.byref(p), None) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_kld_count(None, C.byref(p), C.byref(info)) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_resample_kld(g.h, None, None, None) == A.ERR_INVALID_ARG
    assert g.L.eslam_gpu_resample_kld(None, C.byref(p), None, None) == A.ERR_INVALID_ARG
    assert g.count() == n
    assert_bit_identical(g.download(), before, "the refused calls")
    # a too-spread cloud refuses the resample too, with the box in info and nothing changed
    with pytest.raises(gpu_mod.EslamError) as e:
        g.resample_kld(n_min=1, max_bins=64)
    assert e.value.code == A.ERR_UNSUPPORTED and e.value.info.bins[0] > 1 and e.value.info.samples == 0
    assert_bit_identical(g.download(), before, "the refused resample")
    # both infos may be null
    assert g.L.eslam_gpu_resample_kld(g.h, C.byref(g.kld_params(n_min=300, n_max=300)), None, None) == 0
    assert g.count() == 300
    g.close()


def twins(gpu_mod, cfg, pa, grid=None):
    out = []
    for _ in range(2):
        f = gpu_mod.GpuFilter(cfg)
        if grid is not None:
            f.set_map(grid)
        f.upload(pa)
        out.append(f)
    return out


def assert_same_filter(a, b, label, ancestors=True):
    assert a.count() == b.count(), label
    assert_bit_identical(a.download(), b.download(), label)
    assert bytes(a.rng_state()) == bytes(b.rng_state()), label
    if ancestors:
        assert np.array_equal(a.ancestors(), b.ancestors()), label


# (name, n, sigma, params, what the count must do)
RESAMPLES = [("shrink", 4096, 0.03, dict(n_min=1), "shrink"),
             ("shrink_multinomial", 4096, 0.03, dict(n_min=1, multinomial=1), "shrink"),
             ("grow", 257, 0.3, dict(n_min=1), "grow"),
             ("grow_multinomial", 257, 0.3, dict(n_min=1, multinomial=1), "grow"),
             ("n_max", 1000, 0.3, dict(n_min=1, n_max=640), "shrink"),
             ("held", 1000, 0.3, dict(n_min=1, min_change=1e6), "held"),
             ("held_multinomial", 1000, 0.3, dict(n_min=1, min_change=1e6, multinomial=1), "held")]


@pytest.mark.parametrize("case", RESAMPLES, ids=[c[0] for c in RESAMPLES])
def test_resample_kld_equals_the_resample_to_its_count(gpu_mod, case):
    name, n, sigma, params, what = case
    x, y, th, w = K.cloud(n, seed=len(name), sigma=sigma)
    pa = particles(x, y, th, w / w.sum())
    a, b = twins(gpu_mod, config(n=n, flags=A.FLAG_RECORD_ANCESTORS), pa)
    want = R.count(x, y, th, w / w.sum(), **params)[1]
    info, rinfo = a.resample_kld(**params)
    assert info.as_tuple() == want.as_tuple()
    if what == "shrink":
        assert info.samples < n
    elif what == "grow":
        assert info.samples > n                      # beyond the capacity: a larger particle set
    else:
        assert info.samples == n and info.clamped & 8
    twin = (b.resample_multinomial if params.get("multinomial") else b.resample_stratified)(info.samples)
    assert rinfo.as_dict() == twin.as_dict() and rinfo.n_before == n
    assert_same_filter(a, b, name)
    if what == "held" and not params.get("multinomial"):
        c = twins(gpu_mod, config(n=n, flags=A.FLAG_RECORD_ANCESTORS), pa)[0]
        c.resample()                                 # at an unchanged count the call is eslam_gpu_resample
        assert_same_filter(a, c, name + " against resample()")
        c.close()
    # the filter goes on at the new count
    assert a.kld_count(**params).as_tuple() == b.kld_count(**params).as_tuple()
    a.close()
    b.close()


def test_particle_maps_cut_to_the_capacity_then_a_step(gpu_mod):
    """per-particle maps: the count asked for exceeds the capacity the maps were sized for and is
    cut to it (bit 2); a smaller one shrinks the filter; a contact step runs after each"""
    import synthetic as S
    n = 512
    cfg = S.bench_config(config(flags=A.FLAG_RECORD_ANCESTORS | A.FLAG_PARTICLE_MAPS, rows=0), n)
    grid = S.unmapped_beyond(S.rough_map(cells=80), 0.3)
    stream = S.step_stream(3)
    scan = S.scan_patches()
    a, b = gpu_mod.GpuFilter(cfg), gpu_mod.GpuFilter(cfg)
    for f in (a, b):
        f.set_map(grid)
        f.init_gaussian(n, [0.0, 0.0, 0.0], [0.05, 0.05, 0.02], 0.18, 0.05)
        f.step(stream[0])                            # normalised weights (init leaves them 0)
        f.map_update(scan)
    fine = dict(n_min=1, bin_xy=0.002, theta_bins=360)
    info, rinfo = a.resample_kld(**fine)
    assert info.bound > n and info.samples == n and info.clamped == 4 | 8
    b.resample_stratified(n)
    assert (rinfo.n_before, rinfo.n_after) == (n, n)
    for f in (a, b):
        f.step(stream[1])
        f.map_update(scan)
    assert_same_filter(a, b, "cut to the capacity, then a step", ancestors=False)
    coarse = dict(n_min=1, bin_xy=0.25, theta_bins=4)
    info, rinfo = a.resample_kld(**coarse)
    assert 1 < info.samples < n and rinfo.n_after == info.samples
    b.resample_stratified(info.samples)
    for f in (a, b):
        f.step(stream[2])
        f.map_update(scan)
    assert_same_filter(a, b, "shrunk with maps, then a step", ancestors=False)
    for i in (0, info.samples - 1):
        assert all(np.array_equal(p, q) for p, q in zip(a.particle_map(i), b.particle_map(i)))
    a.close()
    b.close()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def words(info):
    import kld_dist_worker as W
    return W.info_words(info).tolist()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_equals_one_gpu(gpu_mod, tmp_path, world):
    """gloo ranks sharing the GPU (tests/kld_dist_worker.py): every rank's info is the single
    context's bit for bit; resample_kld leaves the shards that one context's result laid out by
    eslam_gpu_shard_bounds gives; bad arguments and per-particle maps are refused before any
    collective, differing parameters on every rank, nobody hanging"""
    import kld_dist_worker as W
    store = str(tmp_path / "store")
    procs, outs = [], []
    for r in range(world):
        out = str(tmp_path / f"rank{r}.npz")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), ESLAM_DIST_STORE=store, OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "kld_dist_worker.py"), out], env=env,
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
    # A: the refusals and the counts
    xa = W.cloud_a()
    one = gpu_mod.GpuFilter(A.default_config())
    one.upload(W.particles(*xa))
    for p in parts:
        assert p["a/codes"].tolist() == [A.ERR_INVALID_ARG] * (len(W.BAD) + 4)
        assert p["a/spread"].tolist() == [A.ERR_UNSUPPORTED] * 2
    for i, params in enumerate(W.COUNTS):
        info = one.kld_count(**params)
        assert info.as_tuple() == R.count(*xa, **params)[1].as_tuple(), i
        for r, p in enumerate(parts):
            assert p[f"a/info{i}"].tolist() == words(info), (i, r)
    table = A.shard_bounds(W.N, world)
    pa = one.download()
    for r, p in enumerate(parts):
        for fld in A.ParticleArrays.FIELDS:
            assert same_bits(p[f"a/{fld}"], getattr(pa, fld)[table[r]:table[r + 1]]), (fld, r)
    one.close()
    # B: the sequence of counts and resamples on one context
    cfg = A.default_config()
    cfg.particle_count = W.N
    one = gpu_mod.GpuFilter(cfg)
    one.upload(W.particles(*W.cloud_b()))
    rec = {}
    W.run_ops(rec, one)
    counts = []
    for i, (what, params) in enumerate(W.OPS):
        key = f"ops/{i}"
        n_now = rec[f"{key}/x"].shape[0]
        counts.append(n_now)
        table = A.shard_bounds_c(one.L, n_now, world)
        for r, p in enumerate(parts):
            if what != "normalize":
                assert p[f"{key}/info"].tolist() == rec[f"{key}/info"].tolist(), (key, r)
            if what == "resample":
                assert p[f"{key}/rinfo"].tolist() == rec[f"{key}/rinfo"].tolist(), (key, r)
            assert p[f"{key}/rng"].tolist() == rec[f"{key}/rng"].tolist(), (key, r)
            for fld in A.ParticleArrays.FIELDS:
                want = rec[f"{key}/{fld}"][table[r]:table[r + 1]]
                assert same_bits(p[f"{key}/{fld}"], want), (key, fld, r)
    assert [w for w, _ in W.OPS] == ["resample", "count", "resample", "count", "normalize", "resample", "resample"]
    assert counts[0] > W.N and counts[2] < counts[0] and counts[5] == counts[3] and counts[6] != counts[5], counts
    for p in parts:
        assert p["b/bounds"].tolist() == A.shard_bounds_c(one.L, counts[-1], world)
    one.close()
    # C: refused by the sharded resample on every rank, nothing changed; D: refused before any collective
    xc = K.one_bin(W.N)
    table = A.shard_bounds(W.N, world)
    for r, p in enumerate(parts):
        assert p["c/code"].tolist() == [A.ERR_INVALID_ARG] and p["c/count"].tolist() == [table[r + 1] - table[r], W.N]
        assert np.array_equal(p["c/x"], xc[0][table[r]:table[r + 1]]) and np.array_equal(p["c/weight"], xc[3][table[r]:table[r + 1]])
        assert p["d/code"].tolist() == [A.ERR_UNSUPPORTED] * 2
        assert p["d/info"].tolist() == parts[0]["d/info"].tolist()
        assert p["d/fixed"].tolist() == [W.N, p["d/fixed"][1], W.N, W.N, table[r + 1] - table[r]]
