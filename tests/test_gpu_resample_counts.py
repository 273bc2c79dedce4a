"""eslam_gpu_resample_stratified / eslam_gpu_resample_multinomial to any count, on the GPU, bit
for bit against the CPU reference tests/c/resample_ref.c (pinned to the oracle by
tests/test_resample_ref.py): every particle field after a numpy gather by the reference's
ancestors, the ancestors, the info and the RNG state.

The kernels' tile is 2048 particles (a coarse entry of the cumulative sum) and 2048 draws (a
compaction tile): 70 001 and 33 333 span 35 and 17 of either.  The path picks no tile width by
count, so there is no case above 512k or 2M."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eslam_abi as A
import resample_ref as R
import synthetic as S
from parity_util import assert_bit_identical
from test_resample_ref import gather, particles

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTS = [(1, 1), (1, 130), (63, 64), (65, 63), (257, 255), (2049, 5000), (5000, 777), (70001, 33333), (33333, 70001)]


def patterns(n, rng):
    """the weight patterns of one count (name -> weights); patterns a count cannot hold are left out"""
    out = {}
    w = rng.uniform(size=n)
    out["normalised"] = w / w.sum()
    for name, i in (("all_first", 0), ("all_middle", n // 2), ("all_last", n - 1)):
        v = np.zeros(n)
        v[i] = 1.0
        out[name] = v
    if n >= 5:
        v = rng.uniform(size=n)
        v[:max(n // 7, 2)] = 0.0                               # runs of zeros: the first particles,
        v[n // 2:n // 2 + max(n // 9, 2)] = 0.0                # a run inside,
        v[-max(n // 5, 1):] = 0.0                              # and the last ones
        out["zero_runs"] = v / v.sum()
    out["sum_0.37"] = rng.uniform(size=n) * (0.37 / (0.5 * n)) if n > 1 else np.array([0.37])
    out["sum_5.3"] = rng.uniform(size=n) * (5.3 / (0.5 * n)) if n > 1 else np.array([5.3])
    if n >= 2:
        v = rng.uniform(size=n)
        v[::2] = 1e-30                                         # fixes to 0 at any shift in use
        out["tiny"] = v / v.sum()
    return out


def config(flags=A.FLAG_RECORD_ANCESTORS):
    cfg = A.default_config()
    cfg.flags |= flags
    return cfg


def state_of(g):
    return g.download(), g.rng_state().minstd_x, g.count()


@pytest.mark.parametrize("kind", ["stratified", "multinomial"])
@pytest.mark.parametrize("n,samples", COUNTS)
def test_counts_equal_the_reference(gpu_mod, kind, n, samples):
    g = gpu_mod.GpuFilter(config())
    rng = np.random.default_rng(1000 * n + samples)
    multi = kind == "multinomial"
    for name, w in patterns(n, rng).items():
        label = f"{kind} {n} -> {samples} {name}"
        pa = particles(w)
        g.upload(pa)
        x0 = g.rng_state().minstd_x
        shift = R.shift_of(g.weights_sum())
        anc, beyond, x1 = (R.multinomial if multi else R.stratified)(w, samples, x0, shift)
        if multi and name == "sum_0.37" and samples > 1:
            assert 0 < beyond < samples, label                 # draws are dropped, and not all of them
        info = (g.resample_multinomial if multi else g.resample_stratified)(samples)
        want = (n, len(anc), 0 if multi else beyond, beyond if multi else 0)
        assert (info.n_before, info.n_after, info.overruns, info.dropped) == want, label
        assert g.count() == len(anc), label
        assert g.rng_state().minstd_x == x1, label
        if len(anc):
            assert np.array_equal(g.ancestors(), anc), label
        assert_bit_identical(g.download(), gather(pa, anc, 1.0 / n if multi else None), label)
    g.close()


@pytest.mark.parametrize("n", [1, 777, 70001])
def test_stratified_at_n_is_resample(gpu_mod, n):
    """samples == n: particles, ancestors and RNG state of eslam_gpu_resample on a second context"""
    rng = np.random.default_rng(n)
    for name, w in patterns(n, rng).items():
        pa = particles(w)
        a, b = gpu_mod.GpuFilter(config()), gpu_mod.GpuFilter(config())
        a.upload(pa)
        b.upload(pa)
        info = a.resample_stratified(n)
        b.resample()
        assert (info.n_before, info.n_after, info.dropped) == (n, n, 0)
        assert_bit_identical(a.download(), b.download(), name)
        assert np.array_equal(a.ancestors(), b.ancestors()), name
        assert a.rng_state().minstd_x == b.rng_state().minstd_x, name
        x0 = R.minstd_seed(a.cfg.seed)
        assert info.overruns == R.stratified(w, n, x0, R.shift_of(float(np.sum(w))))[1], name
        a.close()
        b.close()


def test_multinomial_dropping_every_draw_empties_the_filter(gpu_mod):
    n = 300
    g = gpu_mod.GpuFilter(config())
    g.set_map(S.flat_map(cells=100))
    g.upload(particles(np.zeros(n)))
    x0 = g.rng_state().minstd_x
    u = R.uniforms(x0, 500)
    assert (u > 0).all()                                       # U = 0 would take particle 0
    info = g.resample_multinomial(500)
    assert (info.n_before, info.n_after, info.dropped) == (n, 0, 500)
    assert g.count() == 0
    with pytest.raises(gpu_mod.EslamError) as e:
        g.step(S.step_stream(1)[0])
    assert e.value.code == A.ERR_NOT_INITIALISED
    with pytest.raises(gpu_mod.EslamError) as e:
        g.resample_stratified(10)
    assert e.value.code == A.ERR_NOT_INITIALISED
    g.upload(particles(np.full(10, 0.1)))                      # and it starts over like any empty filter
    assert g.count() == 10
    g.close()


def flat_filter(gpu_mod, cfg):
    g = gpu_mod.GpuFilter(cfg)
    g.set_map(S.flat_map(cells=100))
    return g


def step_record(g, stream):
    out = []
    for st in stream:
        g.step(st)
        i = g.sync()
        out.append((i.effective, i.weight_sum, i.floating_weight, i.max_weight, i.data_particles, i.total_points, i.resampled,
                    i.uniform_reset, i.resample_overruns))
    return out


def rng_tuple(r):
    return (r.minstd_x, r.project_count, r.init_count, r.hash_count, r.max_weight, tuple(r.ud_pose), r.libc_rand_pos)


@pytest.mark.parametrize("kind", ["stratified", "multinomial"])
@pytest.mark.parametrize("n,samples", [(4096, 1000), (1000, 4096)])
def test_continuation_equals_a_fresh_filter(gpu_mod, kind, n, samples):
    """3 steps of the flat golden scenario, a resize, 5 more steps: bit for bit a fresh context
    that is uploaded the resized particles and given the RNG state, then run for the same 5 steps
    -- every buffer and the chunk-row rule followed the new count.  With the best index, a
    standalone sum, the records and the centroid at the new count."""
    cfg = S.bench_config(config(), max(n, samples))            # minEffective above both counts: every update resamples
    cfg.seed = 2024
    stream = S.step_stream(8)
    a = flat_filter(gpu_mod, cfg)
    a.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)
    step_record(a, stream[:3])
    info = (a.resample_multinomial if kind == "multinomial" else a.resample_stratified)(samples)
    assert info.n_before == n and info.n_after == a.count()
    assert info.n_after == samples or kind == "multinomial"
    pa, rs = a.download(), a.rng_state()
    b = flat_filter(gpu_mod, cfg)
    b.upload(pa)
    b.set_rng_state(rs)
    assert a.weights_sum() == b.weights_sum()
    assert a.best_index() == b.best_index()
    ra, rb = step_record(a, stream[3:]), step_record(b, stream[3:])
    assert ra == rb
    assert any(r[6] for r in ra)                               # the continued steps resampled (K3 at the new count)
    assert_bit_identical(a.download(), b.download(), "continuation")
    assert np.array_equal(a.ancestors(), b.ancestors())
    assert rng_tuple(a.rng_state()) == rng_tuple(b.rng_state())
    rec_a, _ = a.download_records()
    rec_b, _ = b.download_records()
    assert rec_a.tobytes() == rec_b.tobytes()
    # getCentroid at the new count (it normalises in place, so it comes last): bit for bit the
    # fresh filter's, and the weighted mean of the particles.  Its sums run in another order than
    # numpy's: at most n = 4096 terms, so the quotients agree within n * 2^-53 relative to the
    # sums' magnitudes (positions below 1 m: 1e-11 absolute is generous)
    ca, cb = a.centroid(), b.centroid()
    assert ca == cb
    d = a.download()
    for got, field in zip(ca[0], (d.x, d.y, d.zpos)):
        assert abs(got - float(np.sum(field * d.weight) / np.sum(d.weight))) < 1e-11
    a.close()
    b.close()


def test_centroid_of_two_contexts_with_the_same_particles(gpu_mod):
    """getCentroid is a function of the particles: two contexts of one process (each on its own
    stream) holding the same set answer alike, whichever asks first, and with the weighted mean.
    (With its scratch in stream-ordered pool memory the second context to ask got another answer;
    the continuation test above met it.)"""
    rng = np.random.default_rng(11)
    w = rng.uniform(size=1000)
    pa = particles(w / w.sum())
    f = [gpu_mod.GpuFilter(config()) for _ in range(3)]
    for g in f:
        g.upload(pa)
    want = [float(np.sum(v * pa.weight)) for v in (pa.x, pa.y, pa.zpos)]
    got = [g.centroid() for g in (f[0], f[1], f[2], f[1], f[0])]
    for c in got:
        assert c == got[0]
        assert all(abs(p - q) < 1e-11 * 4 for p, q in zip(c[0], want))      # |x| up to 4 here
    for g in f:
        g.close()


@pytest.mark.parametrize("n,samples", [(4096, 1000), (1000, 4096)])
def test_resize_then_save_and_load(gpu_mod, n, samples):
    cfg = S.bench_config(config(), n)
    stream = S.step_stream(6)
    a = flat_filter(gpu_mod, cfg)
    a.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)
    step_record(a, stream[:3])
    a.resample_stratified(samples)
    blob = a.save_state()
    b = gpu_mod.GpuFilter(cfg)
    b.load_state(blob)
    assert b.count() == samples
    assert step_record(a, stream[3:]) == step_record(b, stream[3:])
    assert_bit_identical(a.download(), b.download(), "save / load after a resize")
    assert rng_tuple(a.rng_state()) == rng_tuple(b.rng_state())
    a.close()
    b.close()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_particle_maps_follow_their_ancestors(gpu_mod, oracle):
    """512 particles with their own maps, a map update, stratified to 200 and multinomial to 512,
    another map update: every particle's map is its ancestor's map before the calls merged with
    the new scan -- the oracle's map of that ancestor, which it updated at the same pose without
    resampling.  Beyond the capacity: ESLAM_ERR_UNSUPPORTED, nothing changed."""
    n = 512
    cfg = S.bench_config(config(A.FLAG_RECORD_ANCESTORS | A.FLAG_PARTICLE_MAPS), n)
    grid = S.unmapped_beyond(S.rough_map(cells=80), 0.3)
    g = gpu_mod.GpuFilter(cfg)
    o = oracle.OracleFilter(cfg, oracle.SUM_CONTRACT)
    for f in (g, o):
        f.set_map(grid)
        f.init_gaussian(n, [0.0, 0.0, 0.0], [0.05, 0.05, 0.02], 0.18, 0.05)
    scan = S.scan_patches()
    assert g.step(S.step_stream(1)[0]) == o.step(S.step_stream(1)[0])    # normalised weights (init leaves them 0)
    g.map_update(scan)
    o.map_update(scan)
    # beyond the capacity the maps were sized for
    before, x0, _ = state_of(g)
    maps0 = [g.particle_map(i) for i in (0, 100, n - 1)]
    for call in (g.resample_stratified, g.resample_multinomial):
        with pytest.raises(gpu_mod.EslamError) as e:
            call(n + 1)
        assert e.value.code == A.ERR_UNSUPPORTED
    after, x1, cnt = state_of(g)
    assert cnt == n and x1 == x0
    assert_bit_identical(after, before, "refused call")
    for i, m0 in zip((0, 100, n - 1), maps0):
        assert all(np.array_equal(u32(p), u32(q)) for p, q in zip(g.particle_map(i), m0))
    # the particles' poses differ, so a particle's map tells its ancestor
    i1 = g.resample_stratified(200)
    a1 = g.ancestors().astype(np.int64)
    assert i1.n_after == 200 and len(np.unique(a1)) > 50
    i2 = g.resample_multinomial(512)
    a2 = g.ancestors().astype(np.int64)
    # the 200 carried weights sum to 200 / 512: most of the 512 draws are dropped
    assert i2.n_before == 200 and i2.n_after == g.count() == len(a2) and i2.n_after + i2.dropped == 512
    assert 100 < i2.n_after < 300
    anc = a1[a2]
    assert len(np.unique(anc)) < len(anc)                      # copies share a table until the update
    pa, po = g.download(), o.download()
    for f in ("x", "y", "orientation", "zpos", "zsigma"):
        assert np.array_equal(getattr(pa, f).view(np.uint64), getattr(po, f)[anc].view(np.uint64)), f
    g.map_update(scan)
    o.map_update(scan)
    info = g.sync()
    assert info.map_patches_dropped == 0 and info.map_stores_copied > 0
    for k in range(len(anc)):
        gc, gm, gs = g.particle_map(k)
        oc, om, os_ = o.particle_map(int(anc[k]))
        go, oo = np.argsort(gc), np.argsort(oc)
        assert len(gc) > 0 and np.array_equal(gc[go], oc[oo]), k
        assert np.array_equal(u32(gm[go]), u32(om[oo])) and np.array_equal(u32(gs[go]), u32(os_[oo])), k
    g.close()


def test_invalid_counts_change_nothing(gpu_mod):
    n = 1000
    g = gpu_mod.GpuFilter(config())
    w = np.random.default_rng(3).uniform(size=n)
    g.upload(particles(w / w.sum()))
    before, x0, _ = state_of(g)
    for call in (g.resample_stratified, g.resample_multinomial):
        for samples in (0, 2 ** 32 - 1, 2 ** 32, 2 ** 40):
            with pytest.raises(gpu_mod.EslamError) as e:
                call(samples)
            assert e.value.code == A.ERR_INVALID_ARG, samples
    after, x1, cnt = state_of(g)
    assert cnt == n and x1 == x0
    assert_bit_identical(after, before, "invalid samples")
    # a null info is allowed
    assert g.L.eslam_gpu_resample_stratified(g.h, 10, None) == 0 and g.count() == 10
    g.close()


@pytest.mark.parametrize("maps", [False, True])
def test_sharded_filters_resample_to_their_own_count_only(gpu_mod, tmp_path, maps):
    """two gloo ranks (tests/resample_dist_worker.py): multinomial and a stratified call with
    samples != n_global return ESLAM_ERR_UNSUPPORTED on both ranks and neither blocks; stratified
    with samples == n_global is one context's eslam_gpu_resample -- also with per-particle maps,
    whose capacity on a rank is the shard's, below n_global"""
    n_global, world = 3000, 2
    store = str(tmp_path / "store")
    procs, outs = [], []
    for r in range(world):
        out = str(tmp_path / f"rank{r}.npz")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), ESLAM_DIST_STORE=store, OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "resample_dist_worker.py"), str(n_global), out] +
                                      (["maps"] if maps else []), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
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
    from resample_dist_worker import shard_particles
    pa = shard_particles(n_global, 0, n_global)
    one = gpu_mod.GpuFilter(config())
    one.upload(pa)
    one.resample()
    want, want_anc = one.download(), one.ancestors()
    for p in parts:
        assert p["codes"].tolist() == [A.ERR_UNSUPPORTED] * 3
        assert p["info"].tolist()[:2] == [n_global, n_global]
        assert int(p["rng"][0]) == one.rng_state().minstd_x
    for f in A.ParticleArrays.FIELDS:
        got = np.concatenate([p[f] for p in parts])
        assert np.array_equal(got.view(np.uint8), getattr(want, f).view(np.uint8)), f
    assert np.array_equal(np.concatenate([p["anc"] for p in parts]), want_anc)
    one.close()


@pytest.mark.parametrize("kind", ["stratified", "multinomial"])
def test_draws_beyond_the_first_jump_table_block(gpu_mod, kind):
    """2^22 + 100 draws from 3 particles: draw k's minstd value comes from the three jump tables,
    and the third (bits 22 and up of k + 1) is read beyond its first entry only from k = 2^22 - 1
    on.  The ancestors of every draw against the reference (no download: the gather is checked
    at the other counts)."""
    samples = (1 << 22) + 100
    w = np.array([0.3, 0.25, 0.45])
    g = gpu_mod.GpuFilter(config())
    g.upload(particles(w))
    x0 = g.rng_state().minstd_x
    multi = kind == "multinomial"
    anc, beyond, x1 = (R.multinomial if multi else R.stratified)(w, samples, x0, R.shift_of(g.weights_sum()))
    info = (g.resample_multinomial if multi else g.resample_stratified)(samples)
    assert (info.n_before, info.n_after, info.overruns + info.dropped) == (3, len(anc), beyond)
    assert g.rng_state().minstd_x == x1
    got = g.ancestors()
    assert np.array_equal(got, anc)
    assert len(np.unique(got[1 << 22:])) == 3 or not multi     # the last 100 draws are not all one particle
    g.close()
