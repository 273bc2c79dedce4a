"""K3's draw counting decides "stratified draw <= target" in integers (dm_draw_compare) and
evaluates the draws only for a wave that holds an ambiguous target.  Both ways must give the
oracle's resample: ancestors and every particle field bit for bit, at sizes around the wave (64
particles x items), the tile (256 x items) and several tiles, with the 8-items instantiation
the large filters run (debug_set_scan_items) and with the rule by particle count.

Which waves fall back follows from the weights: equal weights 1 / n with n a power of two put
every target on a stratum edge (remainder 0: ambiguous), one particle holding all the mass
leaves targets 0 and the total (k* = 0 with remainder 0, k* = n), and a run of exact 2^-j
weights whose start lies on a stratum edge does it for one wave among waves of random weights."""
import functools

import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import synthetic as S
from parity_util import assert_bit_identical, info_tuple

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097]
ITEMS = [8, 0]
STEPS = 5
INIT = dict(mu=[0.0, 0.0, 0.0], sigma=[0.1, 0.1, 0.1], z=0.18, zs=1.001)
FAR = dict(mu=[40.0, 40.0, 0.0], sigma=[0.1, 0.1, 0.1], z=0.18, zs=1.0)


def snapshot(f, info):
    return f.download(), info_tuple(info), np.array(f.ancestors())


def run_steps(f, grid, n, init, stream, info_fn):
    f.set_map(grid)
    f.init_gaussian(n, init["mu"], init["sigma"], init["z"], init["zs"])
    out = []
    for st in stream:
        assert f.step(st)                                        # the measurement update ran
        out.append(snapshot(f, info_fn(f)))
    return out


def forced_config(n):
    cfg = S.bench_config(A.default_config(), n)
    cfg.flags |= A.FLAG_RECORD_ANCESTORS
    return cfg


@functools.lru_cache(maxsize=None)
def oracle_flat(n):
    """the oracle's particles, info and ancestors after each of five forced-resample steps of
    the flat scenario (computed once per size, shared by both tile settings)"""
    f = O.OracleFilter(forced_config(n), O.SUM_CONTRACT)
    return run_steps(f, S.flat_map(cells=200), n, INIT, S.step_stream(STEPS), lambda g: g.info())


@functools.lru_cache(maxsize=None)
def oracle_uniform_reset(n):
    f = O.OracleFilter(forced_config(n), O.SUM_CONTRACT)
    return run_steps(f, S.flat_map(cells=20), n, FAR, S.step_stream(3, ltc=1), lambda g: g.info())


def gpu_filter(gpu_mod, cfg, items):
    f = gpu_mod.GpuFilter(cfg)
    f.debug_set_scan_items(items)
    return f


def assert_steps_equal(got, want, label):
    assert len(got) == len(want)
    for k, ((gp, gi, ga), (wp, wi, wa)) in enumerate(zip(got, want)):
        assert_bit_identical(gp, wp, f"{label} step {k}")
        assert gi == wi, f"{label} step {k}: info {gi} != {wi}"
        assert np.array_equal(ga, wa), f"{label} step {k}: ancestors differ"


@pytest.mark.parametrize("items", ITEMS)
@pytest.mark.parametrize("n", SIZES)
def test_random_weights_forced_resample(gpu_mod, oracle, n, items):
    """(a) five forced-resample steps of the flat scenario: weights that are no multiples of
    1 / n, the targets the integer decision settles"""
    want = oracle_flat(n)
    assert all(info[6] == 1 for _, info, _ in want)              # resampled every step
    gpu = gpu_filter(gpu_mod, forced_config(n), items)
    got = run_steps(gpu, S.flat_map(cells=200), n, INIT, S.step_stream(STEPS), lambda g: g.sync())
    gpu.close()
    assert_steps_equal(got, want, f"flat n={n} items={items}")


def arrays(weights, seed=3):
    n = len(weights)
    rng = np.random.default_rng(seed)
    pa = A.ParticleArrays(n)
    pa.x[:] = rng.normal(0, 0.2, n)
    pa.y[:] = rng.normal(0, 0.2, n)
    pa.orientation[:] = rng.normal(0, 0.1, n)
    pa.zpos[:] = 0.18
    pa.zsigma[:] = 0.2
    pa.weight[:] = weights
    pa.floating[:] = 1
    return pa


def resample_pair(gpu_mod, pa, items, label):
    """upload -> resample on the device and on the oracle; returns the ancestors"""
    cfg = A.default_config()
    cfg.flags |= A.FLAG_RECORD_ANCESTORS
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    gpu = gpu_filter(gpu_mod, cfg, items)
    orc.upload(pa)
    gpu.upload(pa)
    orc.resample()
    gpu.resample()
    gpu.sync()
    anc = np.array(orc.ancestors())
    assert np.array_equal(gpu.ancestors(), anc), f"{label}: ancestors differ"
    assert_bit_identical(gpu.download(), orc.download(), label)
    gpu.close()
    return anc


@pytest.mark.parametrize("items", ITEMS)
@pytest.mark.parametrize("n", [n for n in SIZES if n & (n - 1) == 0])
def test_equal_weights_every_target_on_an_edge(gpu_mod, oracle, n, items):
    """(b) weights 1 / n, n a power of two: c N is a multiple of 2^shift for every target, so
    every wave takes the fallback"""
    anc = resample_pair(gpu_mod, arrays(np.full(n, 1.0 / n)), items, f"equal n={n} items={items}")
    assert np.all(np.diff(anc.astype(np.int64)) >= 0) and anc[0] >= 0 and anc[-1] < n


@pytest.mark.parametrize("items", ITEMS)
@pytest.mark.parametrize("n", [64, 512, 2048, 2049])
def test_step_ending_in_the_uniform_reset(gpu_mod, oracle, n, items):
    """(b) no particle touches the map: normalizeWeights resets every weight to 1 / n and the
    forced resample runs on them"""
    want = oracle_uniform_reset(n)
    assert want[0][1][7] == 1 and all(info[6] == 1 for _, info, _ in want)   # step 0: uniform reset; resampled
    gpu = gpu_filter(gpu_mod, forced_config(n), items)
    got = run_steps(gpu, S.flat_map(cells=20), n, FAR, S.step_stream(3, ltc=1), lambda g: g.sync())
    gpu.close()
    assert_steps_equal(got, want, f"uniform n={n} items={items}")


def mixed_weights(n, start):
    """n = 2^11 weights in units of 2^-40, sum below 1 (shift 59: the stratum edges are the
    multiples of 2^-11 = 2^29 units).  Random odd weights, except that the particle before
    `start` brings the prefix sum onto an edge and the 64 from `start` on are exact 2^-11 and
    2^-10: each of their targets sits on an edge."""
    unit = 1 << 29
    rng = np.random.default_rng(start + 17)
    a = rng.integers(unit * 2 // 5, unit * 6 // 5, n, dtype=np.int64) | 1
    if start > 0:
        a[start - 1] += (-int(a[:start].sum())) % unit
    a[start:start + 64] = np.where(np.arange(64) % 5 == 0, 2 * unit, unit)
    assert int(a[:start].sum()) % unit == 0 and int(a.sum()) < (1 << 40)
    return a.astype(np.float64) * 2.0 ** -40           # exact


@pytest.mark.parametrize("items", ITEMS)
@pytest.mark.parametrize("offset", [0, 63, 448])
def test_dyadic_run_among_random_weights(gpu_mod, oracle, offset, items):
    """(c) the run sits at `offset` of the second 512-particle wave of the one 8-items tile:
    that wave falls back, its neighbours do not (with one item per thread: at the same
    particles, in 64-particle waves)"""
    n = 2048
    resample_pair(gpu_mod, arrays(mixed_weights(n, 512 + offset)), items, f"mixed offset={offset} items={items}")


@pytest.mark.parametrize("items", ITEMS)
@pytest.mark.parametrize("n,at", [(1, 0), (513, 200), (2049, 0), (2049, 1000), (2049, 2048), (4097, 2100)])
def test_single_weight_holds_all_the_mass(gpu_mod, oracle, n, at, items):
    """(d) one particle receives every draw: its wave takes the per-target windows (more draws
    than two chunks, n = 2049 and 4097) or the staged draws (n = 513); the targets after it
    have k* >= n"""
    w = np.zeros(n)
    w[at] = 1.0
    anc = resample_pair(gpu_mod, arrays(w), items, f"single n={n} at={at} items={items}")
    assert np.all(anc == at)


def test_one_rank_sharded_filter(oracle, tmp_path):
    """(e) k_segments_multi shares the draw counting: a one-rank sharded filter over the torch
    communicator (device buffers), forced resample every step, against the one-process oracle"""
    from test_dist_cpu import assert_same, launch, merge, single_oracle
    n = 2049
    want = single_oracle("forced", n)
    got = merge(launch("gpu", "forced", n, 1, str(tmp_path), mem="device", timeout=120))
    assert_same(got, want, f"one-rank sharded forced N={n}")
