"""The scenario of tests/test_gpu_trajectory_sharded.py: one function, run(), drives both ONE
unsharded context holding all N particles with the one-GPU trajectory log (the yardstick) and
every rank of a filter sharded over 1, 2 or 3 ranks (tests/trajectory_dist_worker.py).  It only
picks the sharded or the plain call.

N = 1050 is 17 chunks of 64 with a ragged tail: shards of 8 + 9 chunks, or 5 + 6 + 6.  The log
holds 4 entries.  Phases, each followed by the queries (query()):

  a   two updates that resample, one that does not, one step whose update gate stays closed
  b0  resample_multinomial(900): unsorted ancestors, links across the ranks, a new shard table
      (the queries start at a link that is not the identity, under a table no entry has)
  b   a resampling update: a record through the composed link
  c0  resample_stratified(1300): 21 chunks, every shard grows
  c   two updates: 7 records into 4 entries, held under three different tables
  d   all the weight written onto one particle of the last rank, then a resampling update: every
      lineage converges on one rank, some rank pairs exchange nothing

What a run saves per phase: trajectory_info, the lineages of LEAVES' particles (capacity 2 and
all), the smoothed trajectory, all as raw bytes, and the filter's particles.
"""
import numpy as np

import eslam_abi as A
import synthetic as S

N = 1050
CAPACITY = 4
PHASES = ("a", "b0", "b", "c0", "c", "d")
RESAMPLE_ALWAYS = 1 << 20                        # minEffective above every count
WORLDS = (1, 2, 3)
GROWN = 1300
TOO_MANY = 2200                                  # 35 chunks: 18 of 2 ranks, 12 of 3 are beyond MAX_PARTICLES
# per rank: room for the largest shard of GROWN (11 chunks of 2 ranks), not for TOO_MANY's
MAX_PARTICLES = {0: 1408, 1: 1408, 2: 704, 3: 704}


def config():
    from test_gpu_trajectory import config as trajectory_config     # its update gate: open after 0.02 m, closed on a repeat
    cfg = trajectory_config(N)
    cfg.min_effective = RESAMPLE_ALWAYS
    return cfg


def global_particles():
    """a Gaussian cloud around the origin with uneven weights, the same in every process"""
    rng = np.random.default_rng(N)
    pa = A.ParticleArrays(N)
    pa.x[:] = rng.normal(0.0, 0.1, size=N)
    pa.y[:] = rng.normal(0.0, 0.1, size=N)
    pa.orientation[:] = rng.normal(0.0, 0.1, size=N)
    pa.zpos[:] = 0.18
    pa.zsigma[:] = 0.05
    w = rng.uniform(0.2, 1.0, size=N)
    pa.weight[:] = w / w.sum()
    pa.mprob[:] = 1.0
    return pa


def leaves(n, best):
    """0, n - 1, both sides of every shard boundary of 2 and of 3 ranks, the best particle, a repeat"""
    out = [0, n - 1]
    for world in (2, 3):
        for b in A.shard_bounds(n, world)[1:-1]:
            out += [b - 1, b]
    return out + [best, out[2]]


def query(rec, key, f, n, log):
    pa = f.download()
    for fld in A.ParticleArrays.FIELDS:
        rec[f"{key}/{fld}"] = np.array(getattr(pa, fld))
    rec[f"{key}/n"] = np.array([n], dtype=np.uint64)
    if not log:
        return
    info = f.trajectory_info()
    # max_particles and bytes are the rank's own
    rec[f"{key}/info"] = np.array([info.enabled, info.capacity_steps, info.entries, info.first_step, info.last_step, info.particles],
                                  dtype=np.uint64)
    idx = leaves(n, f.best_index())
    rec[f"{key}/leaves"] = np.array(idx, dtype=np.uint64)
    rec[f"{key}/two"] = np.frombuffer(f.trajectories(idx, capacity=2).tobytes(), dtype=np.uint8)
    rec[f"{key}/all"] = np.frombuffer(f.trajectories(idx).tobytes(), dtype=np.uint8)
    sm = f.trajectory_smoothed()
    rec[f"{key}/smoothed"] = np.frombuffer(b"".join(bytes(e) for e in sm), dtype=np.uint8)
    rec[f"{key}/distinct"] = np.array([e.distinct_ancestors for e in sm], dtype=np.uint64)


def run(rec, f, lo, hi, sharded, log=True, world=0, before_enable=None, after_enable=None):
    """the scenario on filter f holding particles [lo, hi) of the global set.  sharded: f is a
    ShardedGpuFilter (world ranks); before_enable / after_enable: the worker's refusal checks"""
    full = global_particles()
    pa = A.ParticleArrays(hi - lo)
    for fld in A.ParticleArrays.FIELDS:
        getattr(pa, fld)[:] = getattr(full, fld)[lo:hi]
    f.set_map(S.flat_map(cells=120))
    f.upload(pa)
    if before_enable:
        before_enable()
    if log:
        f.trajectory_enable(CAPACITY, MAX_PARTICLES[world])
    if after_enable:
        after_enable()
    stream = S.step_stream(7)
    count = lambda: f.n_global if sharded else f.count()            # noqa: E731

    def step(k, resample):
        f.set_min_effective(RESAMPLE_ALWAYS if resample else 0)
        return f.step(stream[k])

    assert step(0, True) and step(1, True) and step(2, False)
    assert not step(2, False)                                       # the input again: the update gate stays closed
    query(rec, "a", f, count(), log)
    (f.resample_multinomial_sharded if sharded else f.resample_multinomial)(900)
    query(rec, "b0", f, count(), log)
    assert step(3, True)
    query(rec, "b", f, count(), log)
    (f.resample_stratified_sharded if sharded else f.resample_stratified)(GROWN)
    query(rec, "c0", f, count(), log)
    assert step(4, True) and step(5, True)
    query(rec, "c", f, count(), log)
    # all the weight on one particle of the last rank (a collective write: every rank calls it)
    g = count() - 3
    gbase = f.gbase if sharded else 0
    mine = f.download()
    mine.weight[:] = 0.0
    if gbase <= g < gbase + mine.n:
        mine.weight[g - gbase] = 1.0
    f.write(0, mine)
    assert step(6, True)
    query(rec, "d", f, count(), log)
