"""The trajectory log on the GPU (eslam_gpu_trajectory_*, eslam_gpu_get_trajectories,
eslam_gpu_trajectory_smoothed) against code that existed before it.

Three filters run the same configuration, seed, map and inputs: A with the log, B with
ESLAM_FLAG_RECORD_ANCESTORS, and C with neither.  B is downloaded after every step (download(),
sync().resampled, ancestors()) and feeds the numpy restatement (tests/trajectory_ref.py); A's log
must equal it as bits.  C, which never materialises a gather outside the fused kernels, says that
the log leaves the filter itself unchanged.  n = 1000 is no multiple of 64 and less than a chunk;
4096 + 37 has several chunks, a ragged tail and crosses the 2048-particle scan tile."""
import ctypes as C

import numpy as np
import pytest

import eslam_abi as A
import synthetic as S
import trajectory_ref as T
from parity_util import assert_bit_identical

pytestmark = pytest.mark.gpu

SIZES = [1000, 4096 + 37]
GATE = 1e-3                                  # update thresholds: open after 0.02 m, closed on a repeated input
INIT = ([0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 0.05)


def config(n, flags=0):
    cfg = S.bench_config(A.default_config(), n)
    cfg.measurement_threshold_distance = GATE
    cfg.measurement_threshold_angle = GATE
    cfg.flags |= flags
    return cfg


def with_flags(cfg, add=0, remove=0):
    c = type(cfg).from_buffer_copy(cfg)
    c.flags = (c.flags | add) & ~remove
    return c


def trio(gpu_mod, cfg, grid, init=None):
    """A (no flag; the log is enabled by the caller), B (the flag) and C (neither), initialised alike"""
    base = with_flags(cfg, remove=A.FLAG_RECORD_ANCESTORS)
    fs = [gpu_mod.GpuFilter(base), gpu_mod.GpuFilter(with_flags(base, add=A.FLAG_RECORD_ANCESTORS)), gpu_mod.GpuFilter(base)]
    for f in fs:
        f.set_map(grid)
        if init is None:
            f.init_gaussian(cfg.particle_count, *INIT)
        else:
            init(f)
    return fs


def step_all(fs, ref, st, after=None):
    """one step on every filter; B's download, resample decision and ancestors into the restatement"""
    a, b, c = fs
    upd = [f.step(st) for f in fs]
    assert upd[0] == upd[1] == upd[2]
    if after is not None:
        for f in fs:
            after(f)
    pa = b.download()
    anc = b.ancestors() if upd[1] and b.sync().resampled else None
    ref.record_particles(pa, anc)
    return upd[0], anc


def same_nodes(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), label


def assert_log_equals(a, ref, label, capacity=None):
    n = a.count()
    assert n == len(ref.link)
    same_nodes(a.trajectories(np.arange(n), capacity), ref.trace(np.arange(n), capacity), label)


def same_filter(f, g, label):
    assert_bit_identical(f.download(), g.download(), label)
    assert bytes(f.rng_state()) == bytes(g.rng_state()), label


def close_all(fs):
    for f in fs:
        f.close()


@pytest.mark.parametrize("n", SIZES)
def test_lineage_over_resampling_idle_and_gate_closed_steps(gpu_mod, n):
    fs = trio(gpu_mod, config(n), S.flat_map(cells=120))
    a, b, c = fs
    a.trajectory_enable(16)
    assert a.trajectory_info().as_dict() == dict(enabled=1, capacity_steps=16, max_particles=n, entries=0, first_step=0, last_step=0,
                                                 particles=0, bytes=a.trajectory_info().bytes)
    assert a.trajectory_info().bytes >= 16 * 44 * n + 8 * n
    ref = T.TrajectoryLog(16, n)
    stream = S.step_stream(11)
    # True: a resample forced, False: none, None: the previous input again (the update gate stays closed)
    plan = [True, False, True, True, False, None, True, False, False, True, True, False]
    k, seen = 0, []
    for p in plan:
        if p is None:
            st = stream[k - 1]
        else:
            st = stream[k]
            k += 1
            for f in fs:
                f.set_min_effective(n + 1 if p else 0)
        upd, anc = step_all(fs, ref, st)
        assert upd == (p is not None) and (anc is not None) == bool(p)
        seen.append((upd, anc is not None))
        # the newest entry whole (link is the identity now): its columns are B's download, its
        # parents B's ancestors or the identity
        assert_log_equals(a, ref, f"step {len(seen)}", capacity=2)
        if anc is None:
            assert np.array_equal(ref.entries[-1]["parent"], np.arange(n))
    assert seen.count((True, True)) == 6 and seen.count((True, False)) == 5 and seen.count((False, False)) == 1
    info = a.trajectory_info()
    assert (info.entries, info.first_step, info.last_step, info.particles) == (12, 0, 11, n)
    assert_log_equals(a, ref, "the whole log")
    # lineages did coalesce: the check above is not one of identity maps
    assert len(np.unique(ref.trace(np.arange(n))["slot"][:, 0])) < n
    same_filter(a, c, "the log leaves the filter unchanged")
    close_all(fs)


@pytest.mark.parametrize("n", SIZES)
def test_resamples_between_steps_compose_the_link(gpu_mod, n):
    fs = trio(gpu_mod, config(n), S.flat_map(cells=120))
    a, b, c = fs
    a.trajectory_enable(8, max_particles=n)
    ref = T.TrajectoryLog(8, n)
    stream = S.step_stream(5)

    def resample_all(call):
        for f in fs:
            call(f)
        assert a.count() == b.count() == c.count()
        ref.compose(b.ancestors())

    step_all(fs, ref, stream[0])
    step_all(fs, ref, stream[1])
    resample_all(lambda f: f.resample_stratified(n // 2))
    assert a.trajectory_info().entries == 2 and len(ref.link) == n // 2
    step_all(fs, ref, stream[2])
    resample_all(lambda f: f.resample_multinomial(n))
    resample_all(lambda f: f.resample())          # two compositions between two records
    step_all(fs, ref, stream[3])
    resample_all(lambda f: f.resample())
    # a query between a composition and the next record starts at link, not at the identity
    assert not np.array_equal(ref.link, np.arange(len(ref.link)))
    assert_log_equals(a, ref, "after a composition")
    step_all(fs, ref, stream[4])
    counts = [len(e["parent"]) for e in ref.entries]
    assert counts[:3] == [n, n, n // 2] and counts[2] != counts[3]
    assert_log_equals(a, ref, "the whole log")
    assert np.array_equal(a.trajectories([0])["particles"][0], counts)
    # growing beyond max_particles is refused before anything changes
    before, rng = a.download(), bytes(a.rng_state())
    entries = a.trajectory_info().entries
    for call in (lambda: a.resample_stratified(n + 64), lambda: a.resample_multinomial(n + 1)):
        with pytest.raises(gpu_mod.EslamError) as e:
            call()
        assert e.value.code == A.ERR_INVALID_ARG and "max_particles" in str(e.value)
    assert_bit_identical(a.download(), before, "a refused resample")
    assert bytes(a.rng_state()) == rng and a.count() == before.n and a.trajectory_info().entries == entries
    assert_log_equals(a, ref, "the log after the refusals")
    same_filter(a, c, "the log leaves the filter unchanged")
    close_all(fs)


def test_ring_wrap_keeps_the_newest_entries(gpu_mod):
    n = SIZES[0]
    fs = trio(gpu_mod, config(n), S.flat_map(cells=120))
    a = fs[0]
    a.trajectory_enable(4)
    ref = T.TrajectoryLog(4, n)
    for st in S.step_stream(7):
        step_all(fs, ref, st)
    info = a.trajectory_info()
    assert (info.entries, info.first_step, info.last_step, info.capacity_steps) == (4, 3, 6, 4)
    got = a.trajectories(np.arange(n))
    assert got.shape == (n, 4) and np.array_equal(got["step"][0], [3, 4, 5, 6])
    same_nodes(got, ref.trace(np.arange(n)), "four entries held")
    two = a.trajectories(np.arange(n), capacity=2)
    assert two.shape == (n, 2) and np.array_equal(two["step"][0], [5, 6])
    same_nodes(two, ref.trace(np.arange(n), 2), "the newest two")
    assert a.trajectories([0], capacity=0).shape == (1, 0)
    close_all(fs)


@pytest.mark.parametrize("n", SIZES)
def test_trace_of_chosen_particles(gpu_mod, n):
    fs = trio(gpu_mod, config(n), S.rough_map(cells=120))
    a = fs[0]
    a.trajectory_enable(8)
    ref = T.TrajectoryLog(8, n)
    for st in S.step_stream(6, tilt=True):
        step_all(fs, ref, st)
    best = a.best_index()
    idx = [0, n - 1, best, 7, 7]
    got = a.trajectories(idx)
    same_nodes(got, ref.trace(idx), "chosen leaves")
    assert got.tobytes()[-2 * got[0].nbytes:-got[0].nbytes] == got.tobytes()[-got[0].nbytes:]     # a repeated index, the same lineage
    pa = a.download()
    last = got[2, -1]
    assert last["slot"] == best and last["x"] == pa.x[best] and last["yaw"] == pa.orientation[best]
    close_all(fs)


@pytest.mark.parametrize("n", SIZES)
def test_smoothed_trajectory_equals_the_moments_of_the_ancestors(gpu_mod, n):
    cfg = config(n)
    fs = trio(gpu_mod, cfg, S.rough_map(cells=120))
    a, b, c = fs
    a.trajectory_enable(16)
    ref = T.TrajectoryLog(16, n)
    for st in S.step_stream(12, tilt=True):
        step_all(fs, ref, st)
    for f in fs:
        f.resample()                              # the newest level starts at a link that is not the identity
    ref.compose(b.ancestors())
    before, rng = a.download(), bytes(a.rng_state())
    got = a.trajectory_smoothed()
    want = ref.smoothed(before.weight, sum_chunk_rows=cfg.sum_chunk_rows)
    assert len(got) == len(want) == 12
    for k, (g, (step, distinct, m)) in enumerate(zip(got, want)):
        print(f"entry {k}: step {g.step} distinct {g.distinct_ancestors} (restated {distinct})")
        assert g.step == step and g.distinct_ancestors == distinct, k
        assert bytes(g.moments) == bytes(m), k
        assert g.moments.particles_counted == n
    # not identity maps: the newest level's ancestors are the distinct values of link, and
    # going back the lineages coalesce
    assert got[-1].distinct_ancestors == len(np.unique(ref.link)) < n
    assert got[0].distinct_ancestors < got[-1].distinct_ancestors
    # twice the same bytes, the filter and the log untouched
    again = a.trajectory_smoothed()
    assert [bytes(g) for g in again] == [bytes(g) for g in got]
    assert_bit_identical(a.download(), before, "after the smoothed queries")
    assert bytes(a.rng_state()) == rng
    assert_log_equals(a, ref, "the log after the smoothed queries")
    newest3 = a.trajectory_smoothed(capacity=3)
    assert [bytes(g) for g in newest3] == [bytes(g) for g in got[-3:]]
    same_filter(a, c, "the log leaves the filter unchanged")
    close_all(fs)


def test_lineage_with_hash_respawns(gpu_mod):
    from hash_util import hash_config, hash_grid, slope_stream
    n = SIZES[0]
    cfg = hash_config(n, steps=8, bins=20, period=2)
    fs = trio(gpu_mod, cfg, hash_grid(cells=60), init=lambda f: f.init_pose([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]))
    a, b, c = fs
    a.trajectory_enable(8)
    ref = T.TrajectoryLog(8, n)
    h0 = a.rng_state().hash_count
    for k, st in enumerate(slope_stream(7)):
        step_all(fs, ref, st)
        assert_log_equals(a, ref, f"step {k}", capacity=2)
    assert a.rng_state().hash_count == h0 + 7      # every step asked the respawn's counter
    assert_log_equals(a, ref, "the whole log")
    same_filter(a, c, "the log leaves the filter unchanged")
    close_all(fs)


def test_lineage_with_particle_maps(gpu_mod):
    import particle_grid_ref as R
    n = SIZES[0]
    cfg = config(n, A.FLAG_PARTICLE_MAPS)
    cfg.local_map_pages = 48
    grid = R.prior_grid("beyond", 83)
    fs = trio(gpu_mod, cfg, grid, init=lambda f: f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.05], 0.18, 0.05))
    a, b, c = fs
    a.trajectory_enable(8)
    ref = T.TrajectoryLog(8, n)
    scan = S.scan_patches()
    for k, st in enumerate(S.step_stream(6, tilt=True)):
        step_all(fs, ref, st, after=lambda f: f.map_update(scan))
        assert_log_equals(a, ref, f"step {k}", capacity=2)
    assert_log_equals(a, ref, "the whole log")
    same_filter(a, c, "the log leaves the filter unchanged")
    best = a.best_index()
    assert best == c.best_index()
    assert len(a.particle_map(best)[0]) > 0
    assert R.grids_equal(a.particle_grid(best), c.particle_grid(best))
    close_all(fs)


def test_clearing_disabling_and_refusals(gpu_mod):
    n = SIZES[0]
    f = gpu_mod.GpuFilter(config(n))
    f.set_map(S.flat_map(cells=120))
    f.init_gaussian(n, *INIT)
    stream = S.step_stream(4)

    def code(call):
        with pytest.raises(gpu_mod.EslamError) as e:
            call()
        return e.value.code

    # off: info says so, everything else is refused
    assert f.trajectory_info().enabled == 0
    assert code(f.trajectory_clear) == A.ERR_INVALID_ARG
    assert code(lambda: f.trajectories([0], capacity=4)) == A.ERR_INVALID_ARG
    assert code(lambda: f.trajectory_smoothed(capacity=4)) == A.ERR_INVALID_ARG
    assert code(lambda: f.trajectory_enable(0)) == A.ERR_INVALID_ARG
    f.trajectory_disable()                        # idempotent
    f.trajectory_enable(4)
    blob = None
    for what in ("upload", "init_gaussian", "load_state", "clear"):
        f.step(stream[0])
        f.step(stream[1])
        assert f.trajectory_info().entries == 2, what
        if blob is None:
            blob = f.save_state()
        if what == "upload":
            f.upload(f.download())
        elif what == "init_gaussian":
            f.init_gaussian(n, *INIT)
        elif what == "load_state":
            f.load_state(blob)
        else:
            f.trajectory_clear()
        info = f.trajectory_info()
        assert (info.enabled, info.entries, info.capacity_steps, info.max_particles) == (1, 0, 4, n), what
        assert f.trajectories(np.arange(n)).shape == (n, 0) and f.trajectory_smoothed() == [], what
    # ... and the log goes on from the particles as they stand, the step ids counting on
    f.step(stream[2])
    got = f.trajectories(np.arange(n))
    pa = f.download()
    assert got.shape == (n, 1) and np.array_equal(got["slot"][:, 0], np.arange(n)) and got["step"][0, 0] == 8
    assert got["x"][:, 0].tobytes() == pa.x.tobytes() and got["zsigma"][:, 0].tobytes() == pa.zsigma.tobytes()
    # more particles than max_particles: refused, the filter and the log as they were
    assert code(lambda: f.init_gaussian(n + 1, *INIT)) == A.ERR_INVALID_ARG
    assert f.count() == n and f.trajectory_info().entries == 1
    assert code(lambda: f.trajectories([n])) == A.ERR_INVALID_ARG
    assert code(lambda: f.trajectories([0, 2 ** 40])) == A.ERR_INVALID_ARG
    f.trajectory_disable()
    assert f.trajectory_info().as_dict() == dict.fromkeys([k for k, _ in A.TrajectoryInfo._fields_], 0)
    assert code(lambda: f.trajectories([0], capacity=4)) == A.ERR_INVALID_ARG
    f.step(stream[3])                             # and the filter steps on without it
    f.close()


def test_sharded_filters_are_refused(gpu_mod):
    n = 256
    ag = A.ALLGATHER_FN(lambda *a: 1)
    a2a = A.ALLTOALLV_FN(lambda *a: 1)
    comm = A.Comm(None, 0, 1, 0, 0, ag, a2a)
    bounds = (C.c_uint64 * 2)(0, n)
    f = gpu_mod.GpuFilter(config(n))
    f._check(f.L.eslam_gpu_set_comm(f.h, C.byref(comm), n, bounds))
    f.set_map(S.flat_map(cells=120))
    f.init_gaussian(n, *INIT)
    with pytest.raises(gpu_mod.EslamError) as e:
        f.trajectory_enable(4)
    assert e.value.code == A.ERR_UNSUPPORTED and "sharded" in str(e.value)
    assert f.trajectory_info().enabled == 0
    f.close()
    g = gpu_mod.GpuFilter(config(n))
    g.set_map(S.flat_map(cells=120))
    g.init_gaussian(n, *INIT)
    g.trajectory_enable(4)
    assert g.L.eslam_gpu_set_comm(g.h, C.byref(comm), n, bounds) == A.ERR_UNSUPPORTED
    assert b"trajectory" in g.L.eslam_gpu_last_error(g.h)
    assert g.count() == n and g.trajectory_info().enabled == 1     # nothing was dropped
    g.close()
