"""The trajectory log of a sharded filter (eslam_gpu_trajectory_enable_sharded; DESIGN.md 5j
"Sharded") against code that existed before it: ONE context holding all the particles with the
one-GPU log, driven by the same scenario function (tests/trajectory_shard_scenarios.run).

World sizes 1, 2 and 3, gloo ranks sharing the GPU (tests/trajectory_dist_worker.py), one launch
per world size shared by the tests.  After every phase every rank's trajectory_info, lineages
(of particles at the ends, on both sides of every shard boundary, the best one and a repeat;
the newest two entries and all) and smoothed trajectory equal the one context's byte for byte:
no case is left out and no tolerance applies.  The filter's particles with the log on equal those
of a sharded run with the log off, and the one context's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eslam_abi as A
import trajectory_shard_scenarios as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = 56                                        # sizeof(eslam_trajectory_pose)


def launch(tmp, world, timeout=240):
    """the ranks of one world size; a timeout kills them all"""
    store = os.path.join(tmp, "store")
    procs, outs = [], []
    for r in range(world):
        out = os.path.join(tmp, f"rank{r}.npz")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), ESLAM_DIST_STORE=store, OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "trajectory_dist_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        outs.append(out)
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    bad = [f"--- rank {r} (exit {p.returncode}) ---\n{log[-2500:]}" for r, (p, log) in enumerate(zip(procs, logs)) if p.returncode]
    assert not bad, "\n".join(bad)
    return [dict(np.load(o)) for o in outs]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    cache = {}

    def get(world):
        if world not in cache:
            cache[world] = launch(str(tmp_path_factory.mktemp(f"w{world}")), world)
        return cache[world]
    return get


@pytest.fixture(scope="module")
def single(gpu_mod):
    """the scenario on one unsharded context with the one-GPU log (computed once, never changed)"""
    rec = {}
    f = gpu_mod.GpuFilter(T.config())
    T.run(rec, f, 0, T.N, False)
    f.close()
    return rec


def test_the_one_context_scenario_is_not_trivial(single):
    """what the sharded runs are compared with: the ring wrapped, the entries hold three counts,
    the lineages coalesce and, in the last phase, converge on one ancestor"""
    n_b = int(single["b/n"][0])
    # the multinomial call keeps the draws below the weight sum; three ranks need more than two chunks
    assert 128 < n_b <= 900 and int(single["c/n"][0]) == T.GROWN
    assert single["a/info"].tolist() == [1, T.CAPACITY, 4, 0, 3, T.N]
    assert single["b/info"].tolist() == [1, T.CAPACITY, 4, 1, 4, n_b]
    assert single["c/info"].tolist() == [1, T.CAPACITY, 4, 3, 6, T.GROWN]
    assert single["d/info"].tolist() == [1, T.CAPACITY, 4, 4, 7, T.GROWN]
    nodes = np.frombuffer(single["c/all"].tobytes(), dtype=gpu_node_dtype()).reshape(-1, T.CAPACITY)
    assert nodes["particles"][0].tolist() == [T.N, n_b, T.GROWN, T.GROWN]          # records 3 .. 6: three counts
    nodes = np.frombuffer(single["b/all"].tobytes(), dtype=gpu_node_dtype()).reshape(-1, T.CAPACITY)
    assert nodes["particles"][0].tolist() == [T.N, T.N, T.N, n_b]
    # after the multinomial call the link is no identity: the leaves' newest slots are not the leaves
    nodes = np.frombuffer(single["b0/all"].tobytes(), dtype=gpu_node_dtype()).reshape(-1, T.CAPACITY)
    assert not np.array_equal(nodes["slot"][:, -1], single["b0/leaves"])
    # a repeated leaf, the same lineage
    assert nodes[-1].tobytes() == nodes[2].tobytes()
    d = single["a/distinct"].tolist()
    # records 2 and 3 did not resample: their parents are the identity; record 1 did
    assert d[1:] == [T.N] * 3 and 1 < d[0] < T.N
    # phase d: every lineage goes through the one particle that held all the weight
    d = single["d/distinct"].tolist()
    assert d[-1] == T.GROWN and d[:-1] == [1, 1, 1]
    nodes = np.frombuffer(single["d/all"].tobytes(), dtype=gpu_node_dtype()).reshape(-1, T.CAPACITY)
    assert set(nodes["slot"][:, -2].tolist()) == {T.GROWN - 3}


def gpu_node_dtype():
    import eslam_amd
    assert eslam_amd.GpuFilter.TRAJECTORY_NODE.itemsize == NODE
    return eslam_amd.GpuFilter.TRAJECTORY_NODE


@pytest.mark.parametrize("world", T.WORLDS)
@pytest.mark.parametrize("phase", T.PHASES)
def test_every_rank_answers_as_the_one_context(ranks, single, world, phase):
    parts = ranks(world)
    for r, p in enumerate(parts):
        assert int(p[f"on/{phase}/n"][0]) == int(single[f"{phase}/n"][0]), r
        for what in ("info", "leaves", "two", "all", "smoothed"):
            got, want = p[f"on/{phase}/{what}"], single[f"{phase}/{what}"]
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (phase, what, r)
    if phase == "c":
        # the leaves sit on both sides of this world's shard boundaries, in the table of the grown filter
        table = A.shard_bounds(T.GROWN, world)
        lv = single["c/leaves"].tolist()
        assert all(b - 1 in lv and b in lv for b in table[1:-1])


@pytest.mark.parametrize("world", T.WORLDS)
def test_the_log_leaves_the_filter_unchanged(ranks, single, world):
    parts = ranks(world)
    for phase in T.PHASES:
        for fld in A.ParticleArrays.FIELDS:
            on = np.concatenate([p[f"on/{phase}/{fld}"] for p in parts])
            off = np.concatenate([p[f"off/{phase}/{fld}"] for p in parts])
            assert on.tobytes() == off.tobytes(), (phase, fld)
            assert on.tobytes() == single[f"{phase}/{fld}"].tobytes(), (phase, fld)


@pytest.mark.parametrize("world", T.WORLDS)
def test_refusals_mismatches_and_the_ranks_own_figures(ranks, world):
    parts = ranks(world)
    many = world > 1
    for r, p in enumerate(parts):
        code = lambda k: int(p["code/" + k][0])                     # noqa: E731
        # refused before any collective (rank 0 asked alone)
        for k in ("off", "capacity0", "index", "too_many"):
            assert code(k) == A.ERR_INVALID_ARG, (k, r)
        # the ranks asked together with different arguments: every rank refuses (one rank has nobody to differ from)
        for k in ("capacity_differs", "leaves_differ", "counts_differ"):
            assert code(k) == (A.ERR_INVALID_ARG if many else 0), (k, r)
        assert code("enabled_after_mismatch") == (0 if many else 1)
        table = A.shard_bounds(T.N, world)
        assert code("count_after") == table[r + 1] - table[r]       # the refused resample changed nothing
        maxp, nbytes = p["on/max_particles"].tolist()
        assert maxp == T.MAX_PARTICLES[world] and nbytes >= T.CAPACITY * 44 * maxp + 8 * maxp
        assert p["on/cleared"].tolist() == [0, 0]
