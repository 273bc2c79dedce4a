"""eslam_gpu_resample_stratified_sharded / _multinomial_sharded: a filter sharded over gloo ranks
that share the GPU resamples to any count, and the ranks' shards in rank order are bit for bit
the particle set ONE unsharded context has after the plain call (every field, the ancestors, the
info, the minstd state), laid out by the canonical shard table of the new count.

Yardsticks: the CPU reference tests/resample_ref.py gives the expected ancestors, the draws
beyond the sum and the new minstd state; one unsharded GpuFilter running the same scenario code
(resample_sharded_dist_worker.run) gives the expected fields.  Every comparison is on bytes.
One worker launch per world size runs all its scenarios, a fresh filter each."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eslam_abi as A
import resample_ref as R
import resample_sharded_dist_worker as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PART_FIELDS = tuple(A.ParticleArrays.FIELDS) + ("anc",)


def launch(tmp, world, mem="host", timeout=300):
    """the ranks of one world size; a timeout kills them all"""
    store = os.path.join(tmp, f"store_{world}_{mem}")
    procs, outs = [], []
    for r in range(world):
        out = os.path.join(tmp, f"rank_{world}_{mem}_{r}.npz")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), ESLAM_DIST_STORE=store, OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "resample_sharded_dist_worker.py"), out, mem], env=env,
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
    """the workers' records, one launch per world size, shared by the tests"""
    cache = {}

    def get(world, mem="host"):
        if (world, mem) not in cache:
            cache[(world, mem)] = launch(str(tmp_path_factory.mktemp(f"w{world}{mem}")), world, mem)
        return cache[(world, mem)]
    return get


@pytest.fixture(scope="module")
def single(gpu_mod):
    """the same scenario on one unsharded context (computed once per scenario, never changed)"""
    cache = {}

    def get(sc):
        if sc[0] not in cache:
            rec = {}
            f = gpu_mod.GpuFilter(W.config(sc[2]))
            W.run(rec, f, sc, 0, W.N, False)
            f.close()
            cache[sc[0]] = rec
        return cache[sc[0]]
    return get


def scenario(world, name, mem="host"):
    return next(sc for sc in W.scenarios(world, mem) if sc[0] == name)


def owners(bounds, idx):
    return np.searchsorted(np.asarray(bounds, dtype=np.int64), np.asarray(idx, dtype=np.int64), side="right") - 1


def reference(wname, kind, samples, x0=None):
    """the CPU reference's ancestors, draws beyond the sum and new minstd state"""
    w = W.weights(wname)
    import math
    x0 = R.minstd_seed(42) if x0 is None else x0
    fn = R.multinomial if kind == "multinomial" else R.stratified
    return fn(w, samples, x0, R.shift_of(math.fsum(w)))


def moves(world, wname, kind, samples):
    """(source rank, destination rank) of every output, from the reference"""
    anc, _, _ = reference(wname, kind, samples)
    src = owners(A.shard_bounds(W.N, world), anc)
    dst = owners(A.shard_bounds(len(anc), world), np.arange(len(anc)))
    return src, dst


def assert_op_equal(parts, want, key, world, label):
    """the ranks' records of one operation against the one context's"""
    n_after = int(want[f"{key}/count"][0])
    table = A.shard_bounds(n_after, world)
    for r, p in enumerate(parts):
        assert p[f"{key}/bounds"].tolist() == table, (label, r)
        assert int(p[f"{key}/count"][0]) == table[r + 1] - table[r], (label, r)
        assert int(p[f"{key}/rng"][0]) == int(want[f"{key}/rng"][0]), (label, r)
        if f"{key}/info" in want:
            assert np.array_equal(p[f"{key}/info"].view(np.uint8), want[f"{key}/info"].view(np.uint8)), (label, r)
    for fld in PART_FIELDS:
        if f"{key}/{fld}" not in want:
            continue
        got = np.concatenate([p[f"{key}/{fld}"] for p in parts])
        assert np.array_equal(got.view(np.uint8), want[f"{key}/{fld}"].view(np.uint8)), (label, fld)


def check_against_reference(want, key, wname, kind, samples, label):
    """the one context's own result against the CPU reference: ancestors, info, minstd state"""
    anc, beyond, x1 = reference(wname, kind, samples)
    multi = kind == "multinomial"
    assert want[f"{key}/info"].tolist() == [W.N, len(anc), 0 if multi else beyond, beyond if multi else 0], label
    assert int(want[f"{key}/rng"][0]) == x1, label
    assert np.array_equal(want[f"{key}/anc"], anc), label
    return anc, beyond


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("kind", W.KINDS)
def test_counts(ranks, single, world, kind):
    """3000 -> 129, 130, 2999, 3001, 7001: 129 on 3 ranks leaves the last rank one particle; 7001
    crosses the 2048 tile in particles and draws and exceeds every rank's capacity.  In every case
    outputs land on a rank other than their ancestor's."""
    pairs = set()
    for samples in W.COUNTS:
        sc = scenario(world, f"count_{kind}_{samples}")
        src, dst = moves(world, "base", kind, samples)
        assert (src != dst).any(), (kind, samples)
        pairs |= set(zip(src.tolist(), dst.tolist()))
        want = single(sc)
        check_against_reference(want, sc[0] + "/0", "base", kind, samples, sc[0])
        assert_op_equal(ranks(world), want, sc[0] + "/0", world, sc[0])
    if kind == "multinomial":
        assert pairs == {(s, d) for s in range(world) for d in range(world)}
    if world == 3:
        assert A.shard_bounds(129, 3) == [0, 64, 128, 129]
    assert max(np.diff(A.shard_bounds(7001, world))) > max(np.diff(A.shard_bounds(W.N, world)))


def test_unnormalised_weights(ranks, single):
    world = 3
    # x 2: toward higher ranks; the last rank's particles are never drawn
    src, dst = moves(world, "x2", "stratified", 3001)
    pairs = set(zip(src.tolist(), dst.tolist()))
    assert (0, 1) in pairs and (1, 2) in pairs and 2 not in set(src.tolist())
    sc = scenario(world, "x2_stratified")
    check_against_reference(single(sc), sc[0] + "/0", "x2", "stratified", 3001, sc[0])
    assert_op_equal(ranks(world), single(sc), sc[0] + "/0", world, sc[0])
    # x 0.5, stratified: 1501 overruns, all the last global particle's
    sc = scenario(world, "x0.5_stratified")
    anc, beyond = check_against_reference(single(sc), sc[0] + "/0", "x0.5", "stratified", 3001, sc[0])
    assert beyond == 1501 and (anc[-1501:] == W.N - 1).all()
    assert_op_equal(ranks(world), single(sc), sc[0] + "/0", world, sc[0])
    assert all(int(p[sc[0] + "/0/info"][2]) == 1501 for p in ranks(world))
    # x 0.5, multinomial: 1473 dropped
    sc = scenario(world, "x0.5_multinomial")
    anc, beyond = check_against_reference(single(sc), sc[0] + "/0", "x0.5", "multinomial", 3001, sc[0])
    assert beyond == 1473 and len(anc) == 1528 and A.shard_bounds(1528, 3) == [0, 512, 1024, 1528]
    assert_op_equal(ranks(world), single(sc), sc[0] + "/0", world, sc[0])
    for p in ranks(world):
        assert (p[sc[0] + "/0/weight"] == 1.0 / 3000).all()


@pytest.mark.parametrize("kind", W.KINDS)
def test_zero_weight_rank_and_single_survivor(ranks, single, kind):
    world = 3
    assert A.shard_bounds(W.N, 3)[1:3] == [960, 1984]
    src, _ = moves(world, "zero_mid", kind, 4000)
    assert 1 not in set(src.tolist()) and {0, 2} <= set(src.tolist())
    anc, _, _ = reference("single", kind, 4000)
    assert len(anc) > 0 and (anc == W.N - 1).all()
    for wname in ("zero_mid", "single"):
        sc = scenario(world, f"{wname}_{kind}")
        check_against_reference(single(sc), sc[0] + "/0", wname, kind, 4000, sc[0])
        assert_op_equal(ranks(world), single(sc), sc[0] + "/0", world, sc[0])


@pytest.mark.parametrize("kind", W.KINDS)
def test_chunk_rows_change(ranks, single, kind):
    """3000 -> 330000 -> 3000: the summation chunk goes from one row to two and back"""
    world = 2
    assert A.chunk_rows(327680) == 1 and A.chunk_rows(327681) == 2
    assert A.shard_bounds(330000, 2) == [0, 164992, 330000]
    sc = scenario(world, f"rows_{kind}")
    want = single(sc)
    check_against_reference(want, sc[0] + "/0", "base", kind, 330000, sc[0])
    n1 = int(want[sc[0] + "/0/count"][0])
    assert A.chunk_rows(n1) == 2 and A.chunk_rows(int(want[sc[0] + "/1/count"][0])) == 1
    assert n1 == 330000 or kind == "multinomial"
    for i in (0, 1):
        assert_op_equal(ranks(world), want, f"{sc[0]}/{i}", world, f"{sc[0]} op {i}")


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["after_stratified", "after_multinomial", "after_step_first"])
def test_the_filter_afterwards(ranks, single, world, name):
    """two forced-resample steps after the call (after_step_first: also one right before it, whose
    deferred exchange the call settles), then the sum, the best index, a 3-component mixture and
    the centroid: every rank answers as the one context, and holds its slice of its particles"""
    sc = scenario(world, name)
    want = single(sc)
    parts = ranks(world)
    last = len(sc[4]) - 1
    for i, op in enumerate(sc[4]):
        if op[0] in W.KINDS:
            assert_op_equal(parts, want, f"{name}/{i}", world, f"{name} op {i}")
    key = f"{name}/{last}"
    assert want[f"{key}/info"][3] == 1.0                  # the last step resampled, at the new count
    assert_op_equal(parts, want, key, world, f"{name} after")
    assert_op_equal(parts, want, key + "c", world, f"{name} after the centroid")
    for p in parts:
        for what in ("sum", "best", "gmm", "centroid"):
            assert np.array_equal(p[f"{key}/{what}"].view(np.uint8), want[f"{key}/{what}"].view(np.uint8)), what


def test_refusals(ranks, single):
    """refused before any collective (one rank asks before the barrier, the other after it: a call
    that entered a collective would hang until the launch's timeout), nothing changed"""
    world = 2
    parts = ranks(world)
    table = A.shard_bounds(W.N, world)
    for name in ("refuse_args", "refuse_maps"):
        sc = scenario(world, name)
        full = W.global_particles(sc[1])
        for i, op in enumerate(sc[4]):
            key = f"{name}/{i}"
            code = A.ERR_UNSUPPORTED if name == "refuse_maps" else A.ERR_INVALID_ARG
            for r, p in enumerate(parts):
                assert p[f"{key}/code"].tolist() == [code], (key, r)
                assert p[f"{key}/bounds"].tolist() == table and int(p[f"{key}/rng"][0]) == R.minstd_seed(42), (key, r)
            for fld in A.ParticleArrays.FIELDS:
                got = np.concatenate([p[f"{key}/{fld}"] for p in parts])
                assert np.array_equal(got.view(np.uint8), getattr(full, fld).view(np.uint8)), (key, fld)
    # weights x 0.01: the reference keeps 35 draws of 3001, fewer than the 65 two ranks need
    anc, beyond, _ = reference("x0.01", "multinomial", 3001)
    assert len(anc) == 35 and beyond == 3001 - 35
    with pytest.raises(ValueError):
        A.shard_bounds(35, 2)
    sc = scenario(world, "refuse_kept")
    full = W.global_particles("x0.01")
    key = "refuse_kept/0"
    for r, p in enumerate(parts):
        assert p[f"{key}/code"].tolist() == [A.ERR_INVALID_ARG]
        assert p[f"{key}/bounds"].tolist() == table and int(p[f"{key}/rng"][0]) == R.minstd_seed(42)
        assert int(p[f"{key}/count"][0]) == table[r + 1] - table[r]
    for fld in A.ParticleArrays.FIELDS:
        got = np.concatenate([p[f"{key}/{fld}"] for p in parts])
        assert np.array_equal(got.view(np.uint8), getattr(full, fld).view(np.uint8)), fld
    # the one context makes only the stratified call (its multinomial one would keep the 35)
    one = {}
    ref_sc = (sc[0], sc[1], sc[2], sc[3], [("stratified", 3001)])
    f_rec = single(("refuse_kept_ref",) + ref_sc[1:])
    for k, v in f_rec.items():
        one[k.replace("refuse_kept_ref/0", "refuse_kept/1")] = v
    check_against_reference(one, "refuse_kept/1", "x0.01", "stratified", 3001, "after the refusal")
    assert_op_equal(parts, one, "refuse_kept/1", world, "stratified after the refused multinomial")


def test_one_rank_over_the_librarys_rccl(ranks, single):
    """RcclShardedGpuFilter on one rank: the exchanges run through RCCL on device buffers to the
    rank itself.  More than one RCCL rank cannot run on a box with one GPU, so the
    exchange between RCCL ranks is covered only as far as the callbacks' contract is the same."""
    parts = ranks(1, "rccl")
    for sc in W.scenarios(1, "rccl"):
        want = single(sc)
        kind, samples = sc[4][0]
        check_against_reference(want, sc[0] + "/0", "base", kind, samples, sc[0])
        assert_op_equal(parts, want, sc[0] + "/0", 1, sc[0])
