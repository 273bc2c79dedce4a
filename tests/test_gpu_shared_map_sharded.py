"""processMap's merge into the shared map on a sharded filter (eslam_gpu_shared_map_update_sharded,
DESIGN.md 5c): every rank merges every run of the global particle order into its own copy of the
grid, from the run's poses exchanged between the ranks.  After every merge every rank's grid and
counters equal the sequential reference (tests/c/shared_map_ref.c) applied to the CPU oracle's
particles, bit for bit, and the next step on the merged grid leaves every shard equal to the
oracle's slice -- so the rebuilt cell table, occupancy bits and K1's window are right on every
rank.  The ranks are processes sharing the card (tests/shared_map_dist_worker.py) that meet
through a file store; the expected values are computed here, by the reference alone."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import shared_map_ref as R
import synthetic as S
from test_gpu_shared_map import N, COUNTERS, assert_same_grid, case_grid, case_sigma, counters, u32, wide_scans

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INFO_FIELDS = [f for f, _ in A.SharedMergeInfo._fields_]
RANK_LIMIT = 120                            # seconds a rank may take


def launch(case, n_global, world, tmp, mem, program, tag):
    """Run the ranks once; they meet through a FileStore in `tmp`.  Every rank is under a time
    limit; when one passes it or exits non-zero, all of them are killed."""
    store = os.path.join(tmp, f"store_{tag}")
    if os.path.exists(store):
        os.remove(store)
    procs, outs, logs = [], [], []
    for r in range(world):
        out = os.path.join(tmp, f"{tag}_{r}.npz")
        log = os.path.join(tmp, f"{tag}_{r}.log")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), ESLAM_DIST_STORE=store, OMP_NUM_THREADS="1")
        with open(log, "wb") as lf:
            procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "shared_map_dist_worker.py"), case, str(n_global),
                                           out, mem, json.dumps(program)], env=env, stdout=lf, stderr=subprocess.STDOUT))
        outs.append(out)
        logs.append(log)
    deadline = time.monotonic() + RANK_LIMIT
    pending, failed = set(range(world)), None
    while pending and failed is None:
        for r in sorted(pending):
            try:
                rc = procs[r].wait(timeout=0.05)
            except subprocess.TimeoutExpired:
                continue
            pending.discard(r)
            if rc != 0:
                failed = f"rank {r} exited with {rc}"
                break
        if failed is None and pending and time.monotonic() > deadline:
            failed = f"ranks {sorted(pending)} passed {RANK_LIMIT} s"
    if failed is not None:
        for p in procs:
            p.kill()
        for p in procs:
            p.wait()
        tails = [f"--- rank {r} (exit {p.returncode}) ---\n{open(log, errors='replace').read()[-2500:]}"
                 for r, (p, log) in enumerate(zip(procs, logs))]
        raise AssertionError(failed + "\n" + "\n".join(tails))
    return [dict(np.load(o)) for o in outs]


def scans():
    w = wide_scans()
    return {"s48": S.scan_patches(), "w0": w[0], "w1": w[1], "w2": w[2]}


def runs_of(n, patches, max_records):
    """the one-context formula: whole particles, at most max_records records, at least one particle"""
    lim = min(max_records if max_records else 1 << 21, 1 << 31)
    per = max(1, min(n, lim // patches))
    return -(-n // per)


_expected = {}


def expected(oracle, case, n, program):
    """What the program leaves, by the oracle and the reference alone: per op the oracle's particles
    and, for a merge, the merged grid and the reference's counters (computed once per case, size
    and program; max_records does not enter)."""
    key = (case, n, tuple((op[0], op[1]) for op in program))
    if key in _expected:
        return _expected[key]
    grid = case_grid(case)
    cfg = S.bench_config(A.default_config(), n)
    cfg.flags |= A.FLAG_RECORD_ANCESTORS
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    orc.set_map(grid)
    orc.init_gaussian(n, [0.0, 0.0, 0.0], case_sigma(case), 0.18, 0.05)
    stream, scan = S.step_stream(3, tilt=True), scans()
    cur, want = grid, []
    for op in program:
        e = {}
        if op[0] == "step":
            if cur is not grid:
                orc.set_map(cur)
            e["updated"] = int(orc.step(stream[op[1]]))
            e["anc"] = np.array(orc.ancestors()) if orc.info().resampled else None
        elif op[0] == "merge":
            cur, info = R.merge(cur, orc.download(), scan[op[1]])
            e["info"] = counters(info)
        e["grid"] = cur
        e["particles"] = orc.download()
        want.append(e)
    _expected[key] = want
    return want


def check(parts, want, program, n, label):
    """every rank's records against the expected ones, bit for bit"""
    bounds = [int(b) for b in parts[0]["bounds"]]
    scan = scans()
    for rank, rec in enumerate(parts):
        lo, hi = bounds[rank], bounds[rank + 1]
        for i, (op, e) in enumerate(zip(program, want)):
            where = f"{label} rank {rank} op {i} {op}"
            for fld in A.ParticleArrays.FIELDS:
                got, exp = rec[f"{i}/p/{fld}"], np.array(getattr(e["particles"], fld))[lo:hi]
                assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(exp).view(np.uint8)), (where, fld)
            if op[0] == "step":
                assert int(rec[f"{i}/updated"]) == e["updated"], where
                continue
            g, w = e["grid"], rec
            assert np.array_equal(w[f"{i}/g/cell_start"], g.cell_start), where
            assert np.array_equal(u32(w[f"{i}/g/mean"]), u32(g.mean)), where
            assert np.array_equal(u32(w[f"{i}/g/stdev"]), u32(g.stdev)), where
            assert (f"{i}/g/patch_height" in w) == (g.patch_height is not None), where
            if g.patch_height is not None:
                assert np.array_equal(u32(w[f"{i}/g/patch_height"]), u32(g.patch_height)), where
            if op[0] == "differ":
                assert int(rec[f"{i}/code"]) == A.ERR_INVALID_ARG, where
                continue
            info = dict(zip(INFO_FIELDS, (int(v) for v in rec[f"{i}/info"])))
            print(where, info)
            assert {f: info[f] for f in COUNTERS} == e["info"], where
            assert info["runs"] == runs_of(n, len(scan[op[1]]), op[2]), where
            assert info["particles_done"] == n and info["n_patches"] == g.mean.shape[0], where
    return bounds


def crossings(anc, bounds):
    """outputs of a resample whose ancestor lives in another shard"""
    shard = np.searchsorted(np.array(bounds[1:]), np.arange(len(anc)), side="right")
    return int(np.count_nonzero(shard != shard[np.asarray(anc, dtype=np.int64)]))


SEQUENCE = [["step", 0], ["merge", "s48", 0], ["merge", "w0", 0], ["step", 1], ["merge", "s48", 0], ["merge", "w1", 0], ["step", 2]]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", ["rough_heights", "rotated_grid", "spread"])
def test_sharded_merge_equals_the_reference(oracle, tmp_path, case, world):
    want = expected(oracle, case, N, SEQUENCE)
    parts = launch(case, N, world, str(tmp_path), "host", SEQUENCE, f"seq_{case}_{world}")
    bounds = check(parts, want, SEQUENCE, N, f"{case} world {world}")
    # a no-op cannot pass
    total = {f: sum(e["info"][f] for e in want if "info" in e) for f in COUNTERS}
    assert total["fused"] > 0 and total["inserted"] > 0, total
    assert want[-1]["grid"].mean.shape[0] > case_grid(case).mean.shape[0]
    if case == "rough_heights":
        assert total["absorbed"] > 0, total
        # step 1's resample takes particles across the shard boundaries: the merge after it starts
        # with a migration just behind it
        assert want[3]["anc"] is not None and crossings(want[3]["anc"], bounds) > 0
    if case == "spread":
        assert total["patches_off_grid"] > 0, total
    else:
        assert total["patches_off_grid"] == 0, total


@pytest.mark.parametrize("n,max_records", [(N, 0), (N, 7 * 48), (N, 1664 * 48), (200, 40)])
def test_runs_against_the_shard_boundaries(oracle, tmp_path, n, max_records):
    """one run spanning all ranks; runs of 7 particles straddling both boundaries (neither is a
    multiple of 7); run ends exactly on the shard ends; and one particle per run, so most ranks
    contribute nothing to a given run"""
    program = [["step", 0], ["merge", "s48", max_records], ["merge", "w2", max_records]]
    want = expected(oracle, "rough", n, program)
    parts = launch("rough", n, 3, str(tmp_path), "host", program, f"runs_{n}_{max_records}")
    bounds = check(parts, want, program, n, f"runs n {n} max_records {max_records}")
    assert bounds == ([0, 1664, 3328, 5003] if n == N else [0, 64, 128, 200])
    assert all(b % 7 for b in bounds[1:3])
    assert want[1]["info"]["fused"] > 0 and want[2]["info"]["inserted"] > 0
    runs = [int(parts[0][f"{i}/info"][INFO_FIELDS.index("runs")]) for i in (1, 2)]
    assert runs == {(N, 0): [1, 1], (N, 7 * 48): [715, 1668], (N, 1664 * 48): [4, 7], (200, 40): [200, 200]}[(n, max_records)]


@pytest.mark.parametrize("mem", ["device", "rccl"])
def test_device_memory_one_rank(oracle, tmp_path, mem):
    """torch's device-memory callbacks and the library's own RCCL, one rank each (RCCL cannot host
    two ranks on one device)"""
    program = [[op[0], op[1]] + ([7 * 48] if op[0] == "merge" else []) for op in SEQUENCE[:4]]
    want = expected(oracle, "rough_heights", N, program)
    parts = launch("rough_heights", N, 1, str(tmp_path), mem, program, f"dev_{mem}")
    check(parts, want, program, N, mem)


def test_ranks_that_disagree(oracle, tmp_path):
    """rank 1 passes another scan: both ranks are refused with the grid untouched, and the same
    scan on both then merges -- nothing hung or lost its place"""
    program = [["step", 0], ["differ", "s48", 0], ["merge", "s48", 0]]
    want = expected(oracle, "rough_heights", N, program)
    assert want[1]["grid"] is want[0]["grid"]
    parts = launch("rough_heights", N, 2, str(tmp_path), "host", program, "differ")
    check(parts, want, program, N, "differ")
    assert want[2]["info"]["fused"] > 0


def failing_comm_filter(gpu_mod, n, flags=0):
    """a world-size-1 eslam_gpu_set_comm filter whose collectives fail"""
    cfg = S.bench_config(A.default_config(), n)
    cfg.flags |= flags
    f = gpu_mod.GpuFilter(cfg)
    f._callbacks = (A.ALLGATHER_FN(lambda *a: 1), A.ALLTOALLV_FN(lambda *a: 1))
    comm = A.Comm(None, 0, 1, 0, 0, *f._callbacks)
    bounds = (C.c_uint64 * 2)(0, n)
    f._check(f.L.eslam_gpu_set_comm(f.h, C.byref(comm), n, bounds))
    return f


def test_refusals_before_any_collective(gpu_mod):
    """every check of the plain call comes first, with its code; the first collective (which
    fails here) is reached only by a valid call, and leaves the grid alone"""
    n, grid, scan = 256, case_grid("flat"), S.scan_patches()

    def code(f, patches=scan, call="shared_map_update_sharded"):
        with pytest.raises(gpu_mod.EslamError) as e:
            getattr(f, call)(patches)
        return e.value.code

    f = failing_comm_filter(gpu_mod, n, A.FLAG_PARTICLE_MAPS)
    f.set_map(grid)
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.05], 0.18, 0.05)
    assert code(f) == A.ERR_INVALID_ARG
    f.close()
    f = failing_comm_filter(gpu_mod, n)
    assert code(f) == A.ERR_NO_ENVIRONMENT
    f.set_map(grid)
    assert code(f) == A.ERR_NOT_INITIALISED
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.05], 0.18, 0.05)
    bad = S.scan_patches()
    bad[17].position[2] = float("nan")
    assert code(f, bad) == A.ERR_INVALID_ARG
    assert code(f) == A.ERR_COMM
    assert_same_grid(f.get_map(), grid, "a failed collective")
    assert code(f, call="shared_map_update") == A.ERR_UNSUPPORTED
    f.close()


def test_unsharded_is_the_plain_call(gpu_mod):
    grid, st = case_grid("rough"), S.step_stream(1, tilt=True)[0]
    got = []
    for call in ("shared_map_update", "shared_map_update_sharded"):
        cfg = S.bench_config(A.default_config(), N)
        f = gpu_mod.GpuFilter(cfg)
        f.set_map(grid)
        f.init_gaussian(N, [0.0, 0.0, 0.0], case_sigma("rough"), 0.18, 0.05)
        f.step(st)
        infos = [getattr(f, call)(scan, 7 * 48) for scan in (S.scan_patches(), wide_scans()[2])]
        got.append((f.get_map(), [[int(getattr(i, fld)) for fld in INFO_FIELDS] for i in infos]))
        f.close()
    assert_same_grid(got[1][0], got[0][0], "unsharded")
    assert got[1][1] == got[0][1]
    assert got[0][1][0][INFO_FIELDS.index("runs")] == 715 and got[0][1][0][INFO_FIELDS.index("fused")] > 0


def test_cpp_facade_shared_map_sharded():
    """EmbodiedSlamFilter::processMap(scan, true, true) and the camera update on a sharded estimator
    == the unsharded filter"""
    sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
    import build_lib
    exe = build_lib.build_facade_test(verbose=False, name="test_facade_shared_map_sharded")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade shared map sharded OK" in r.stdout
