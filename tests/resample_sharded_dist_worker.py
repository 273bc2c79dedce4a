"""One rank of tests/test_gpu_resample_sharded.py: eslam_gpu_resample_stratified_sharded /
_multinomial_sharded on a filter sharded over the ranks, which share one GPU.

    RANK=r WORLD_SIZE=w ESLAM_DIST_STORE=file python tests/resample_sharded_dist_worker.py OUT.npz [host|rccl]

One launch runs every scenario of its world size in sequence, a fresh filter each (scenarios()).
run() is the same code the test runs on ONE unsharded context for the expected values: it only
picks the sharded or the plain call.  What a rank saves per scenario: after every operation its
particles, ancestors, the info, the minstd state, its count and the shard table; after a refused
call its code.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "slam-eslam_amd"))

import numpy as np  # noqa: E402

N = 3000
COUNTS = (129, 130, 2999, 3001, 7001)
KINDS = ("stratified", "multinomial")
STEP_CAP = 1 << 20                               # minEffective above every count: every update resamples


def weights(name):
    """the base weights (concentrated: ancestors cross the ranks) and their variants"""
    w = np.random.default_rng(N).uniform(size=N) ** 6
    w /= w.sum()
    if name == "base":
        return w
    if name.startswith("x"):
        return w * float(name[1:])
    if name == "zero_mid":                       # the middle shard of 3 ranks holds no weight
        w[960:1984] = 0.0
        return w / w.sum()
    if name == "single":                         # all the weight on the last global particle
        w[:] = 0.0
        w[N - 1] = 1.0
        return w
    raise ValueError(name)


def global_particles(name):
    from test_resample_ref import particles
    return particles(weights(name))


def scenarios(world, mem="host"):
    """(name, weights, flags, with a map, operations).  An operation: (kind, samples) a resample
    expected to succeed; ("refuse", kind, samples, staggered) one expected to fail; ("step", k)
    step k of the stream; ("after",) the later calls at the new count."""
    import eslam_abi as A
    out = []
    if mem == "rccl":
        return [("rccl_stratified_7001", "base", 0, False, [("stratified", 7001)]),
                ("rccl_multinomial_129", "base", 0, False, [("multinomial", 129)])]
    for kind in KINDS:
        for samples in COUNTS:
            out.append((f"count_{kind}_{samples}", "base", 0, False, [(kind, samples)]))
    if world == 3:
        out.append(("x2_stratified", "x2", 0, False, [("stratified", 3001)]))
        out.append(("x0.5_stratified", "x0.5", 0, False, [("stratified", 3001)]))
        out.append(("x0.5_multinomial", "x0.5", 0, False, [("multinomial", 3001)]))
        for kind in KINDS:
            out.append((f"zero_mid_{kind}", "zero_mid", 0, False, [(kind, 4000)]))
            out.append((f"single_{kind}", "single", 0, False, [(kind, 4000)]))
    if world == 2:
        for kind in KINDS:
            out.append((f"rows_{kind}", "base", 0, False, [(kind, 330000), (kind, N)]))
    out.append(("after_stratified", "base", 0, True, [("stratified", 3001), ("step", 0), ("step", 1), ("after",)]))
    out.append(("after_multinomial", "base", 0, True, [("multinomial", 2999), ("step", 0), ("step", 1), ("after",)]))
    out.append(("after_step_first", "base", 0, True, [("step", 0), ("stratified", 3001), ("step", 1), ("step", 2), ("after",)]))
    if world == 2:
        ops = []
        for kind in KINDS:
            ops += [("refuse", kind, 0, True), ("refuse", kind, 2 ** 30, True)]
        ops.append(("refuse", "stratified", 64, True))
        out.append(("refuse_args", "base", 0, False, ops))
        out.append(("refuse_maps", "base", A.FLAG_PARTICLE_MAPS, True,
                    [("refuse", "stratified", 3001, True), ("refuse", "multinomial", 3001, True)]))
        out.append(("refuse_kept", "x0.01", 0, False, [("refuse", "multinomial", 3001, False), ("stratified", 3001)]))
    return out


def config(flags):
    import eslam_abi as A
    import synthetic as S
    cfg = S.bench_config(A.default_config(), STEP_CAP)
    cfg.particle_count = N
    cfg.flags |= A.FLAG_RECORD_ANCESTORS | flags
    return cfg


def snap(rec, key, f, bounds):
    import eslam_abi as A
    pa = f.download()
    for fld in A.ParticleArrays.FIELDS:
        rec[f"{key}/{fld}"] = np.array(getattr(pa, fld))
    rec[f"{key}/count"] = np.array([f.count()], dtype=np.uint64)
    rec[f"{key}/rng"] = np.array([f.rng_state().minstd_x], dtype=np.uint64)
    rec[f"{key}/bounds"] = np.array(bounds, dtype=np.uint64)


def run(rec, f, sc, lo, hi, sharded, barrier=None, rank=0):
    """one scenario on filter f holding particles [lo, hi) of the scenario's global set"""
    import eslam_abi as A
    import eslam_amd
    import synthetic as S
    name, wname, flags, with_map, ops = sc
    if with_map:
        f.set_map(S.flat_map(cells=100))
    full = global_particles(wname)
    pa = A.ParticleArrays(hi - lo)
    for fld in A.ParticleArrays.FIELDS:
        getattr(pa, fld)[:] = getattr(full, fld)[lo:hi]
    f.upload(pa)
    stream = S.step_stream(3)
    bounds = lambda: f.get_shard_bounds() if sharded else [0, f.count()]    # noqa: E731

    def call(kind, samples):
        if sharded:
            return (f.resample_multinomial_sharded if kind == "multinomial" else f.resample_stratified_sharded)(samples)
        return (f.resample_multinomial if kind == "multinomial" else f.resample_stratified)(samples)

    for i, op in enumerate(ops):
        key = f"{name}/{i}"
        if op[0] == "refuse":
            _, kind, samples, staggered = op
            # rank 0 asks after the barrier, the others before it: a call that entered a collective would hang
            if staggered and barrier and rank == 0:
                barrier()
            try:
                call(kind, samples)
                code = 0
            except eslam_amd.EslamError as e:
                code = e.code
            if staggered and barrier and rank != 0:
                barrier()
            rec[f"{key}/code"] = np.array([code])
            snap(rec, key, f, bounds())
        elif op[0] == "step":
            f.step(stream[op[1]])
        elif op[0] == "after":
            info = f.sync()
            rec[f"{key}/info"] = np.array([info.effective, info.weight_sum, info.max_weight, float(info.resampled)])
            snap(rec, key, f, bounds())
            rec[f"{key}/anc"] = np.array(f.ancestors())
            rec[f"{key}/sum"] = np.array([f.weights_sum()])
            rec[f"{key}/best"] = np.array([f.best_index()], dtype=np.uint64)
            wts, means, covs, _ = f.fit_pose_gmm(3)
            rec[f"{key}/gmm"] = np.concatenate([wts, means.ravel(), covs.ravel()])
            pos, quat = f.centroid()                       # normalises in place: last
            rec[f"{key}/centroid"] = np.array(list(pos) + list(quat))
            snap(rec, key + "c", f, bounds())
        else:
            kind, samples = op
            info = call(kind, samples)
            rec[f"{key}/info"] = np.array([info.n_before, info.n_after, info.overruns, info.dropped], dtype=np.uint64)
            snap(rec, key, f, bounds())
            rec[f"{key}/anc"] = np.array(f.ancestors())


def main():
    out = sys.argv[1]
    mem = sys.argv[2] if len(sys.argv) > 2 else "host"
    import torch
    import torch.distributed as dist
    import eslam_abi as A
    import eslam_dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    init = dict(init_method="file://" + os.environ["ESLAM_DIST_STORE"], rank=rank, world_size=world)
    if mem == "rccl":
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", **init)
    else:
        dist.init_process_group("gloo", **init)
    comm = eslam_dist.TorchComm(device_memory=False) if mem == "host" else None
    rec = {}
    for sc in scenarios(world, mem):
        cfg = config(sc[2])
        if mem == "rccl":
            f = eslam_dist.RcclShardedGpuFilter(cfg, N, rank, world, device=0)
        else:
            f = eslam_dist.ShardedGpuFilter(cfg, N, comm, device=0)
        assert f.bounds == A.shard_bounds(N, world)
        run(rec, f, sc, f.bounds[rank], f.bounds[rank + 1], True, barrier=dist.barrier, rank=rank)
        # the wrapper's attributes follow the context's table
        assert f.bounds == f.get_shard_bounds() and f.n_global == f.bounds[-1]
        assert (f.gbase, f.n_local) == (f.bounds[rank], f.bounds[rank + 1] - f.bounds[rank]) and f.count() == f.n_local
        f.close()
        if comm is not None and comm.error is not None:
            raise comm.error
    np.savez(out, **rec)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
