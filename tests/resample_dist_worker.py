"""One gloo rank of tests/test_gpu_resample_counts.py's sharded test: the calls a sharded filter
refuses (before any collective: a rank that blocked would hang its peer), then the stratified
resample to n_global, and what the rank holds afterwards.

    RANK=r WORLD_SIZE=w ESLAM_DIST_STORE=file python tests/resample_dist_worker.py N_GLOBAL OUT.npz [maps]

With `maps` the filter has per-particle maps (ESLAM_FLAG_PARTICLE_MAPS) and a map: its capacity is
the shard's, below n_global, and the stratified call to n_global is still the sharded resample.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "slam-eslam_amd"))

import numpy as np  # noqa: E402


def shard_particles(n_global, lo, hi):
    """particles [lo, hi) of the test's n_global (concentrated weights: ancestors cross the ranks)"""
    import eslam_abi as A
    from test_resample_ref import particles
    w = np.random.default_rng(n_global).uniform(size=n_global) ** 6
    full = particles(w / w.sum())
    pa = A.ParticleArrays(hi - lo)
    for f in A.ParticleArrays.FIELDS:
        getattr(pa, f)[:] = getattr(full, f)[lo:hi]
    return pa


def main():
    n_global, out = int(sys.argv[1]), sys.argv[2]
    maps = len(sys.argv) > 3 and sys.argv[3] == "maps"
    import torch.distributed as dist
    import eslam_abi as A
    import eslam_amd
    import eslam_dist
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo", init_method="file://" + os.environ["ESLAM_DIST_STORE"], rank=rank,
                            world_size=int(os.environ["WORLD_SIZE"]))
    comm = eslam_dist.TorchComm(device_memory=False)
    cfg = A.default_config()
    cfg.flags |= A.FLAG_RECORD_ANCESTORS | (A.FLAG_PARTICLE_MAPS if maps else 0)
    f = eslam_dist.ShardedGpuFilter(cfg, n_global, comm, device=0)
    if maps:
        import synthetic as S
        f.set_map(S.flat_map(cells=60))
    lo, hi = f.bounds[rank], f.bounds[rank + 1]
    f.upload(shard_particles(n_global, lo, hi))
    codes = []
    # rank 1 asks first and rank 0 after a barrier, so a call that entered a collective would hang
    calls = [(f.resample_multinomial, n_global), (f.resample_stratified, n_global - 1), (f.resample_multinomial, 10)]
    for call, samples in calls:
        if rank == 0:
            dist.barrier()
        try:
            call(samples)
            codes.append(0)
        except eslam_amd.EslamError as e:
            codes.append(e.code)
        if rank != 0:
            dist.barrier()
    info = f.resample_stratified(n_global)
    pa = f.download()
    rec = {fld: np.array(getattr(pa, fld)) for fld in A.ParticleArrays.FIELDS}
    rec["anc"] = np.array(f.ancestors())
    rec["codes"] = np.array(codes)
    rec["info"] = np.array([info.n_before, info.n_after, info.overruns, info.dropped], dtype=np.uint64)
    rec["rng"] = np.array([f.rng_state().minstd_x], dtype=np.uint64)
    f.close()
    if comm.error is not None:
        raise comm.error
    np.savez(out, **rec)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
