"""One gloo rank of tests/test_gpu_gmm.py's sharded test: eslam_gpu_fit_pose_gmm on a filter
sharded over 2 or 3 ranks that share one GPU.

    RANK=r WORLD_SIZE=w ESLAM_DIST_STORE=file python tests/gmm_dist_worker.py N_GLOBAL OUT.npz

First the calls every rank refuses before any collective (bad arguments): rank 1 and up ask first
and rank 0 after a barrier, so a call that entered a collective would hang.  Then the ranks ask
together with different max_iterations: the parameter all_gather is the call's first collective,
every rank sees the mismatch and returns ESLAM_ERR_INVALID_ARG, and the fits that follow show
that no rank is a collective behind.  Then the fits of FITS, every output and info field saved.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "slam-eslam_amd"))

import numpy as np  # noqa: E402

# (components, max_iterations, tolerance)
FITS = [(1, 10, 1e-5), (3, 10, 1e-5), (8, 10, 0.0), (3, 0, 1e-5), (5, 1, 1e-5), (2, 10, 1e-5)]
BAD = [dict(components=0), dict(components=9), dict(tolerance=-1.0), dict(min_variance=0.0)]


def global_cloud(n_global):
    """the test's particles: three clusters, some skipped particles among them"""
    import gmm_cases as G
    x, y, w = G.cloud(n_global, seed=n_global)
    return G.with_skipped(x, y, w, seed=5)[:3]


def particles(x, y, w):
    import eslam_abi as A
    pa = A.ParticleArrays(x.shape[0])
    pa.x[:], pa.y[:], pa.weight[:] = x, y, w
    pa.zsigma[:] = 0.01
    return pa


def main():
    n_global, out = int(sys.argv[1]), sys.argv[2]
    import torch.distributed as dist
    import eslam_abi as A
    import eslam_amd
    import eslam_dist
    import gmm_ref as R
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo", init_method="file://" + os.environ["ESLAM_DIST_STORE"], rank=rank,
                            world_size=int(os.environ["WORLD_SIZE"]))
    comm = eslam_dist.TorchComm(device_memory=False)
    f = eslam_dist.ShardedGpuFilter(A.default_config(), n_global, comm, device=0)
    lo, hi = f.bounds[rank], f.bounds[rank + 1]
    x, y, w = global_cloud(n_global)
    f.upload(particles(x[lo:hi], y[lo:hi], w[lo:hi]))
    codes = []
    for kw in BAD:
        if rank == 0:
            dist.barrier()
        try:
            f.fit_pose_gmm(**kw)
            codes.append(0)
        except eslam_amd.EslamError as e:
            codes.append(e.code)
        if rank != 0:
            dist.barrier()
    try:
        f.fit_pose_gmm(3, 5 + rank)
        codes.append(0)
    except eslam_amd.EslamError as e:
        codes.append(e.code)
    rec = {"codes": np.array(codes), "chunks": np.array([-(-(hi - lo) // 64)])}
    for i, (k, iters, tol) in enumerate(FITS):
        wts, means, covs, info = f.fit_pose_gmm(k, iters, tol)
        rec[f"fit{i}"] = np.concatenate([wts, means.ravel(), covs.ravel()])
        rec[f"info{i}"] = np.array([v & (2 ** 64 - 1) for v in R.info_tuple(info)], dtype=np.uint64)
    f.close()
    if comm.error is not None:
        raise comm.error
    np.savez(out, **rec)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
