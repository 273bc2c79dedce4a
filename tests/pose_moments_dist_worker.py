"""One gloo rank of tests/test_gpu_pose_moments.py's sharded test: eslam_gpu_pose_moments on a filter
sharded over 2 or 3 ranks that share one GPU.

    RANK=r WORLD_SIZE=w ESLAM_DIST_STORE=file python tests/pose_moments_dist_worker.py N_GLOBAL OUT.npz

First the calls every rank refuses before any collective (refused gates): rank 1 and up ask first
and rank 0 after a barrier, so a call that entered a collective would hang.  Then the ranks ask
together with different gates, and with a gate on rank 0 only: the gate all_gather is the call's
first collective, every rank sees the mismatch and returns ESLAM_ERR_INVALID_ARG, and the calls
that follow show that no rank is a collective behind.  Then the calls of global_cloud()'s gates,
every field saved.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "slam-eslam_amd"))

import numpy as np  # noqa: E402

BAD = [dict(cov=(1.0, 1.0, 1.0)), dict(cov=(-1.0, 0.0, -1.0)), dict(chi2=-1.0), dict(centre=(float("nan"), 0.0))]


def global_cloud(n_global):
    """the test's particles -- two clusters, every kind of skipped particle among them -- and the
    gates asked for: none, the first cluster's, none again, a circle that holds nothing"""
    import eslam_abi as A
    import moments_cases as M
    c, gate = M.cloud(n_global, seed=n_global)
    c = M.with_skipped(c, seed=5)[0]
    return c, [None, gate, None, A.PoseGate((-500.0, 500.0), (1.0, 0.0, 1.0), 1.0), A.PoseGate((26.0, -7.5), (1.0, 0.3, 1.0), 4.0)]


def main():
    n_global, out = int(sys.argv[1]), sys.argv[2]
    import torch.distributed as dist
    import eslam_abi as A
    import eslam_amd
    import eslam_dist
    import moments_cases as M
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo", init_method="file://" + os.environ["ESLAM_DIST_STORE"], rank=rank,
                            world_size=int(os.environ["WORLD_SIZE"]))
    comm = eslam_dist.TorchComm(device_memory=False)
    f = eslam_dist.ShardedGpuFilter(A.default_config(), n_global, comm, device=0)
    lo, hi = f.bounds[rank], f.bounds[rank + 1]
    c, gates = global_cloud(n_global)
    f.upload(M.particles({k: a[lo:hi] for k, a in c.items()}))
    codes = []

    def ask(gate):
        try:
            f.pose_moments(gate)
            codes.append(0)
        except eslam_amd.EslamError as e:
            codes.append(e.code)

    for kw in BAD:
        if rank == 0:
            dist.barrier()
        ask(A.PoseGate(**kw))
        if rank != 0:
            dist.barrier()
    ask(A.PoseGate((20.0, -7.0), (0.16, 0.0, 0.0625), 9.0 + rank))
    ask(A.PoseGate() if rank == 0 else None)
    rec = {"codes": np.array(codes), "chunks": np.array([-(-(hi - lo) // 64)])}
    for i, gt in enumerate(gates):
        rec[f"m{i}"] = np.array([v & (2 ** 64 - 1) for v in f.pose_moments(gt).as_tuple()], dtype=np.uint64)
    f.close()
    if comm.error is not None:
        raise comm.error
    np.savez(out, **rec)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
