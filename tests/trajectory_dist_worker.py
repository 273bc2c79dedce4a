"""One gloo rank of tests/test_gpu_trajectory_sharded.py: the trajectory log on a filter sharded
over 1, 2 or 3 ranks that share one GPU (eslam_gpu_trajectory_enable_sharded).

    RANK=r WORLD_SIZE=w ESLAM_DIST_STORE=file python tests/trajectory_dist_worker.py OUT.npz

Two runs of tests/trajectory_shard_scenarios.run, a fresh filter each: with the log ("on/...") and
without it ("off/...": the particles only).  Around the first run's enable, the refusals.  Those
every rank refuses before any collective: rank 1 and up ask first and rank 0 after a barrier, so
a call that entered a collective would hang.  Then the mismatches, asked by the ranks together:
every rank sees them in the call's first collective and returns ESLAM_ERR_INVALID_ARG, and the
scenario that follows shows that no rank is a collective behind.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "slam-eslam_amd"))

import numpy as np  # noqa: E402


def main():
    out = sys.argv[1]
    import torch.distributed as dist
    import eslam_amd
    import eslam_dist
    import trajectory_shard_scenarios as T
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", init_method="file://" + os.environ["ESLAM_DIST_STORE"], rank=rank, world_size=world)
    comm = eslam_dist.TorchComm(device_memory=False)
    rec = {}
    for log in (True, False):
        f = eslam_dist.ShardedGpuFilter(T.config(), T.N, comm, device=0)
        codes = {}

        def code(call):
            try:
                call()
                return 0
            except eslam_amd.EslamError as e:
                return e.code

        def alone(name, call):
            """rank 0 asks after the others: refused before any collective, or the launch hangs"""
            if rank == 0:
                dist.barrier()
            codes[name] = code(call)
            if rank != 0:
                dist.barrier()

        def before_enable():
            alone("off", lambda: f.trajectories([0], capacity=4))
            alone("capacity0", lambda: f.trajectory_enable(0))
            codes["capacity_differs"] = code(lambda: f.trajectory_enable(T.CAPACITY + rank, T.MAX_PARTICLES[world]))
            codes["enabled_after_mismatch"] = f.trajectory_info().enabled

        def after_enable():
            alone("index", lambda: f.trajectories([0, T.N]))
            alone("too_many", lambda: f.resample_stratified_sharded(T.TOO_MANY))
            codes["leaves_differ"] = code(lambda: f.trajectories([rank, 7]))
            codes["counts_differ"] = code(lambda: f.trajectories([7] * (1 + rank)))
            codes["count_after"] = f.count()

        sub = {}
        T.run(sub, f, f.bounds[rank], f.bounds[rank + 1], True, log=log, world=world,
              before_enable=before_enable if log else None, after_enable=after_enable if log else None)
        for k, v in sub.items():
            rec[("on/" if log else "off/") + k] = v
        for k, v in codes.items():
            rec["code/" + k] = np.array([v], dtype=np.int64)
        if log:
            info = f.trajectory_info()
            rec["on/max_particles"] = np.array([info.max_particles, info.bytes], dtype=np.uint64)
            f.trajectory_clear()                                    # a collective; every rank resets alike
            rec["on/cleared"] = np.array([f.trajectory_info().entries, len(f.trajectory_smoothed())], dtype=np.uint64)
            f.trajectory_disable()
        f.close()
        if comm.error is not None:
            raise comm.error
    np.savez(out, **rec)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
