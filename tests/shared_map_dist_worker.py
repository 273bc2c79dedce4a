"""One rank of tests/test_gpu_shared_map_sharded.py: a sharded filter on the shared map goes
through a program of steps and collective merges (eslam_gpu_shared_map_update_sharded) and saves
what it holds after each: its shard's particles, and after a merge its copy of the grid and the
call's counters.  The expected values are the parent's (the CPU reference), never this file's.

    RANK=r WORLD_SIZE=w ESLAM_DIST_STORE=file python tests/shared_map_dist_worker.py CASE N_GLOBAL OUT.npz MEM PROGRAM

MEM      host (gloo, host-memory callbacks), device (torch's nccl backend on device buffers) or
         rccl (the library's own RCCL communicator)
PROGRAM  a JSON list of ["step", k] (the k-th input of S.step_stream(3, tilt=True)),
         ["merge", scan, max_records] and ["differ", scan, max_records] (rank 1 passes the scan
         with one patch's z changed: every rank must be refused); scan is s48, w0, w1 or w2
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "slam-eslam_amd"))

import numpy as np  # noqa: E402


def scans():
    import synthetic as S
    from test_gpu_shared_map import wide_scans
    w = wide_scans()
    return {"s48": S.scan_patches(), "w0": w[0], "w1": w[1], "w2": w[2]}


def main():
    case, n_global, out, mem, program = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4], json.loads(sys.argv[5])
    import torch
    import torch.distributed as dist
    import eslam_abi as A
    import eslam_amd
    import eslam_dist
    import synthetic as S
    from test_gpu_shared_map import case_grid, case_sigma
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    init = dict(init_method="file://" + os.environ["ESLAM_DIST_STORE"], rank=rank, world_size=world)
    if mem in ("device", "rccl"):
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", **init)
    else:
        dist.init_process_group("gloo", **init)
    comm = eslam_dist.TorchComm(device_memory=mem != "host")
    cfg = S.bench_config(A.default_config(), n_global)
    cfg.flags |= A.FLAG_RECORD_ANCESTORS
    if mem == "rccl":
        f = eslam_dist.RcclShardedGpuFilter(cfg, n_global, rank, world, device=0)
    else:
        f = eslam_dist.ShardedGpuFilter(cfg, n_global, comm, device=0)
    lo, hi = f.bounds[rank], f.bounds[rank + 1]
    f.set_map(case_grid(case))
    f.init_gaussian(hi - lo, [0.0, 0.0, 0.0], case_sigma(case), 0.18, 0.05)
    stream, scan = S.step_stream(3, tilt=True), scans()
    rec = {"bounds": np.array(f.bounds, dtype=np.uint64)}

    def keep_particles(i):
        pa = f.download()
        for fld in A.ParticleArrays.FIELDS:
            rec[f"{i}/p/{fld}"] = np.array(getattr(pa, fld))

    def keep_grid(i):
        g = f.get_map()
        rec[f"{i}/g/cell_start"], rec[f"{i}/g/mean"], rec[f"{i}/g/stdev"] = g.cell_start, g.mean, g.stdev
        if g.patch_height is not None:
            rec[f"{i}/g/patch_height"] = g.patch_height

    try:
        for i, op in enumerate(program):
            if op[0] == "step":
                rec[f"{i}/updated"] = np.array(int(f.step(stream[op[1]])))
            elif op[0] == "merge":
                info = f.shared_map_update_sharded(scan[op[1]], op[2])
                rec[f"{i}/info"] = np.array([getattr(info, fld) for fld, _ in A.SharedMergeInfo._fields_], dtype=np.uint64)
                keep_grid(i)
            elif op[0] == "differ":
                patches = scans()[op[1]]
                if rank == 1:
                    patches[5].position[2] += 0.25
                try:
                    f.shared_map_update_sharded(patches, op[2])
                    rec[f"{i}/code"] = np.array(0)
                except eslam_amd.EslamError as e:
                    rec[f"{i}/code"] = np.array(e.code)
                keep_grid(i)
            else:
                raise ValueError(op)
            keep_particles(i)
    except Exception as e:
        if comm.error is not None:           # the collective's own failure, not the library's report of it
            raise RuntimeError(f"rank {rank}: {e}") from comm.error
        raise
    f.close()
    if comm.error is not None:
        raise comm.error
    np.savez(out, **rec)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
