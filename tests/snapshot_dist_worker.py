"""One rank of tests/test_gpu_snapshot_sharded.py: a sharded GPU filter runs a short
program of scenario steps and positional saves and loads of one shared file.

    RANK=r WORLD_SIZE=w ESLAM_DIST_STORE=file python tests/snapshot_dist_worker.py SCENARIO N_GLOBAL OUT.npz PROGRAM [MEM]

MEM (as in tests/dist_worker.py): 'host' (the default) exchanges host buffers over gloo; 'device'
exchanges device buffers through the torch.distributed callbacks (nccl); 'rccl' goes over the
library's own RCCL communicator (eslam_gpu_set_comm_rccl).

PROGRAM is a JSON list of operations:
    ["prepare"]                 set_map and the scenario's initialisation of this rank's shard
    ["steps", k0, k1]           steps [k0, k1) of the scenario's stream (every step's update info is recorded)
    ["save", path, chunk]       save_state_at into the one file at path (all ranks write their parts)
    ["load", path, chunk]       load_state_at from it
    ["load_mem", path]          eslam_gpu_load of the whole blob held in memory by every rank
    ["refusals", good, other]   the refusals and the agreement on failure (2 ranks; `other` has another n)
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "slam-eslam_amd"))

import numpy as np  # noqa: E402


def code_of(call, *args):
    import eslam_amd
    try:
        call(*args)
        return 0
    except eslam_amd.EslamError as e:
        return e.code


def refusals(rec, dist, comm, name, n_global, good, other):
    """Return codes on a healthy device (none of this faults): a blob of another n is refused
    before any collective; a read or write callback failing on one rank, and a page pool too
    small on one rank, fail the call on every rank."""
    import eslam_abi as A
    import eslam_dist
    from snapshot_shard_scenarios import config, stream
    rank = comm.rank
    f = eslam_dist.ShardedGpuFilter(config(name, n_global), n_global, comm, device=0)
    # rank 1 asks first and rank 0 after a barrier: a call that entered a collective would hang
    if rank == 0:
        dist.barrier()
    rec["other_n"] = np.array([code_of(f.load_state_at, other)])
    if rank != 0:
        dist.barrier()
    # a read callback that fails on rank 1 only, behind the header
    size = os.path.getsize(good)
    fd = os.open(good, os.O_RDONLY)
    calls = []

    def pread(_user, offset, data, nbytes):
        calls.append(offset)
        if rank == 1 and len(calls) > 3:
            return 1
        C.memmove(data, os.pread(fd, nbytes, offset), nbytes)
        return 0

    info = A.SnapshotInfo()
    rec["bad_read"] = np.array([f.L.eslam_gpu_load_at(f.h, A.PREAD_FN(pread), None, size, 0, C.byref(info))])
    os.close(fd)
    rec["bad_read_step"] = np.array([code_of(f.step, stream(name)[0])])      # no particles on any rank
    # the good file loads; a write callback that fails on rank 0 only
    f.load_state_at(good)
    rec["bad_write"] = np.array([f.L.eslam_gpu_save_at(f.h, A.PWRITE_FN(lambda u, off, data, n: 1 if rank == 0 else 0), None, 0,
                                                      C.byref(info))])
    rec["still_saves"] = np.array([f.L.eslam_gpu_save_at(f.h, A.PWRITE_FN(lambda u, off, data, n: 0), None, 0, C.byref(info))])
    f.close()
    # a page pool too small on rank 1 only
    cfg = config(name, n_global)
    if rank == 1:
        cfg.local_map_pages = 1
    g = eslam_dist.ShardedGpuFilter(cfg, n_global, comm, device=0)
    rec["small_pool"] = np.array([code_of(g.load_state_at, good)])
    rec["small_pool_step"] = np.array([code_of(g.step, stream(name)[0])])
    g.close()


def main():
    name, n_global, out, program = sys.argv[1], int(sys.argv[2]), sys.argv[3], json.loads(sys.argv[4])
    mem = sys.argv[5] if len(sys.argv) > 5 else "host"
    import torch
    import torch.distributed as dist
    import eslam_dist
    from snapshot_shard_scenarios import advance, config, prepare
    rank = int(os.environ["RANK"])
    if mem in ("device", "rccl"):
        torch.cuda.set_device(0)
    dist.init_process_group("nccl" if mem in ("device", "rccl") else "gloo", init_method="file://" + os.environ["ESLAM_DIST_STORE"],
                            rank=rank, world_size=int(os.environ["WORLD_SIZE"]))
    comm = eslam_dist.TorchComm(device_memory=(mem in ("device", "rccl")))
    rec = {}
    if program[0][0] == "refusals":
        refusals(rec, dist, comm, name, n_global, program[0][1], program[0][2])
    else:
        if mem == "rccl":
            f = eslam_dist.RcclShardedGpuFilter(config(name, n_global), n_global, rank, comm.nranks, device=0)
        else:
            f = eslam_dist.ShardedGpuFilter(config(name, n_global), n_global, comm, device=0)
        lo, hi = f.bounds[rank], f.bounds[rank + 1]
        for k, op in enumerate(program):
            if op[0] == "prepare":
                prepare(f, name, n_global, lo, hi)
            elif op[0] == "steps":
                advance(f, name, op[1], op[2], rec)
            elif op[0] == "save":
                info = f.save_state_at(op[1], chunk_bytes=op[2])
                rec[f"op{k}/save"] = np.array([info.bytes, info.particles, info.tables, info.pages, info.chunks], np.uint64)
            elif op[0] == "load":
                info = f.load_state_at(op[1], chunk_bytes=op[2])
                rec[f"op{k}/load"] = np.array([info.bytes, info.particles, info.tables, info.pages, info.chunks], np.uint64)
                rec[f"op{k}/count"] = np.array([f.count()], np.uint64)
            elif op[0] == "load_mem":
                f.load_state(open(op[1], "rb").read())
            else:
                raise ValueError(op)
        f.close()
    if comm.error is not None:
        raise comm.error
    np.savez(out, **rec)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
