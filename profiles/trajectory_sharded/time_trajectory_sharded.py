"""Times the trajectory log of a sharded filter on the GPU (DESIGN.md 5j "Sharded"), on ONE rank:
the ranks of the tests share a GPU and talk through gloo in host memory, and RCCL has never run
with more than one rank in this project, so nothing here says what more than one rank costs.

    python profiles/trajectory_sharded/time_trajectory_sharded.py [--n 4194304] [--steps 50] [--reps 7]
        [--held 16] [--parent-lib PATH/libeslam_gpu.so] [--out profiles/trajectory_sharded/time_trajectory_sharded.json]

1. Log off (only with --parent-lib, a library built from the parent commit): `bench.py --gpus 1
   --steps 50 --warmup 10` and the same with --sharded (the one-rank sharded step), this commit's
   library and the parent's alternating three times, one process each.  The only addition on
   that path is a host branch.
2. Log on, one rank sharded, a resample forced every step: windows of `steps` back-to-back steps
   closed by a sync, log off / log on alternating `reps` times in one process after a warm-up
   window of each; the median window's time per step.  The floor the addition is compared with:
   the record's 96 B and the un-fused gather's 130 B per particle at 8 TB/s (as in
   profiles/trajectory/time_trajectory.py).  Beyond the floor the log ends the deferral of the
   update's exchange: the record settles it, so the next step's weighting kernel no longer
   overlaps the host's wait for the slice totals.
3. The queries, one rank sharded against the one-GPU log of a plain filter given the same steps in
   the same process, alternating: trajectory_smoothed over `held` entries, get_trajectories of 1 and
   of 4096 leaves.  Wall clock around the synchronous calls, medians.  On one rank every slot is
   local: the difference is what going through the exchange's serve kernel and item array costs
   over the one-GPU kernels, which chase the indices in place.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 8e12
RECORD_BYTES = 5 * 8 * 2 + 4 + 4 + 4 + 4            # columns in and out, anc, link, parent, the next link
GATHER_BYTES = (7 * 8 + 1) * 2 + 4 + 4 + 4 + 4      # the state in and out, the marks read and cleared, anc


def bench_ms(extra, lib):
    env = dict(os.environ)
    env.pop("ESLAM_GPU_LIB", None)
    if lib:
        env["ESLAM_GPU_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "10"] + extra,
                       env=env, capture_output=True, text=True, timeout=600, check=True)
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def log_off_against_parent(parent_lib, rounds=3):
    out = {}
    for name, extra in (("bench", []), ("bench_sharded_one_rank", ["--sharded"])):
        this, parent = [], []
        for _ in range(rounds):
            parent.append(bench_ms(extra, parent_lib))
            this.append(bench_ms(extra, None))
        out[name] = {"ms_per_step_parent": parent, "ms_per_step_this": this}
        print(json.dumps({name: out[name]}), flush=True)
    return out


def timed(call, reps, warm=1):
    for _ in range(warm):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--held", type=int, default=16)
    ap.add_argument("--map-cells", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory_sharded", "time_trajectory_sharded.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    res = {"n": args.n, "steps": args.steps, "reps": args.reps, "held": args.held, "device": torch.cuda.get_device_name(0),
           "ranks": 1, "more_than_one_rank": "not measured"}
    if args.parent_lib:
        res["log_off"] = log_off_against_parent(os.path.abspath(args.parent_lib))

    import torch.distributed as dist
    import eslam_abi as A
    import eslam_amd
    import eslam_dist
    import synthetic as S
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl")
    n = args.n
    grid = S.flat_map(cells=args.map_cells)
    stream = S.step_stream(args.steps)

    def config():
        cfg = S.bench_config(A.default_config(), n)
        cfg.sum_chunk_rows = A.chunk_rows(n)            # as bench.py --sharded
        return cfg

    sf = eslam_dist.RcclShardedGpuFilter(config(), n, 0, 1, device=0)
    pf = eslam_amd.GpuFilter(config())
    for f in (sf, pf):
        f.set_map(grid)
        f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)

    def window(f):
        t0 = time.perf_counter()
        for st in stream:
            f.step(st)
        info = f.sync()
        assert info.resampled == 1
        return (time.perf_counter() - t0) * 1e3 / len(stream)

    # 2. the one-rank sharded step, log off and on; the plain filter takes the same windows (its
    # one-GPU log's cost in the same run, and the same particles for the queries below)
    off, on, poff, pon = [], [], [], []
    for rep in range(-1, args.reps):                    # rep -1 warms both up
        sf.trajectory_disable()
        pf.trajectory_disable()
        t_off, p_off = window(sf), window(pf)
        sf.trajectory_enable(args.held)
        pf.trajectory_enable(args.held)
        t_on, p_on = window(sf), window(pf)
        if rep >= 0:
            off.append(t_off)
            on.append(t_on)
            poff.append(p_off)
            pon.append(p_on)
    diff_us = (statistics.median(on) - statistics.median(off)) * 1e3
    floor_us = (RECORD_BYTES + GATHER_BYTES) * n / HBM_BYTES_PER_S * 1e6
    res["step_sharded_one_rank"] = {"ms_off_median": statistics.median(off), "ms_off": off, "ms_on_median": statistics.median(on),
                                    "ms_on": on, "log_adds_us": diff_us, "record_bytes_per_particle": RECORD_BYTES,
                                    "gather_bytes_per_particle": GATHER_BYTES, "floor_us": floor_us,
                                    "floor_fraction_of_addition": floor_us / diff_us if diff_us > 0 else None,
                                    "one_gpu_ms_off_median": statistics.median(poff), "one_gpu_ms_on_median": statistics.median(pon),
                                    "one_gpu_log_adds_us": (statistics.median(pon) - statistics.median(poff)) * 1e3}
    print(json.dumps({"step_sharded_one_rank": res["step_sharded_one_rank"]}), flush=True)

    # 3. the queries: both filters took the same steps and hold the same entries
    assert sf.trajectory_info().entries == pf.trajectory_info().entries == min(args.held, args.steps)
    same = [bytes(a) == bytes(b) for a, b in zip(sf.trajectory_smoothed(), pf.trajectory_smoothed())]
    leaves = np.linspace(0, n - 1, 4096).astype(np.uint64)
    same.append(sf.trajectories(leaves).tobytes() == pf.trajectories(leaves).tobytes())
    res["queries_equal_one_gpu_bytes"] = all(same)
    q = {}
    for name, call in (("smoothed", lambda f: f.trajectory_smoothed()), ("leaves_1", lambda f: f.trajectories([n // 2])),
                       ("leaves_4096", lambda f: f.trajectories(leaves))):
        a, b = [], []
        for _ in range(3):                              # alternate the two filters
            b.append(timed(lambda: call(pf), args.reps)["ms_median"])
            a.append(timed(lambda: call(sf), args.reps)["ms_median"])
        q[name] = {"ms_sharded_one_rank": statistics.median(a), "ms_one_gpu_log": statistics.median(b),
                   "ms_sharded_series": a, "ms_one_gpu_series": b, "difference_ms": statistics.median(a) - statistics.median(b)}
    res["queries"] = q
    print(json.dumps({"queries": q, "equal_bytes": res["queries_equal_one_gpu_bytes"]}), flush=True)
    pf.close()
    sf.close()
    dist.destroy_process_group()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
