"""Times eslam_gpu_resample_stratified_sharded / _multinomial_sharded on one rank (the library's
own RCCL communicator to itself) against the plain one-context calls of the same shapes.

    python profiles/resample_sharded/time_resample_sharded.py [--n 4194304] [--reps 10]
        [--out profiles/resample_sharded/time_resample_sharded.json]

Shapes: n -> n / 2, n -> n + 64, n -> 2 n, stratified and multinomial.  The calls are synchronous
and change the count, so every repetition starts from the same uploaded particles (the upload,
and on the sharded filter the resample back to the table of n, are not timed); the sharded and
the plain call of a shape are interleaved repetition by repetition.  Each figure is the median
over `reps` calls after 2 warm-up calls, with device events around the call (torch.cuda.Event)
and with the host clock.  On one rank no record crosses a rank: the difference is the call's
collectives (to the rank itself), the routing passes and the host's reads between them.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))

import numpy as np  # noqa: E402


def once(call, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    info = call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, info


def summary(ev, host):
    return {"event_ms_median": statistics.median(ev), "event_ms_min": min(ev), "event_ms_max": max(ev),
            "host_ms_median": statistics.median(host)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_sharded", "time_resample_sharded.json"))
    args = ap.parse_args()
    import torch
    import torch.distributed as dist
    import eslam_abi as A
    import eslam_amd
    import eslam_dist
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    n = args.n
    rng = np.random.default_rng(1)
    pa = A.ParticleArrays(n)
    pa.x[:] = rng.standard_normal(n)
    pa.y[:] = rng.standard_normal(n)
    pa.weight[:] = rng.uniform(size=n) ** 6
    pa.weight[:] /= pa.weight.sum()
    torch.cuda.set_device(0)
    store = os.path.join(tempfile.mkdtemp(), "store")
    dist.init_process_group("nccl", init_method="file://" + store, rank=0, world_size=1)
    plain = eslam_amd.GpuFilter(A.default_config())
    shard = eslam_dist.RcclShardedGpuFilter(A.default_config(), n, 0, 1, device=0)
    res = {"n": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "ranks": 1, "shapes": {}}

    def reset():
        plain.upload(pa)
        if shard.n_global != n:
            shard.resample_stratified_sharded(n)           # back to the table of n particles
        shard.upload(pa)

    for kind in ("stratified", "multinomial"):
        for samples in (n // 2, n + 64, 2 * n):
            calls = {"sharded": lambda: getattr(shard, f"resample_{kind}_sharded")(samples),
                     "plain": lambda: getattr(plain, f"resample_{kind}")(samples)}
            times = {k: ([], []) for k in calls}
            after = {}
            for rep in range(args.reps + 2):
                reset()
                for k in ("sharded", "plain") if rep % 2 == 0 else ("plain", "sharded"):
                    ev, host, info = once(calls[k], torch)
                    after[k] = (info.n_before, info.n_after, info.overruns, info.dropped)
                    if rep >= 2:
                        times[k][0].append(ev)
                        times[k][1].append(host)
            assert after["sharded"] == after["plain"], after
            row = {k: summary(*times[k]) for k in calls}
            row["n_after"] = after["plain"][1]
            row["sharded_minus_plain_ms"] = row["sharded"]["event_ms_median"] - row["plain"]["event_ms_median"]
            res["shapes"][f"{kind} {n} -> {samples}"] = row
            print(json.dumps({"shape": f"{kind} {n} -> {samples}", **row}), flush=True)
    shard.close()
    plain.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
