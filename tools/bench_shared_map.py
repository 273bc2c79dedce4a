"""Time the merge into the shared map (DESIGN.md 5c's workload: a rough 1000 x 1000 map, a
48-patch scan, init sigma 0.1 m, 65,536 particles; the host clock around the call, which ends
in a device synchronise; one warm-up call, then the median of 5):

    python tools/bench_shared_map.py [--libs THIS.so OTHER.so ...] [--rounds 5] [--particles 65536] [--out FILE]

  plain        eslam_gpu_shared_map_update, once per library of --libs (default: the in-tree
               build) in every round, the libraries taking turns within a round (each round
               starting with another one) so that a drift of the box reaches all of them alike.
               Every measurement is a fresh process.
  collective   eslam_gpu_shared_map_update_sharded on one rank over the library's own RCCL
               communicator (the first library only), once per round

Per series it reports the rounds' medians, their median and their spread (max - min over the
median, in per cent), and per pair of libraries the difference of their medians: a change is
free when that difference lies within the spreads.  Prints one JSON line; needs a GPU (no
fallback)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))

REPS = 5
CHILD_LIMIT = 300                            # seconds a measurement may take


def child(mode, n):
    """one measurement: the calls' times in ms (after one warm-up call) as a JSON line"""
    import eslam_abi as A
    import eslam_amd
    import synthetic as S
    cfg = S.bench_config(A.default_config(), n)
    if mode == "collective":
        import torch
        import torch.distributed as dist
        import eslam_dist
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", init_method="file://" + os.environ["ESLAM_DIST_STORE"], rank=0, world_size=1)
        f = eslam_dist.RcclShardedGpuFilter(cfg, n, 0, 1, device=0)
        call = f.shared_map_update_sharded
    else:
        f = eslam_amd.GpuFilter(cfg, device=0)
        call = f.shared_map_update
    f.set_map(S.rough_map())
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 0.05)
    scan = S.scan_patches()
    ms, info = [], None
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        info = call(scan)
        dt = (time.perf_counter() - t0) * 1e3
        if rep:                               # the first call warms up: code objects, scratch
            ms.append(dt)
    out = {"ms": [round(v, 3) for v in ms], "runs": int(info.runs), "records": int(info.patches_placed),
           "cells": int(info.cells_touched), "build_id": eslam_amd.build_id()[:16]}
    f.close()
    if mode == "collective":
        dist.destroy_process_group()
    print("RESULT " + json.dumps(out), flush=True)


def measure(mode, lib, n, tmp):
    env = dict(os.environ)
    if lib:
        env["ESLAM_GPU_LIB"] = os.path.abspath(lib)
    store = os.path.join(tmp, "store")
    if os.path.exists(store):
        os.remove(store)
    env["ESLAM_DIST_STORE"] = store
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--particles", str(n)], env=env,
                       capture_output=True, text=True, timeout=CHILD_LIMIT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"{mode} {lib}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(lines[-1][len("RESULT "):])


def series(results):
    med = [statistics.median(r["ms"]) for r in results]
    m = statistics.median(med)
    return {"median_ms": round(m, 3), "round_medians_ms": [round(v, 3) for v in med],
            "spread_pct": round(100.0 * (max(med) - min(med)) / m, 2), "runs": results[0]["runs"],
            "records": results[0]["records"], "cells": results[0]["cells"], "build_id": results[0]["build_id"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="*", default=[], help="libraries whose plain call is timed in turn (default: the in-tree build)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--particles", type=int, default=65536)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.particles)
    libs = args.libs or [None]
    plain, coll = {lib: [] for lib in libs}, []
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(args.rounds):
            for lib in libs[k % len(libs):] + libs[:k % len(libs)]:      # each round starts with another library
                plain[lib].append(measure("plain", lib, args.particles, tmp))
            coll.append(measure("collective", libs[0], args.particles, tmp))
    out = {"tool": "bench_shared_map", "particles": args.particles, "patches": 48, "reps": REPS, "rounds": args.rounds,
           "plain": {os.path.basename(lib) if lib else "in-tree": series(plain[lib]) for lib in libs},
           "collective_one_rank_rccl": series(coll)}
    names = list(out["plain"])
    base = out["plain"][names[0]]["median_ms"]
    out["plain_vs_first_pct"] = {k: round(100.0 * (out["plain"][k]["median_ms"] - base) / base, 2) for k in names[1:]}
    out["collective_vs_plain_pct"] = round(100.0 * (out["collective_one_rank_rccl"]["median_ms"] - base) / base, 2)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
