"""Time the export of a particle's whole map (eslam_gpu_get_particle_grid) on the
bench workload: the rough 1000 x 1000 map unmapped beyond x = 0.3 m, 65,536 particles, 20 steps
with a map update each; then, on that one context, the host clock around

    particle_grid(i)    eslam_gpu_particle_grid_size + eslam_gpu_get_particle_grid (the export)
    get_map()           the shared grid's arrays copied out: arrays of the same size, no
                        composition -- the yardstick, not the code under test
    particle_map(i)     the older getter of the particle's own cells (one host copy per page)
    grid_size(i)        eslam_gpu_particle_grid_size alone (the directory and the count)

    python tools/bench_particle_grid.py [--particles 65536] [--updates 20] [--reps 20] [--out FILE]

Every call ends in a device synchronise.  One warm-up call each, then the median of --reps
calls, the particle index moving through the set.  Prints one JSON line; needs a GPU (no
fallback)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))


def timed(calls, reps, indices):
    """the calls take turns within a repetition, so a drift of the box reaches all of them alike"""
    ms = {name: [] for name in calls}
    for name, call in calls.items():
        call(indices[0])                     # warm-up: code objects, scratch
    for k in range(reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call(indices[k % len(indices)])
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
            for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=65536)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cells", type=int, default=1000)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import eslam_abi as A
    import eslam_amd
    import synthetic as S
    n = args.particles
    cfg = S.bench_config(A.default_config(), n)
    cfg.flags |= A.FLAG_PARTICLE_MAPS
    f = eslam_amd.GpuFilter(cfg, device=0)
    f.set_map(S.unmapped_beyond(S.rough_map(cells=args.cells), 0.3))
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)
    scan = S.scan_patches()
    for st in S.step_stream(args.updates, tilt=True):
        f.step(st)
        f.map_update(scan)
    f.sync()
    indices = [(k * 7919) % n for k in range(args.reps)]
    count = C.c_uint64()
    whole = f.particle_grid(indices[0])
    shared = f.get_map()
    out = {"tool": "bench_particle_grid", "particles": n, "cells": args.cells, "updates": args.updates, "reps": args.reps,
           "shared_patches": int(shared.cell_start[-1]), "composed_patches": int(whole.cell_start[-1]),
           "own_cells": len(f.particle_map(indices[0])[0]), "build_id": eslam_amd.build_id()[:16]}
    out.update(timed({"particle_grid": f.particle_grid, "get_map": lambda i: f.get_map(), "particle_map": f.particle_map,
                      "grid_size": lambda i: f._check(f.L.eslam_gpu_particle_grid_size(f.h, i, C.byref(count)))},
                     args.reps, indices))
    out["particle_grid_over_get_map"] = round(out["particle_grid"]["median_ms"] / out["get_map"]["median_ms"], 3)
    f.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
