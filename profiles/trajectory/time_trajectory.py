"""Times the trajectory log on the GPU: what recording costs a step, and the two
queries against the route a caller had before -- downloading the particles and the ancestors
after every step and composing lineages on the host.

    python profiles/trajectory/time_trajectory.py [--n 4194304] [--steps 50] [--reps 7] [--held 16]
                                                  [--out profiles/trajectory/time_trajectory.json]

The flat map, a resample forced at every step (bench.py's configuration).  One filter, one
process: windows of `steps` back-to-back steps, each closed by a sync, alternating log off / log on
`reps` times after a warm-up window of each; the figure is the median window's time per step.  The
record moves 96 B per particle (the five columns read and written, anc and link read, parent and
the next link written); the gather that the log materialises instead of leaving it to the next
weighting kernel moves another 130 B per particle (six fp64 columns, mprob and the flags read and
written, the marks read and anc written).  Both against 8 TB/s give the floor the difference is
compared with.  The queries are synchronous calls, timed by the wall clock around them (median
over `reps` after a warm-up call); the download route is eslam_gpu_download_particles plus
eslam_gpu_get_ancestors of the same filter, what every step would cost.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 8e12
RECORD_BYTES = 5 * 8 * 2 + 4 + 4 + 4 + 4            # columns in and out, anc, link, parent, the next link
GATHER_BYTES = (7 * 8 + 1) * 2 + 4 + 4 + 4 + 4      # the state in and out, the marks read and cleared, anc


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory", "time_trajectory.json"))
    args = ap.parse_args()
    import torch
    import eslam_abi as A
    import eslam_amd
    import synthetic as S
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    n = args.n
    cfg = S.bench_config(A.default_config(), n)
    f = eslam_amd.GpuFilter(cfg)
    f.set_map(S.flat_map(cells=args.map_cells))
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)
    stream = S.step_stream(args.steps)
    res = {"n": n, "steps": args.steps, "reps": args.reps, "held": args.held, "device": torch.cuda.get_device_name(0)}

    def window():
        t0 = time.perf_counter()
        for st in stream:
            f.step(st)
        info = f.sync()
        assert info.resampled == 1
        return (time.perf_counter() - t0) * 1e3 / len(stream)

    # 1. the step, log off and on, alternating in one process
    off, on = [], []
    for rep in range(-1, args.reps):                # rep -1 warms both up
        f.trajectory_disable()
        t_off = window()
        f.trajectory_enable(args.held)
        t_on = window()
        if rep >= 0:
            off.append(t_off)
            on.append(t_on)
    diff_us = (statistics.median(on) - statistics.median(off)) * 1e3
    floor_us = (RECORD_BYTES + GATHER_BYTES) * n / HBM_BYTES_PER_S * 1e6
    res["step"] = {"ms_off_median": statistics.median(off), "ms_off": off, "ms_on_median": statistics.median(on), "ms_on": on,
                   "record_us": diff_us, "record_bytes_per_particle": RECORD_BYTES, "gather_bytes_per_particle": GATHER_BYTES,
                   "record_floor_us": RECORD_BYTES * n / HBM_BYTES_PER_S * 1e6, "floor_us": floor_us,
                   "achieved_fraction_of_floor": floor_us / diff_us if diff_us > 0 else None}
    print(json.dumps({"step": res["step"]}), flush=True)

    # 2. the smoothed trajectory over the held entries (the last window left `held` of them)
    info = f.trajectory_info()
    assert info.entries == min(args.held, args.steps)
    est = f.trajectory_smoothed()
    r = timed(f.trajectory_smoothed, args.reps)
    r["entries"] = len(est)
    r["ms_per_level"] = r["ms_median"] / len(est)
    r["distinct_ancestors"] = [int(e.distinct_ancestors) for e in est]
    # a level moves: a read and written, five columns gathered and written, parent gathered, then
    # three passes of the moments over six columns (the bounds, the mean, the covariance)
    r["level_bytes_per_particle"] = 4 + 4 + 5 * 8 * 2 + 4 + 3 * 6 * 8
    r["level_floor_us"] = r["level_bytes_per_particle"] * n / HBM_BYTES_PER_S * 1e6
    res["smoothed"] = r
    print(json.dumps({"smoothed": r}), flush=True)

    # ... against the route without the log: the particles and the ancestors to the host, every step
    out = A.ParticleArrays(n)
    view = out.view()
    anc = np.zeros(n, dtype=np.uint32)

    def download():
        f._check(f.L.eslam_gpu_download_particles(f.h, C.byref(view)))
        f._check(f.L.eslam_gpu_get_ancestors(f.h, anc.ctypes.data_as(C.POINTER(C.c_uint32)), n))

    d = timed(download, args.reps)
    link = np.arange(n, dtype=np.uint32)
    d["host_compose_ms"] = timed(lambda: link[anc], args.reps)["ms_median"]
    d["per_held_window_ms"] = len(est) * (d["ms_median"] + d["host_compose_ms"])
    d["window_over_smoothed"] = d["per_held_window_ms"] / r["ms_median"]
    res["download_particles_and_ancestors"] = d
    print(json.dumps({"download_particles_and_ancestors": d}), flush=True)

    # 3. lineages of 1 and of 4096 leaves
    leaves = np.linspace(0, n - 1, 4096).astype(np.uint64)
    res["trajectories"] = {"leaves_1": timed(lambda: f.trajectories([n // 2]), args.reps),
                           "leaves_4096": timed(lambda: f.trajectories(leaves), args.reps)}
    print(json.dumps({"trajectories": res["trajectories"]}), flush=True)
    f.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
