"""Times eslam_gpu_fit_pose_gmm on the GPU against the only route the library offered before it,
eslam_gpu_download_particles of the same filter (before any host fit).

    python profiles/gmm/time_gmm.py [--n 4194304] [--reps 20] [--out profiles/gmm/time_gmm.json]

Per K in {1, 3, 8}: a whole fit of up to 10 iterations (tolerance 0 on overlapping clusters: K = 3
and 8 run all 10; K = 1 reproduces its log-likelihood bit for bit and stops after the second),
a fit of 1 and of 0 iterations (pass B and the hard assignment).  One fused pass is timed as a
caller pays for it, t1 - t0 and (t10 - t0) / iterations: the pass kernel, the tree's launches,
the read-back, the host's M-step and the stream synchronisation, not the kernel alone (the
kernels' own times are in kernel_stats.csv, from a profiler run of this script).  The calls are
synchronous; each figure is the median over `reps` calls after 3 warm-up calls, taken with
device events around the call (torch.cuda.Event) and with the host clock.  The pass reads x, y,
w once: 24 B per particle.
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

import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed(call, reps, torch):
    for _ in range(3):
        call()
    ev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return {"event_ms_median": statistics.median(ev), "event_ms_min": min(ev), "event_ms_max": max(ev),
            "host_ms_median": statistics.median(host)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm", "time_gmm.json"))
    args = ap.parse_args()
    import torch
    import eslam_abi as A
    import eslam_amd
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    n = args.n
    rng = np.random.default_rng(1)
    which = rng.integers(0, 3, n)
    pa = A.ParticleArrays(n)
    pa.x[:] = 4.0 * which + 1.5 * rng.standard_normal(n)
    pa.y[:] = 1.5 * which + 1.0 * rng.standard_normal(n)
    pa.weight[:] = rng.uniform(0.2, 1.0, n) / n
    g = eslam_amd.GpuFilter(A.default_config())
    g.upload(pa)
    res = {"n": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "floor_us_per_pass": 24.0 * n / HBM_BYTES_PER_S * 1e6,
           "fits": {}}
    for K in (1, 3, 8):
        full = g.fit_pose_gmm(K, 10, 0.0)
        iters = full[3].iterations          # K = 1 repeats L exactly and stops after its second pass
        assert 1 <= iters <= 10 and full[3].particles_used == n, full[3].as_dict()
        t10 = timed(lambda: g.fit_pose_gmm(K, 10, 0.0), args.reps, torch)
        t1 = timed(lambda: g.fit_pose_gmm(K, 1, 0.0), args.reps, torch)
        t0 = timed(lambda: g.fit_pose_gmm(K, 0, 0.0), args.reps, torch)
        # one fused pass as a caller pays for it: kernel, tree, read-back, M-step, the stream sync
        one_pass_ms = t1["event_ms_median"] - t0["event_ms_median"]
        mean_pass_ms = (t10["event_ms_median"] - t0["event_ms_median"]) / iters
        res["fits"][str(K)] = {"iterations_run": iters, "fit_max_10_iterations": t10, "fit_1_iteration": t1,
                               "fit_0_iterations": t0, "one_pass_ms": one_pass_ms, "mean_pass_ms": mean_pass_ms,
                               "floor_over_mean_pass": res["floor_us_per_pass"] * 1e-3 / mean_pass_ms,
                               "weights": full[0].tolist(), "log_likelihood": full[3].log_likelihood}
        print(json.dumps({"K": K, **res["fits"][str(K)]}), flush=True)
    out = A.ParticleArrays(n)
    view = out.view()
    res["download_particles"] = timed(lambda: g._check(g.L.eslam_gpu_download_particles(g.h, C.byref(view))), args.reps, torch)
    res["download_bytes"] = int(sum(getattr(out, f).nbytes for f in A.ParticleArrays.FIELDS))
    print(json.dumps({"download_particles": res["download_particles"], "bytes": res["download_bytes"]}), flush=True)
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
