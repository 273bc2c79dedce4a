"""Times eslam_gpu_pose_moments on the GPU, ungated and gated on the mixture's heaviest component,
and in the same run the two calls it is measured against: eslam_gpu_download_particles of the same
filter (the only route to a pose covariance before it) and eslam_gpu_fit_pose_gmm at K = 1,
max_iterations = 0 (the nearest existing call: pass B, one pass, the tree).

    python profiles/pose_moments/time_pose_moments.py [--n 4194304] [--reps 20] [--out profiles/pose_moments/time_pose_moments.json]

The particles are three overlapping clusters.  The calls are synchronous; each figure is the
median over `reps` calls after 3 warm-up calls, taken with device events around the call
(torch.cuda.Event) and with the host clock: as a caller pays for it -- pass B, the two passes, the
tree's launches, three read-backs and stream synchronisations -- not the kernels alone (their own
times are in kernel_stats.csv, from a profiler run of this script).  Pass B and the two passes each
read x, y, z, theta, zsigma and w once: 48 B per particle per pass.
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
BYTES_PER_PARTICLE = 3 * 48.0          # pass B, pass 1, pass 2


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_moments", "time_pose_moments.json"))
    args = ap.parse_args()
    import torch
    import eslam_abi as A
    import eslam_amd
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    n = args.n
    rng = np.random.default_rng(1)
    which = rng.choice(3, n, p=[0.2, 0.5, 0.3])
    pa = A.ParticleArrays(n)
    pa.x[:] = 4.0 * which + 1.5 * rng.standard_normal(n)
    pa.y[:] = 1.5 * which + 1.0 * rng.standard_normal(n)
    pa.zpos[:] = 0.18 + 0.05 * which + 0.02 * rng.standard_normal(n)
    pa.orientation[:] = 3.0 + 0.4 * which + 0.2 * rng.standard_normal(n)      # across the cut
    pa.zsigma[:] = rng.uniform(0.005, 0.03, n)
    pa.weight[:] = rng.uniform(0.2, 1.0, n) / n
    g = eslam_amd.GpuFilter(A.default_config())
    g.upload(pa)
    floor_us = BYTES_PER_PARTICLE * n / HBM_BYTES_PER_S * 1e6
    res = {"n": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "bytes_read": BYTES_PER_PARTICLE * n, "floor_us": floor_us}
    # the gate: the 3-sigma ellipse of the mixture's heaviest component
    wts, means, covs, _ = g.fit_pose_gmm(3)
    k = int(np.argmax(wts))
    gate = A.PoseGate(tuple(means[k]), tuple(covs[k]), 9.0)
    res["gate"] = {"component": k, "weight": float(wts[k]), "centre": list(gate.centre), "cov": list(gate.cov), "chi2": gate.chi2}
    for name, gt in (("ungated", None), ("gated", gate)):
        m = g.pose_moments(gt)
        assert m.particles_counted + m.particles_gated_out == n and m.particles_counted > 0, m.as_dict()
        t = timed(lambda: g.pose_moments(gt), args.reps, torch)
        res[name] = dict(t, floor_over_call=floor_us * 1e-3 / t["event_ms_median"], result=m.as_dict())
        print(json.dumps({name: res[name]}), flush=True)
    res["fit_pose_gmm_K1_0_iterations"] = timed(lambda: g.fit_pose_gmm(1, 0, 0.0), args.reps, torch)
    print(json.dumps({"fit_pose_gmm_K1_0_iterations": res["fit_pose_gmm_K1_0_iterations"]}), flush=True)
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
