"""Times eslam_gpu_kld_count on the GPU against what a caller did before it: eslam_gpu_download_particles
of the same filter and the bin count on the host (the numpy model of tests/kld_cases.py).

    python profiles/kld/time_kld.py [--n 4194304] [--reps 20] [--out profiles/kld/time_kld.json]

Two clouds at the default lattice (0.1 m, 36 yaw bins): a converged one (sigma 2 cm in x and y,
0.02 rad in yaw: a few dozen bins, every lane of a wave on a handful of bitmap words) and a spread
one (uniform over a 10 m box and the whole turn).  The call is synchronous; each figure is the
wall time around it, the median over `reps` calls after 3 warm-up calls.  The count reads x, y,
theta, w twice (the box, then the marks): 64 B per particle, plus the bitmap.  The host route is
timed in two parts, the download alone and the numpy model on the downloaded arrays (one call).
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


def timed(call, reps, warm=3):
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kld", "time_kld.json"))
    args = ap.parse_args()
    import torch
    import eslam_abi as A
    import eslam_amd
    import kld_cases as K
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    n = args.n
    rng = np.random.default_rng(1)
    clouds = {
        "converged": (1.234 + 0.02 * rng.standard_normal(n), -0.567 + 0.02 * rng.standard_normal(n), 0.3 + 0.02 * rng.standard_normal(n)),
        "spread": (rng.uniform(-5.0, 5.0, n), rng.uniform(-5.0, 5.0, n), rng.uniform(-np.pi, np.pi, n)),
    }
    res = {"n": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "floor_us": 64.0 * n / HBM_BYTES_PER_S * 1e6,
           "clouds": {}}
    for name, (x, y, th) in clouds.items():
        pa = A.ParticleArrays(n)
        pa.x[:], pa.y[:], pa.orientation[:] = x, y, th
        pa.weight[:] = rng.uniform(0.2, 1.0, n) / n
        pa.zpos[:], pa.zsigma[:] = 0.18, 0.01
        g = eslam_amd.GpuFilter(A.default_config())
        g.upload(pa)
        info = g.kld_count(n_min=1)
        rc, want = K.model(pa.x, pa.y, pa.orientation, pa.weight, n_min=1)
        assert rc == 0 and info.bins_occupied == want["bins_occupied"] and info.samples == want["samples"], (info.as_dict(), want)
        r = {"bins_occupied": info.bins_occupied, "box": list(info.bins), "samples": info.samples,
             "kld_count": timed(lambda: g.kld_count(n_min=1), args.reps)}
        out = A.ParticleArrays(n)
        view = out.view()
        r["download_particles"] = timed(lambda: g._check(g.L.eslam_gpu_download_particles(g.h, C.byref(view))), args.reps)
        r["numpy_model_on_host"] = timed(lambda: K.model(out.x, out.y, out.orientation, out.weight, n_min=1), 1, warm=0)
        r["download_over_count"] = r["download_particles"]["ms_median"] / r["kld_count"]["ms_median"]
        res["clouds"][name] = r
        print(json.dumps({"cloud": name, **r}), flush=True)
        g.close()
    res["converged_over_spread"] = res["clouds"]["converged"]["kld_count"]["ms_median"] / res["clouds"]["spread"]["kld_count"]["ms_median"]
    print(json.dumps({"converged_over_spread": res["converged_over_spread"], "floor_us": res["floor_us"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
