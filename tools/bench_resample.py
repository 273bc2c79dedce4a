"""Time the three resamples on the flat scenario's weights after --steps steps:

    python tools/bench_resample.py [--sizes 4194304:4194304 4194304:1048576 1048576:4194304]
                                   [--steps 10] [--reps 7] [--out FILE]

Per n:samples it reports, in ms between two HIP events on the filter's stream around one call
(one warm-up call first, then --reps repeats from the same particles and RNG state, median and
range):
  resample      eslam_gpu_resample (n == samples only): the scan and the marks; its gather is
                left pending for the next step (fused there), so this is not the whole cost
  resample+gather   the same followed by eslam_gpu_get_weights_sum, which runs the pending gather
                (and one weight sum): the resample with its gather run at once
  stratified    eslam_gpu_resample_stratified(samples): synchronous, gather included; growing
                includes the allocation of the larger particle set
  multinomial   eslam_gpu_resample_multinomial(samples): likewise
The passes' own times come from a run of this tool under `rocprofv3 --kernel-trace --stats`
(k_rs_* kernels), not from these events.  Prints one JSON line; needs a GPU (no fallback)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))

import eslam_abi as A  # noqa: E402
import eslam_amd  # noqa: E402
import synthetic as S  # noqa: E402

hip = C.CDLL("libamdhip64.so")


def chk(rc):
    if rc != 0:
        raise RuntimeError(f"HIP call failed ({rc})")


class Events:
    """a stream the filter runs on, and two timing events on it"""

    def __init__(self):
        self.stream, self.a, self.b = C.c_void_p(), C.c_void_p(), C.c_void_p()
        chk(hip.hipStreamCreate(C.byref(self.stream)))
        chk(hip.hipEventCreate(C.byref(self.a)))
        chk(hip.hipEventCreate(C.byref(self.b)))

    def time(self, fn):
        chk(hip.hipEventRecord(self.a, self.stream))
        fn()
        chk(hip.hipEventRecord(self.b, self.stream))
        chk(hip.hipEventSynchronize(self.b))
        ms = C.c_float()
        chk(hip.hipEventElapsedTime(C.byref(ms), self.a, self.b))
        return ms.value


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "reps": len(ms)}


def prepared(n, steps, ev):
    """the flat scenario at n particles after `steps` steps: (filter, its particles, its RNG state)"""
    cfg = S.bench_config(A.default_config(), n)
    f = eslam_amd.GpuFilter(cfg, device=0)
    f._check(f.L.eslam_gpu_set_stream(f.h, ev.stream))
    f.set_map(S.flat_map())
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)
    for st in S.step_stream(steps):
        f.step(st)
    f.sync()
    return f, f.download(), f.rng_state()


def measure(n, samples, args, ev):
    f, pa, rs = prepared(n, args.steps, ev)
    res = {"n": n, "samples": samples, "steps": args.steps, "weight_sum": f.weights_sum()}

    def timed(call):
        out = []
        for rep in range(args.reps + 1):
            f.upload(pa)                         # the same particles (and capacity) every time
            f.set_rng_state(rs)
            f.weights_sum()                      # nothing pending; ends synchronised
            ms = ev.time(call)
            if rep:                              # the first call warms up: code objects, scratch
                out.append(ms)
        return stats(out)

    if n == samples:
        res["resample"] = timed(f.resample)
        res["resample+gather"] = timed(lambda: (f.resample(), f.weights_sum()))
    res["stratified"] = timed(lambda: f.resample_stratified(samples))
    res["multinomial"] = timed(lambda: f.resample_multinomial(samples))
    res["multinomial_kept"] = f.count()
    f.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["4194304:4194304", "4194304:1048576", "1048576:4194304"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    ev = Events()
    out = {"tool": "bench_resample", "build_id": eslam_amd.build_id()[:16],
           "sizes": [measure(*(int(v) for v in s.split(":")), args, ev) for s in args.sizes]}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
