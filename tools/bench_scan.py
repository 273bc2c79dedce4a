"""Time the scan MLS build on a 640 x 480 distance image and a 1081-beam laser scan:

    python tools/bench_scan.py [--reps 20] [--out FILE]

Per reading it reports (host clock around the synchronous call; one warm-up call first, which
also sizes the context's scratch, then --reps repeats, median and range):
  build_ms      eslam_gpu_scan_from_depth / eslam_gpu_scan_from_laser: the copy of the reading to
                the device, the point kernel, both sorts, the two walks, the two counts read back
  patches_ms    eslam_gpu_scan_patches: the copy of the patches to the host
  reference_ms  the single-threaded C reference (tests/c/scan_ref.c) on the same input
The readings are the test suite's generators (tests/scan_ref.py) at the benchmark's sizes: a
camera over a floor with a box, a laser line over a stepped floor.  The device's patches are
compared with the reference's before anything is timed.
Prints one JSON line; needs a GPU (no fallback)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eslam_abi as A  # noqa: E402
import eslam_amd  # noqa: E402
import scan_ref as SR  # noqa: E402
import synthetic as S  # noqa: E402


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "reps": len(ms)}


def timed(fn, reps):
    fn()                                     # warm-up: scratch, code objects
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return stats(out)


def measure(f, rd, reps):
    c, _keep = rd.c_reading()
    info = A.ScanInfo()
    call = f.L.eslam_gpu_scan_from_laser if rd.kind == "laser" else f.L.eslam_gpu_scan_from_depth

    def build():
        assert call(f.h, C.byref(c), C.byref(rd.params), C.byref(info)) == 0

    build()
    want, winfo, sizes = SR.reference(rd)
    got = SR.patches_array(f.scan_patches())
    assert info.as_dict() == winfo.as_dict() and got.tobytes() == want.tobytes(), "the device's scan differs from the reference"
    res = {"reading": rd.name, "largest_cluster": int(sizes.max()) if sizes.size else 0}
    res.update(info.as_dict())
    res["build_ms"] = timed(build, reps)
    res["patches_ms"] = timed(f.scan_patches, reps)
    res["reference_ms"] = timed(lambda: SR.reference(rd), max(reps // 4, 3))
    res["speedup"] = round(res["reference_ms"]["median"] / res["build_ms"]["median"], 2)
    return res


def box():
    """the GPU's name (hipDeviceGetName) and the host CPU the reference ran on"""
    name = C.create_string_buffer(256)
    try:
        C.CDLL("libamdhip64.so").hipDeviceGetName(name, 256, 0)
    except OSError:
        pass
    cpu = ""
    try:
        with open("/proc/cpuinfo") as fh:
            cpu = next((ln.split(":", 1)[1].strip() for ln in fh if ln.startswith("model name")), "")
    except OSError:
        pass
    return {"gpu": name.value.decode(errors="replace") or "unnamed", "cpu": cpu}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    readings = [SR.depth_floor("depth_640x480", 640, 480, 21), SR.cases()["laser_1081"]]
    f = eslam_amd.GpuFilter(S.bench_config(A.default_config(), 64), device=0)
    out = {"tool": "bench_scan", "build_id": eslam_amd.build_id()[:16], "box": box(),
           "readings": [measure(f, rd, args.reps) for rd in readings]}
    f.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
