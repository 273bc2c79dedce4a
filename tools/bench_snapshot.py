"""Time eslam_gpu_save_stream / eslam_gpu_load_stream on the configs[4] workload of
`bench.py --local-maps` (rough terrain unmapped beyond x = 0.3 m, tilted body, a 48-patch scan
merged into every particle's map after every step), after --steps steps:

    python tools/bench_snapshot.py --particles 1048576 [--chunk-mib 64] [--reps 5] [--out FILE]

Per size it reports (host clock around calls that end in a device synchronise; one warm-up call
first, then --reps repeats, median and range):
  census_ms     eslam_gpu_snapshot_size: the pending gather's no-op, the two censuses, the counts
  save_ms       eslam_gpu_save_stream into a callback that discards the chunks
  floor_ms      plain hipMemcpy device -> pinned host of the same number of bytes in chunks of
                the same size, from the same process: the floor a save is measured against
  load_ms       eslam_gpu_load from memory into a second, freshly created context
  baseline      eslam_gpu_get_particle_map on --baseline-particles particles of a 64k filter,
                per particle (the only way out the library had before), extrapolated
The pack kernels' and the copies' own times come from a run of this tool under
`rocprofv3 --kernel-trace --memory-copy-trace --stats` (k_snap_* kernels), not from this clock.
With --at it measures the positional forms instead, on the same state and in one process:
  save_stream_ms / save_at_ms   both into discarding callbacks, alternating
  load_stream_ms / load_at_ms   the whole blob from memory into a second context (the full range)
  subset_load_ms                eslam_gpu_load_at of the first half of the particles: a context that is
                                rank 0 of a 2-rank layout whose peer only answers the all_gathers, with
                                the time spent inside the read callbacks and their count; to be set
                                against load_at_ms, the same blob loaded whole
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

import numpy as np  # noqa: E402

import eslam_abi as A  # noqa: E402
import eslam_amd  # noqa: E402
import synthetic as S  # noqa: E402


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "reps": len(ms)}


def timed(fn, reps):
    fn()                                     # warm-up: staging buffers, code objects
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return stats(out)


def run_filter(n, steps, map_cells, pages):
    cfg = S.bench_config(A.default_config(), n)
    cfg.flags |= A.FLAG_PARTICLE_MAPS
    cfg.local_map_pages = pages
    grid = S.unmapped_beyond(S.rough_map(cells=map_cells), 0.3)
    scan = S.scan_patches()
    f = eslam_amd.GpuFilter(cfg, device=0)
    f.set_map(grid)
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)
    for st in S.step_stream(steps, tilt=True):
        f.step(st)
        f.map_update(scan)
    f.sync()
    return cfg, f


def memcpy_floor(total, chunk, reps):
    """hipMemcpy device -> pinned host of `total` bytes in chunks of `chunk`"""
    hip = C.CDLL("libamdhip64.so")
    dev, host = C.c_void_p(), C.c_void_p()
    size = min(chunk, total)
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(size)) == 0 and hip.hipHostMalloc(C.byref(host), C.c_size_t(size), 0) == 0
    assert hip.hipMemset(dev, 1, C.c_size_t(size)) == 0

    def copy():
        left = total
        while left > 0:
            b = min(size, left)
            assert hip.hipMemcpy(host, dev, C.c_size_t(b), 2) == 0        # hipMemcpyDeviceToHost
            left -= b

    r = timed(copy, reps)
    hip.hipFree(dev)
    hip.hipHostFree(host)
    return r


def measure(n, args):
    cfg, f = run_filter(n, args.steps, args.map_cells, args.map_pages)
    chunk = args.chunk_mib << 20
    info = f.snapshot_info()
    res = {"particles": n, "steps": args.steps, "chunk_bytes": chunk, "bytes": info.bytes, "tables": info.tables, "pages": info.pages,
           "pages_per_particle": round(info.pages / n, 3)}
    res["census_ms"] = timed(f.snapshot_info, args.reps)
    sink = A.WRITE_FN(lambda user, data, nbytes: 0)
    sinfo = A.SnapshotInfo()

    def save():
        assert f.L.eslam_gpu_save_stream(f.h, sink, None, chunk, C.byref(sinfo)) == 0

    res["save_ms"] = timed(save, args.reps)
    res["chunks"] = sinfo.chunks
    res["floor_ms"] = memcpy_floor(info.bytes, chunk, args.reps)
    res["save_GBps"] = round(info.bytes / res["save_ms"]["median"] / 1e6, 2)
    res["floor_GBps"] = round(info.bytes / res["floor_ms"]["median"] / 1e6, 2)
    if args.load:
        blob = f.save_state(chunk_bytes=chunk)
        f.close()                            # the restored context takes the saved one's place
        g = eslam_amd.GpuFilter(cfg, device=0)
        res["load_ms"] = timed(lambda: g.load_state(blob, chunk_bytes=chunk), max(args.reps // 2, 1))
        res["load_GBps"] = round(info.bytes / res["load_ms"]["median"] / 1e6, 2)
        g.close()
    else:
        f.close()
    return res


class HalfComm:
    """rank 0 of 2; the absent peer answers every all_gather with zeros (no error, nothing to add)"""
    rank, nranks, device_memory, error = 0, 2, False, None

    def __init__(self):
        def allgather(user, send, recv, n, stream):
            C.memmove(recv, send, n)
            C.memset(recv + n, 0, n)
            return 0

        self._ag = A.ALLGATHER_FN(allgather)
        self._a2a = A.ALLTOALLV_FN(lambda user, send, sb, recv, rb, stream: 1)
        self.struct = A.Comm(None, 0, 2, 0, 0, self._ag, self._a2a)


def measure_at(n, args):
    import eslam_dist
    cfg, f = run_filter(n, args.steps, args.map_cells, args.map_pages)
    chunk = args.chunk_mib << 20
    info = f.snapshot_info()
    res = {"particles": n, "steps": args.steps, "chunk_bytes": chunk, "bytes": info.bytes, "tables": info.tables, "pages": info.pages}
    sinfo = A.SnapshotInfo()
    sink = A.WRITE_FN(lambda user, data, nbytes: 0)
    psink = A.PWRITE_FN(lambda user, off, data, nbytes: 0)

    def save_stream():
        assert f.L.eslam_gpu_save_stream(f.h, sink, None, chunk, C.byref(sinfo)) == 0

    def save_at():
        assert f.L.eslam_gpu_save_at(f.h, psink, None, chunk, C.byref(sinfo)) == 0

    # alternating, so that neither form has the warmer machine
    a, b = [], []
    save_stream()
    save_at()
    for _ in range(args.reps):
        for fn, out in ((save_stream, a), (save_at, b)):
            t = time.perf_counter()
            fn()
            out.append(1e3 * (time.perf_counter() - t))
    res["save_stream_ms"], res["save_at_ms"] = stats(a), stats(b)
    blob = f.save_state(chunk_bytes=chunk)
    f.close()
    base = blob.ctypes.data
    spent = [0.0, 0]

    def pread(user, off, data, nbytes):
        t = time.perf_counter()
        C.memmove(data, base + off, nbytes)
        spent[0] += time.perf_counter() - t
        spent[1] += 1
        return 0

    src = A.PREAD_FN(pread)
    reps = args.reps
    g = eslam_amd.GpuFilter(cfg, device=0)

    def load_at(h=None):
        assert g.L.eslam_gpu_load_at(h or g.h, src, None, blob.shape[0], chunk, C.byref(sinfo)) == 0

    res["load_stream_ms"] = timed(lambda: g.load_state(blob, chunk_bytes=chunk), reps)
    res["load_at_ms"] = timed(load_at, reps)
    g.close()
    # the subset path: the first half of the particles
    hcfg = S.bench_config(A.default_config(), n)
    hcfg.flags, hcfg.local_map_pages = cfg.flags, cfg.local_map_pages
    h = eslam_dist.ShardedGpuFilter(hcfg, n, HalfComm(), device=0)
    load_at(h.f.h)                           # warm-up
    spent[0], spent[1] = 0.0, 0
    res["subset_load_ms"] = timed(lambda: load_at(h.f.h), reps)
    res["subset"] = {"particles": h.n_local, "read_callbacks_per_load": spent[1] // (reps + 1),
                     "ms_in_read_callbacks_per_load": round(1e3 * spent[0] / (reps + 1), 3),
                     "kernel_split": "not measured by this clock (rocprofv3 --kernel-trace: k_snap_mark_*, k_snap_popc, k_snap_rank_sid, "
                                     "k_snap_renumber_tables)"}
    h.f.close()
    return res


def baseline(args):
    n = 65536
    cfg, f = run_filter(n, args.steps, args.map_cells, args.map_pages)
    idx = np.linspace(0, n - 1, args.baseline_particles).astype(np.int64)
    f.particle_map(0)
    t = time.perf_counter()
    for i in idx:
        f.particle_map(int(i))
    ms = 1e3 * (time.perf_counter() - t) / len(idx)
    f.close()
    return {"filter": n, "sampled": len(idx), "ms_per_particle": round(ms, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, nargs="+", default=[1048576])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--map-cells", type=int, default=1000)
    ap.add_argument("--map-pages", type=int, default=0)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-load", dest="load", action="store_false")
    ap.add_argument("--baseline-particles", type=int, default=256, help="0: skip the get_particle_map baseline")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--at", action="store_true", help="the positional forms (eslam_gpu_save_at / eslam_gpu_load_at) and the subset load")
    args = ap.parse_args()
    if args.at:
        args.baseline_particles = 0
    out = {"tool": "bench_snapshot", "build_id": eslam_amd.build_id()[:16],
           "sizes": [(measure_at if args.at else measure)(n, args) for n in args.particles]}
    if args.baseline_particles:
        out["get_particle_map_baseline"] = b = baseline(args)
        for r in out["sizes"]:
            r["baseline_extrapolated_s"] = round(b["ms_per_particle"] * r["particles"] / 1e3, 1)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
