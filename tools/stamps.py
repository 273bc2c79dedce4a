"""Phase timeline of K1 and K3 from a -DESLAM_STAMPS diagnostic build (s_memrealtime, 10 ns):
    ESLAM_GPU_LIB=$PWD/slam-eslam_amd/lib/ab/lib_stamps.so python tools/stamps.py [particles] [warmup]
(a build with -DESLAM_DRAW_STATS as well also reports how many waves of the last step counted
their stratified draws in integers and how many evaluated them; its timeline is disturbed)
Runs the bench workload (flat map, resample forced) for `warmup` steps plus one, then prints,
per phase of the last step's K1 and K3 (the stamps are cleared before it, and the block
counts are the launches' own), the median / max block duration and when the last block left
the phase (from the kernel's first block start).  Read the shares, not the
lengths: the stamps' waits make the build slower than the product.
K1 also stamps every wave (start, first row, last row done, and where it ran): the report adds
the distribution of the waves' end times, per SIMD the end time by start rank, and the
resident-wave count over time.  For K1 at the product's five waves per SIMD build with
-DESLAM_STAMPS -DESLAM_K1_WPE=5 (the stamps alone take the bench instantiation to 98 VGPRs)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))

import eslam_abi as A  # noqa: E402
import eslam_amd  # noqa: E402
import synthetic as S  # noqa: E402

K1_PHASES = ["start", "window staged", "rows done", "stats flushed"]
K3_PHASES = ["start", "phase-B loads issued", "finalize seen", "phase B applied", "tile scanned",
             "look-back done", "draws counted", "marks written"]


def report(name, st, phases, nblocks):
    st = st[:nblocks, :len(phases)].astype(np.int64)
    done = np.all(st > 0, axis=1)                # blocks that returned early left zeros (cleared)
    st = st[done]
    if not len(st):
        print(f"== {name}: no block passed every phase")
        return
    t0 = st[:, 0].min()
    rel = (st - t0) * 10e-3                      # us
    print(f"== {name}: {nblocks} blocks ({len(st)} through every phase), span {rel[:, -1].max():.2f} us "
          "(first start to last end)")
    for k in range(1, len(phases)):
        d = rel[:, k] - rel[:, k - 1]
        print(f"  {phases[k - 1]:>22s} -> {phases[k]:<22s} median {np.median(d):7.2f}  p90 {np.percentile(d, 90):7.2f}"
              f"  max {d.max():7.2f} us; last block leaves at {rel[:, k].max():7.2f} us")
    starts = rel[:, 0]
    print(f"  block starts: median {np.median(starts):.2f}, p90 {np.percentile(starts, 90):.2f}, last {starts.max():.2f} us")


def pct(v, qs=(0, 10, 25, 50, 75, 90, 100)):
    return "  ".join(f"p{q}={np.percentile(v, q):.2f}" for q in qs)


def report_waves(name, ws, nblocks):
    """K1's per-wave stamps (start, first row starts, last row done, placement): when the waves
    end, how a SIMD's waves end by the order in which they started, and how many waves are
    resident over time.  Times in us from the first wave's start; a wave counts as resident
    from its start to the end of its last row (the block's flush after it is not stamped per
    wave).  Placement: HW_ID wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13], and
    XCC_ID [3:0] in the upper word."""
    ws = ws[:nblocks * 4].astype(np.int64)
    ran = np.all(ws[:, :3] > 0, axis=1)              # a wave without a chunk stamps its start only
    ws = ws[ran]
    if not len(ws):
        print(f"== {name}: no wave stamped its rows")
        return
    t0 = ws[:, 0].min()
    start, rows0, end = ((ws[:, k] - t0) * 10e-3 for k in range(3))
    hw, xcc = ws[:, 3] & 0xffffffff, (ws[:, 3] >> 32) & 0xf
    simd = (xcc << 16) | (hw & 0xff30)               # XCC, SE, SH, CU, SIMD
    span = end.max()
    life = end - start
    print(f"== {name}: {len(ws)} waves with rows, span {span:.2f} us; mean wave lifetime {life.mean():.2f} us "
          f"= {life.mean() / span:.3f} of the span")
    print(f"  wave starts       {pct(start)}")
    print(f"  first row starts  {pct(rows0)}")
    print(f"  wave ends         {pct(end)}")
    print(f"  rows phase        {pct(end - rows0)}")
    keys, inv, counts = np.unique(simd, return_inverse=True, return_counts=True)
    hist = {int(c): int(np.count_nonzero(counts == c)) for c in np.unique(counts)}
    print(f"  {len(keys)} SIMDs seen (XCC, SE, SH, CU, SIMD); waves per SIMD -> SIMDs: {hist}")
    depth = int(np.bincount(counts).argmax())        # the usual number of waves a SIMD ran
    by_rank = [[] for _ in range(depth)]
    spread, gens = [], 0
    for s in np.nonzero(counts == depth)[0]:
        idx = np.nonzero(inv == s)[0]
        idx = idx[np.argsort(start[idx], kind="stable")]
        if np.any(start[idx][1:] >= end[idx].min()):  # a later generation refilled a slot
            gens += 1
            continue
        for r, i in enumerate(idx):
            by_rank[r].append(end[i])
        spread.append(end[idx].max() - end[idx].min())
    if spread:
        print(f"  per SIMD with {depth} waves of one generation ({len(spread)} SIMDs; {gens} with a refill left out), "
              "end by start rank, oldest first, median over SIMDs:")
        print("    " + "  ".join(f"#{r}={np.median(v):.2f}" for r, v in enumerate(by_rank)))
        fin = np.array([np.sort([by_rank[r][k] for r in range(depth)]) for k in range(len(spread))])
        print("    end by finishing order, median over SIMDs: " + "  ".join(f"{np.median(fin[:, r]):.2f}" for r in range(depth)))
        print(f"    first-to-last end within a SIMD: {pct(np.array(spread), (10, 50, 90, 100))} us")
    print("  resident waves over time (all, and per SIMD seen):")
    for t in np.linspace(0.0, span, 17)[1:-1]:
        r = int(np.count_nonzero((start <= t) & (end > t)))
        print(f"    t={t:7.2f} us  {r:6d}  {r / len(keys):.2f}")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4 * 1024 * 1024
    warm = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    L = eslam_amd.load_library()
    L.eslam_gpu_debug_stamps.argtypes = [C.c_int, C.c_void_p, C.c_uint64]
    L.eslam_gpu_debug_stamps.restype = C.c_int64
    cfg = S.bench_config(A.default_config(), n)
    f = eslam_amd.GpuFilter(cfg, device=0)
    f.set_map(S.flat_map())
    f.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)
    steps = list(S.step_stream(warm + 1))
    for st in steps[:-1]:
        f.step(st)
    f.sync()
    assert L.eslam_gpu_debug_stamps_clear() == 0  # the measured step's stamps only
    stats = hasattr(L, "eslam_gpu_debug_draw_waves")       # a -DESLAM_DRAW_STATS build as well
    waves = (C.c_uint32 * 2)()
    if stats:
        assert L.eslam_gpu_debug_draw_waves(waves, 1) == 0
    f.step(steps[-1])
    f.sync()
    buf = np.zeros((32768, 8), dtype=np.uint64)
    for which, label, phases in ((1, "K1", K1_PHASES), (3, "K3", K3_PHASES)):
        blocks = L.eslam_gpu_debug_stamps(which, buf.ctypes.data, 32768)
        assert blocks >= 0
        report(f"{label} at n={n} ({blocks} blocks launched)", buf.copy(), phases, min(blocks, 32768))
    if hasattr(L, "eslam_gpu_debug_stamps_k1_waves"):
        L.eslam_gpu_debug_stamps_k1_waves.argtypes = [C.c_void_p, C.c_uint64]
        L.eslam_gpu_debug_stamps_k1_waves.restype = C.c_int64
        wbuf = np.zeros((32768 * 4, 4), dtype=np.uint64)
        blocks = L.eslam_gpu_debug_stamps_k1_waves(wbuf.ctypes.data, 32768 * 4)
        assert blocks >= 0
        report_waves(f"K1 waves at n={n}", wbuf, min(blocks, 32768))
    if stats:
        assert L.eslam_gpu_debug_draw_waves(waves, 0) == 0
        print(f"== draw counting of the last step: {waves[0]} waves, {waves[1]} of them evaluated their draws")
    f.close()


if __name__ == "__main__":
    main()
