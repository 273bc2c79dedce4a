// eslam_scan.hip -- the scan MLS from a laser scan or a depth image (eslam_gpu_scan_from_laser /
// eslam_gpu_scan_from_depth): what EmbodiedSlamFilter::update(.., LaserScan, ..) and
// update(.., DistanceImage, ..) hand to processMap.  The contract (include/eslam_gpu.h) is a
// sequential rule per cell over its points in the order ((float)z, point index), so a build is
//   k_scan_points   one lane per beam or pixel: the point, its height and variance (dm_scan_place),
//                   its cell (ncell: not binned) and the orderable key of (float)z
//   radix sort      stable, by z key (32 bits), then -- k_scan_cells brings the cells into that
//                   order -- stable by cell (eslam_radix_sort_pairs_passes, as many 8-bit passes as
//                   the cell count needs): cells ascending, inside a cell z ascending, ties by index
//   k_scan_flags / k_scan_excl / k_scan_heads
//                   the first point of every cell's segment, compacted; heights and variances
//                   gathered into canonical order
//   k_scan_patches<0> / k_scan_excl / k_scan_patches<1>
//                   one lane per cell walks its segment: counts its clusters, then writes their
//                   patches at the cell's offset (dm_scan_cluster_len / dm_scan_cluster_patch)
// Nothing depends on the order of atomics (the only atomics add integers into two counters) or on
// how the sort is tiled.  The host reads two words between the stages (the segment count, the
// patch count): the calls are synchronous.  Not on the per-step hot path.
#include <hip/hip_runtime.h>

#include "eslam_internal.h"
#include "eslam_launch.h"
#include "eslam_scratch.h"

namespace eslam_dev {

constexpr int kScanWalkBlock = 64;       // one wave per block: long segments spread over the CUs

template <int DEPTH>
__global__ void __launch_bounds__(kBlock) k_scan_points(dm_scan_frame f, ScanReading rd, uint32_t ncell,
                                                        uint32_t* __restrict__ cell, uint32_t* __restrict__ zkey,
                                                        uint32_t* __restrict__ idx, double* __restrict__ pz,
                                                        double* __restrict__ var, uint64_t* __restrict__ cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    int status = DM_SCAN_VALID;
    bool live = i < rd.n;
    if (live) {
        const uint32_t raw = rd.raw[i];
        double q[3];
        if (DEPTH) {
            const uint32_t v = (uint32_t)(i / rd.width), u = (uint32_t)(i - (uint64_t)v * rd.width);
            status = dm_scan_depth_point(&f, rd.sx, rd.sy, rd.cx, rd.cy, u, v, __uint_as_float(raw), q);
        } else {
            status = dm_scan_laser_point(&f, rd.start_angle, rd.angular_resolution, rd.min_range, rd.max_range, (uint32_t)i,
                                         raw, q);
        }
        double z = 0.0, vr = 1.0;
        uint32_t c = ncell;
        if (status == DM_SCAN_VALID) {
            uint32_t cc;
            if (dm_scan_place(&f, q, &z, &vr, &cc)) c = cc;
            else status = DM_SCAN_OUT_OF_RANGE;          // beyond the grid the host sized (not expected)
        }
        cell[i] = c;
        zkey[i] = dm_scan_zkey(z);
        idx[i] = (uint32_t)i;
        pz[i] = z;
        var[i] = vr;
    }
    const uint64_t binv = __ballot(live && status == DM_SCAN_INVALID);
    const uint64_t boor = __ballot(live && status == DM_SCAN_OUT_OF_RANGE);
    if ((threadIdx.x & 63u) == 0) {
        if (binv) atomicAdd((unsigned long long*)&cnt[kScanInvalid], (unsigned long long)__popcll(binv));
        if (boor) atomicAdd((unsigned long long*)&cnt[kScanOutOfRange], (unsigned long long)__popcll(boor));
    }
}

// out[j] = the cell of the j-th point in z order
__global__ void __launch_bounds__(kBlock) k_scan_cells(const uint32_t* __restrict__ cell, const uint32_t* __restrict__ order,
                                                       uint32_t n, uint32_t* __restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n) out[j] = cell[order[j]];
}

__device__ __forceinline__ bool scan_head(const uint32_t* __restrict__ keys, uint64_t j, uint32_t ncell)
{
    const uint32_t c = keys[j];
    return c != ncell && (j == 0 || keys[j - 1] != c);
}

// flag[j] = sorted point j starts a cell's segment (flag[n] = 0: the scan's total); the heights and
// variances in canonical order
__global__ void __launch_bounds__(kBlock) k_scan_flags(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                                                       uint32_t n, uint32_t ncell, const double* __restrict__ pz,
                                                       const double* __restrict__ var, uint32_t* __restrict__ flag,
                                                       double* __restrict__ sz, double* __restrict__ sv)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j > n) return;
    flag[j] = (j < n && scan_head(keys, j, ncell)) ? 1u : 0u;
    if (j < n) {
        const uint32_t i = order[j];
        sz[j] = pz[i];
        sv[j] = var[i];
    }
}

__global__ void __launch_bounds__(kBlock) k_scan_heads(const uint32_t* __restrict__ keys, uint32_t n, uint32_t ncell,
                                                       const uint32_t* __restrict__ scan, uint32_t* __restrict__ heads)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    if (scan_head(keys, j, ncell)) heads[scan[j]] = (uint32_t)j;
}

// One lane per segment h (its points are sorted positions [heads[h], heads[h + 1]) -- the last
// one's end is nbinned).  EMIT 0: clus[h] = its clusters (clus[nheads] = 0 for the scan).
// EMIT 1: its patches at out[clus[h] ..], clus now the exclusive scan.
template <int EMIT>
__global__ void __launch_bounds__(kScanWalkBlock) k_scan_patches(dm_scan_frame f, const uint32_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ heads, uint32_t nheads,
                                                              uint32_t nbinned, const double* __restrict__ sz,
                                                              const double* __restrict__ sv, uint32_t* __restrict__ clus,
                                                              eslam_scan_patch* __restrict__ out)
{
    for (uint64_t h = (uint64_t)blockIdx.x * kScanWalkBlock + threadIdx.x; h <= nheads; h += (uint64_t)gridDim.x * kScanWalkBlock) {
        if (h == nheads) {
            if (!EMIT) clus[h] = 0u;
            continue;
        }
        const uint32_t j0 = heads[h];
        const uint32_t j1 = h + 1 < nheads ? heads[h + 1] : nbinned;
        const uint32_t len = j1 - j0;
        uint32_t o = EMIT ? clus[h] : 0u;
        double cx = 0.0, cy = 0.0;
        if (EMIT) {
            const uint32_t cell = keys[j0];
            const uint32_t my = cell / f.width, mx = cell - my * f.width;
            cx = dm_scan_cell_centre(&f, mx);
            cy = dm_scan_cell_centre(&f, my);
        }
        uint32_t k = 0, nc = 0;
        while (k < len) {
            const uint32_t l = dm_scan_cluster_len(sz + j0 + k, len - k, f.thickness);
            if (EMIT) {
                double mu, sd;
                dm_scan_cluster_patch(sz + j0 + k, sv + j0 + k, l, &mu, &sd);
                eslam_scan_patch p;
                p.position[0] = cx;
                p.position[1] = cy;
                p.position[2] = mu;
                p.stdev = sd;
                out[o + nc] = p;
            }
            k += l;
            ++nc;
        }
        if (!EMIT) clus[h] = nc;
    }
}

}  // namespace eslam_dev

using namespace eslam_dev;

static uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

// 8-bit passes that order the keys 0 .. ncell
static int scan_passes(uint32_t ncell)
{
    int bits = 1;
    while (bits < 32 && (ncell >> bits)) ++bits;
    return (bits + 7) / 8;
}

// the scratch of a build of n points: its size, and its arrays within `mem` (may be null: size only)
extern "C" size_t eslam_scan_work_bytes(uint64_t n, void* mem, ScanWork* w)
{
    size_t sort_bytes = 0;
    (void)eslam_radix_sort_pairs_passes(nullptr, nullptr, nullptr, nullptr, n, nullptr, &sort_bytes, 4, nullptr);
    eslam_buf::Carver c(mem);
    ScanWork s = {};
    eslam_host::carve_scan(c, n, sort_bytes, &s);
    if (mem && w) *w = s;
    return c.bytes();
}

// stage 1: the points, both sorts, the segment heads.  Afterwards w->b[n] holds the segment count
// and w->cnt the two counters.  n >= 1.
extern "C" hipError_t eslam_launch_scan_order(const dm_scan_frame* f, const ScanReading* rd, const ScanWork* w, hipStream_t stream)
{
    const uint32_t n = rd->n;
    const uint32_t ncell = f->width * f->width;
    hipError_t e = hipMemsetAsync(w->cnt, 0, kScanCounters * 8, stream);
    if (e != hipSuccess) return e;
    if (rd->depth)
        hipLaunchKernelGGL(k_scan_points<1>, dim3(blocks_for(n)), dim3(kBlock), 0, stream, *f, *rd, ncell, w->a, w->b, w->c, w->pz,
                           w->var, w->cnt);
    else
        hipLaunchKernelGGL(k_scan_points<0>, dim3(blocks_for(n)), dim3(kBlock), 0, stream, *f, *rd, ncell, w->a, w->b, w->c, w->pz,
                           w->var, w->cnt);
    size_t tb = w->sort_tmp_bytes;
    e = eslam_radix_sort_pairs_passes(w->b, w->c, w->d, w->e, n, w->sort_tmp, &tb, 4, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_scan_cells, dim3(blocks_for(n)), dim3(kBlock), 0, stream, w->a, w->e, n, w->b);
    tb = w->sort_tmp_bytes;
    e = eslam_radix_sort_pairs_passes(w->b, w->e, w->d, w->c, n, w->sort_tmp, &tb, scan_passes(ncell), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_scan_flags, dim3(blocks_for((uint64_t)n + 1)), dim3(kBlock), 0, stream, w->d, w->c, n, ncell, w->pz, w->var,
                       w->b, w->sz, w->sv);
    e = eslam_launch_scan_excl(w->b, (uint64_t)n + 1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_scan_heads, dim3(blocks_for(n)), dim3(kBlock), 0, stream, w->d, n, ncell, w->b, w->e);
    return hipGetLastError();
}

static uint32_t walk_blocks(uint32_t nheads)
{
    const uint64_t b = ((uint64_t)nheads + 1 + kScanWalkBlock - 1) / kScanWalkBlock;
    return (uint32_t)(b > 4096 ? 4096 : b);
}

// stage 2: the clusters per segment and their exclusive scan; afterwards w->a[nheads] holds the patch count
extern "C" hipError_t eslam_launch_scan_count(const dm_scan_frame* f, const ScanWork* w, uint32_t nheads, uint32_t nbinned,
                                              hipStream_t stream)
{
    hipLaunchKernelGGL(k_scan_patches<0>, dim3(walk_blocks(nheads)), dim3(kScanWalkBlock), 0, stream, *f, w->d, w->e, nheads, nbinned,
                       w->sz, w->sv, w->a, (eslam_scan_patch*)nullptr);
    return eslam_launch_scan_excl(w->a, (uint64_t)nheads + 1, stream);
}

// stage 3: the patches (out has room for w->a[nheads] of them)
extern "C" hipError_t eslam_launch_scan_emit(const dm_scan_frame* f, const ScanWork* w, uint32_t nheads, uint32_t nbinned,
                                             eslam_scan_patch* out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_scan_patches<1>, dim3(walk_blocks(nheads)), dim3(kScanWalkBlock), 0, stream, *f, w->d, w->e, nheads, nbinned,
                       w->sz, w->sv, w->a, out);
    return hipGetLastError();
}
