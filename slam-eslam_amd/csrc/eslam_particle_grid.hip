// eslam_particle_grid.hip -- a particle's whole map as one CSR grid (eslam_gpu_get_particle_grid,
// eslam_gpu_adopt_particle_map).  With per-particle maps the lookup of particle i
// asks its own cell (table X = sid[i]: the window's pages and the trail's) and the shared grid's
// list of the cell (get_patch<DELTA>, eslam_kernels.hip).  The composed grid holds per cell the
// own patch (height 0), then the shared grid's patches in their order, so the first patch of the
// list that passes the 3-sigma gate is the lookup's answer:
//   k_pgrid_dir     X's tiles on the grid as a directory tile -> page (the window's slots by
//                   dm_lm_tile_of, the trail's used entries), filled with DM_LM_NONE before
//   k_pgrid_count   one lane per cell: own + the grid's count, summed per block of 256 cells, and
//                   the own cells' total
//   k_scan_excl     the blocks' starts (a 1000 x 1000 grid: 3 907 sums, one pass of one block)
//   k_pgrid_fill    one lane per cell: its start (the block's + the scan within the block), the
//                   patches, the heights, cell_tab and the occupancy bits
// All of it copies words: no arithmetic on a patch.  A tile is in the window or in the trail, never
// in both (lm_rewrite moves it), and in the trail once, so the directory's writes never collide.
// Not on the per-step hot path.
#include <hip/hip_runtime.h>

#include "eslam_internal.h"
#include "eslam_launch.h"
#include "eslam_scratch.h"

namespace eslam_dev {

// tile (a, b) of the grid, or the directory's size when it is off the grid
__device__ __forceinline__ uint64_t pg_tile(const PgScratch& s, int64_t a, int64_t b)
{
    const uint64_t nt = (uint64_t)s.tx * s.ty;
    return (a >= 0 && a < (int64_t)s.tx && b >= 0 && b < (int64_t)s.ty) ? (uint64_t)b * s.tx + (uint64_t)a : nt;
}

// One lane per window slot, then one per trail entry, of the table *sidp names: its page into
// dir.  The row's padding words (the shadow flag, the trail's high-water mark) are not slots.
__global__ void __launch_bounds__(kBlock) k_pgrid_dir(LocalMaps lm, const uint32_t* __restrict__ sidp, PgScratch s)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t W = lm.wx * lm.wy, toff = lm.S - 4u * lm.V;
    if (t >= W + lm.V) return;
    const uint32_t X = *sidp;
    if (X >= lm.ntables) return;
    const uint32_t* __restrict__ row = lm.slot + (uint64_t)X * lm.S;
    uint32_t pg;
    int64_t a, b;
    if (t < W) {
        const int2 c = lm.ctr[X];
        if (c.x == DM_LM_UNSET || c.y == DM_LM_UNSET) return;      // never centred: no own cells
        pg = row[t];
        a = dm_lm_tile_of(t % lm.wx, c.x, lm.hx, lm.wx);
        b = dm_lm_tile_of(t / lm.wx, c.y, lm.hy, lm.wy);
    } else {
        const uint32_t e = t - W, hwv = row[toff - 1u], hw = hwv == DM_LM_NONE ? 0u : hwv;
        if (e >= hw) return;
        const uint4 v = reinterpret_cast<const uint4*>(row + toff)[e];
        pg = v.z;
        a = (int32_t)v.x;
        b = (int32_t)v.y;
    }
    if (pg == DM_LM_NONE || pg >= lm.npages) return;
    const uint64_t d = pg_tile(s, a, b);
    if (d < (uint64_t)s.tx * s.ty) s.dir[d] = pg;
}

// the own patch of cell (m, n): the page cell of its tile's page, when it holds one
__device__ __forceinline__ bool pg_own(const LocalMaps& lm, const PgScratch& s, uint32_t m, uint32_t n, float2* out)
{
    const uint32_t pg = s.dir[(uint64_t)(n >> DM_LM_TILE_BITS) * s.tx + (m >> DM_LM_TILE_BITS)];
    if (pg == DM_LM_NONE) return false;
    const float2 p = lm.page[(uint64_t)pg * DM_LM_PAGE_CELLS + (m & 7u) + 8u * (n & 7u)];
    *out = p;
    return dm_lm_holds(p.y) != 0;
}

// a wave's inclusive scan of v (lane order)
__device__ __forceinline__ uint32_t pg_wave_incl(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t x = (uint32_t)__shfl_up((int)v, o, 64);
        v += lane >= (uint32_t)o ? x : 0u;
    }
    return v;
}

// One lane per cell (and one for the end of the list): the composed list's length of cell c is
// own + the grid's count.  bsum[block] = the block's cells' total (bsum[blocks] = 0 receives the
// scan's total); *s.own counts the own patches.
__global__ void __launch_bounds__(kBlock) k_pgrid_count(LocalMaps lm, PgScratch s, const uint32_t* __restrict__ cell_start,
                                                        uint32_t width, uint32_t ncell)
{
    __shared__ uint32_t s_w[kWaves];
    const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool own = false;
    uint32_t cnt = 0;
    if (c < ncell) {
        const uint32_t n = (uint32_t)c / width, m = (uint32_t)c - n * width;
        float2 p;
        own = pg_own(lm, s, m, n, &p);
        cnt = (own ? 1u : 0u) + (cell_start[c + 1] - cell_start[c]);
    }
    const uint32_t incl = pg_wave_incl(cnt, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) t += s_w[w];
        s.bsum[blockIdx.x] = t;
        if (blockIdx.x + 1 == gridDim.x) s.bsum[gridDim.x] = 0u;
    }
    const uint64_t b = __ballot(own);
    if (lane == 0 && b) atomicAdd((unsigned long long*)s.own, (unsigned long long)__popcll(b));
}

// The composed arrays, with k_pgrid_count's blocks: a cell's start is its block's (the scanned
// bsum) plus the exclusive scan of the block's counts before it.  Per cell the own patch, then
// the grid's patches with their heights, the 16-byte cell_tab record and, per wave of 64 cells,
// two words of occupancy bits (as k_sm_rebuild writes them).
__global__ void __launch_bounds__(kBlock) k_pgrid_fill(LocalMaps lm, PgScratch s, SmGrid o, SmGrid nw, uint32_t width,
                                                       uint32_t ncell)
{
    __shared__ uint32_t s_w[kWaves];
    const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool occ = false, own = false;
    float2 p = make_float2(0.0f, 0.0f);
    uint32_t ob = 0, old = 0;
    if (c < ncell) {
        const uint32_t n = (uint32_t)c / width, m = (uint32_t)c - n * width;
        own = pg_own(lm, s, m, n, &p);
        ob = o.cell_start[c];
        old = o.cell_start[c + 1] - ob;
    }
    const uint32_t k0 = own ? 1u : 0u, cnt = k0 + old;
    const uint32_t incl = pg_wave_incl(cnt, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t nb = s.bsum[blockIdx.x] + (incl - cnt);
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kWaves; ++w) nb += w < wave ? s_w[w] : 0u;
    if (c < ncell) {
        nw.cell_start[c] = nb;
        if (own) {
            nw.patch[nb] = p;
            if (nw.height) nw.height[nb] = 0.0f;
        }
        for (uint32_t q = 0; q < old; ++q) {
            nw.patch[nb + k0 + q] = o.patch[ob + q];
            if (nw.height) nw.height[nb + k0 + q] = o.height[ob + q];
        }
        const uint32_t total = k0 + old;
        const float2 f = own ? p : (old ? o.patch[ob] : make_float2(0.0f, 0.0f));
        nw.cell_tab[c] = make_uint4(__float_as_uint(f.x), __float_as_uint(f.y), nb, total);
        occ = total != 0;
    } else if (c == ncell) {
        nw.cell_start[c] = nb;               // every cell lies before it: the total
    }
    const uint64_t bits = __ballot(occ);
    const uint64_t nwords = ((uint64_t)ncell + 31) / 32;
    if ((lane & 31u) == 0 && (c >> 5) < nwords) nw.occ[c >> 5] = (uint32_t)(bits >> lane);
}

}  // namespace eslam_dev

using namespace eslam_dev;

static uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

extern "C" size_t eslam_pgrid_work_bytes(uint32_t width, uint32_t height, void* mem, PgScratch* s)
{
    const uint64_t tx = ((uint64_t)width + 7) / 8, ty = ((uint64_t)height + 7) / 8, ncell = (uint64_t)width * height;
    const uint64_t blocks = blocks_for(ncell + 1);
    eslam_buf::Carver c(mem);
    PgScratch p = {};
    eslam_host::carve_pgrid(c, tx, ty, blocks, &p);
    if (mem && s) *s = p;
    return c.bytes();
}

// the directory of the table *sidp names, the blocks' composed counts in s->bsum and the own
// patches' total in *s->own
extern "C" hipError_t eslam_launch_pgrid_count(const LocalMaps* lm, const uint32_t* sidp, const MapView* map, const PgScratch* s,
                                               hipStream_t stream)
{
    const uint64_t ncell = (uint64_t)map->width * map->height_cells;
    hipError_t e = hipMemsetAsync(s->dir, 0xff, (size_t)s->tx * s->ty * 4, stream);      // DM_LM_NONE
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(s->own, 0, 8, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pgrid_dir, dim3(blocks_for((uint64_t)lm->wx * lm->wy + lm->V)), dim3(kBlock), 0, stream, *lm, sidp, *s);
    hipLaunchKernelGGL(k_pgrid_count, dim3(blocks_for(ncell + 1)), dim3(kBlock), 0, stream, *lm, *s, map->cell_start, map->width,
                       (uint32_t)ncell);
    return hipGetLastError();
}

// after eslam_launch_pgrid_count: the scan of the block sums, then the composed grid into `out`,
// whose patch arrays hold at least cur's patches + *s->own
extern "C" hipError_t eslam_launch_pgrid_fill(const LocalMaps* lm, const MapView* map, const PgScratch* s, const SmGrid* cur,
                                              const SmGrid* out, hipStream_t stream)
{
    const uint64_t ncell = (uint64_t)map->width * map->height_cells;
    const hipError_t e = eslam_launch_scan_excl(s->bsum, (uint64_t)blocks_for(ncell + 1) + 1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pgrid_fill, dim3(blocks_for(ncell + 1)), dim3(kBlock), 0, stream, *lm, *s, *cur, *out, map->width,
                       (uint32_t)ncell);
    return hipGetLastError();
}
