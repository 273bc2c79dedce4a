// eslam_shared_map.hip -- processMap's merge into the shared grid (useSharedMap = true;
// eslam_gpu_shared_map_update).  The contract is a sequential loop over
// (particle, patch) pairs; a cell's result depends only on the pairs that land on it, in that
// order, so a run of particles is merged as
//   k_sm_place    one thread per record: the cell it lands on (ncell: not placed), in record order
//   radix sort    stable, by cell (eslam_radix_sort_pairs_passes): a cell's records stay in order
//   k_sm_flags / k_scan_excl / k_sm_heads
//                 the first record of every touched cell's segment, compacted
//   k_sm_apply    one lane per touched cell walks its segment in order: fuses in place, appends
//                 to the segment's own slice of the scratch (a segment of L records appends <= L)
//   k_sm_counts / k_scan_excl / k_sm_rebuild
//                 the new CSR (old patches, then the appended ones), cell_tab and occ
// No step depends on the order of atomics: the only atomics add integers into counters.  The
// chain of one cell is serial by contract (the fp32-rounded fuse is not associative), so a
// concentrated cloud leaves few lanes with long segments; speed was not the goal here.
// Not on the per-step hot path.
// A sharded filter (eslam_gpu_shared_map_update_sharded) runs the same pipeline on every rank's
// copy of the grid: k_sm_stage packs the rank's part of a run as 40-byte pose records, the
// ranks exchange them, and the kGath instantiations of k_sm_place / k_sm_apply read particle ip
// of the run from the gathered records (SmRun::gath: s0.x names them) instead of the rank's own
// columns.  The parameter lists are the same, so the one-context instantiations are the code
// they were before the gathered form existed.
#include <hip/hip_runtime.h>

#include "eslam_internal.h"
#include "eslam_launch.h"

namespace eslam_dev {

constexpr int kSmApplyBlock = 64;        // one wave per block: long segments spread over the CUs

// record r of the run: its cell in keys[r] (run.ncell when the particle is skipped or the patch
// falls off the grid), r itself in vals[r].  The placement is eslam_gpu_map_update's.
// kGath: particle ip's pose is the run's gathered record ip (s0.x: SmRun::gath), not column i0 + ip.
template <bool kGath>
__global__ void __launch_bounds__(kBlock) k_sm_place(DevState s0, DevState s1, const Ctl* __restrict__ ctl, MapView map,
                                                     SmRun run, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                     uint64_t* __restrict__ cnt)
{
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool placed = false;
    if (r < run.R) {
        const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
        const uint64_t ip = r / run.P;
        const uint32_t k = (uint32_t)(r - ip * run.P);
        const uint64_t i = run.i0 + ip;
        const double* pose = kGath ? s0.x + ip * kSmPoseWords : nullptr;
        const double x = kGath ? pose[0] : st.x[i], y = kGath ? pose[1] : st.y[i], th = kGath ? pose[2] : st.th[i];
        const double bx = x - map.offset_x, by = y - map.offset_y;
        uint32_t cell = 0xffffffffu;
        if (dm_isfinite(bx) && dm_isfinite(by) && dm_isfinite(th)) {
            double sn, co;
            dm_sincos(th, &sn, &co);
            const ScanPatch sp = run.sp[k];
            uint32_t cm, cn;
            if (run.is_id) {
                cell = dm_merge_cell_mn(bx, by, co, sn, sp.x, sp.y, map.inv_scale_x, map.inv_scale_y, map.width,
                                        map.height_cells, &cm, &cn);
            } else {
                const double* A = map.g2l;
                const double wz = sp.z + (kGath ? pose[3] : st.z[i]);
                const double wx = (co * sp.x + (-sn) * sp.y) + x;
                const double wy = (sn * sp.x + co * sp.y) + y;
                const double lx = ((A[0] * wx + A[1] * wy) + A[2] * wz) + A[3];
                const double ly = ((A[4] * wx + A[5] * wy) + A[6] * wz) + A[7];
                const double fm = floor((lx - map.offset_x) * map.inv_scale_x);
                const double fn = floor((ly - map.offset_y) * map.inv_scale_y);
                if ((fm >= 0.0) & (fm < (double)map.width) & (fn >= 0.0) & (fn < (double)map.height_cells))
                    cell = (uint32_t)fn * map.width + (uint32_t)fm;
            }
        }
        placed = cell != 0xffffffffu;
        keys[r] = placed ? cell : run.ncell;
        vals[r] = (uint32_t)r;
    }
    const uint64_t b = __ballot(placed);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd((unsigned long long*)&cnt[kSmRunPlaced], (unsigned long long)__popcll(b));
}

__device__ __forceinline__ bool sm_head(const uint32_t* __restrict__ keys, uint64_t j, uint32_t ncell)
{
    const uint32_t c = keys[j];
    return c != ncell && (j == 0 || keys[j - 1] != c);
}

// flag[j] = sorted record j starts a touched cell's segment (flag[R] = 0: the scan's total)
__global__ void __launch_bounds__(kBlock) k_sm_flags(const uint32_t* __restrict__ keys, uint64_t R, uint32_t ncell,
                                                     uint32_t* __restrict__ flag)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j > R) return;
    flag[j] = (j < R && sm_head(keys, j, ncell)) ? 1u : 0u;
}

// heads[h] = the h-th segment's first sorted record (scan: the exclusive scan of the flags)
__global__ void __launch_bounds__(kBlock) k_sm_heads(const uint32_t* __restrict__ keys, uint64_t R, uint32_t ncell,
                                                     const uint32_t* __restrict__ scan, uint32_t* __restrict__ heads)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= R) return;
    if (sm_head(keys, j, ncell)) heads[scan[j]] = (uint32_t)j;
}

// One lane per touched cell: its records in sorted (= record) order against the cell's list,
// the grid's patches (fused in place) and then the patches this segment appended (app[j0 ..]).
// No other lane reads or writes this cell's patches or this slice of app.
template <bool kGath>
__global__ void __launch_bounds__(kSmApplyBlock) k_sm_apply(DevState s0, DevState s1, const Ctl* __restrict__ ctl, SmRun run,
                                                            SmGrid g, const uint32_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ order,
                                                            const uint32_t* __restrict__ heads,
                                                            const uint32_t* __restrict__ nheads_p, float2* app,
                                                            uint32_t* __restrict__ add, uint32_t* __restrict__ segpos,
                                                            uint32_t* __restrict__ touched, uint64_t* __restrict__ cnt)
{
    const uint32_t nheads = *nheads_p;
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    uint32_t fused = 0, absorbed = 0, inserted = 0, cells = 0;
    for (uint64_t h = (uint64_t)blockIdx.x * kSmApplyBlock + threadIdx.x; h < nheads; h += (uint64_t)gridDim.x * kSmApplyBlock) {
        const uint64_t j0 = heads[h];
        const uint32_t cell = keys[j0];
        const uint32_t b = g.cell_start[cell], e = g.cell_start[cell + 1];
        uint32_t napp = 0;
        for (uint64_t j = j0; j < run.R && keys[j] == cell; ++j) {
            const uint32_t r = order[j];
            const uint32_t ip = r / run.P, k = r - ip * run.P;
            const uint64_t i = run.i0 + ip;
            const ScanPatch sp = run.sp[k];
            const double* pose = kGath ? s0.x + (uint64_t)ip * kSmPoseWords : nullptr;
            const double zs = kGath ? pose[4] : st.zs[i];
            const double wz = sp.z + (kGath ? pose[3] : st.z[i]);
            const double var = sp.stdev * sp.stdev + zs * zs;
            bool taken = false;
            for (uint32_t q = b; q < e && !taken; ++q) {
                const float2 p = g.patch[q];
                const float ph = g.height ? g.height[q] : 0.0f;
                if (!dm_mls_gate(p.x, p.y, ph, wz, var)) continue;
                taken = true;
                float mo, so;
                if (!(ph > 0.0f) && dm_lm_fuse(p.x, p.y, wz, var, &mo, &so)) {
                    g.patch[q] = make_float2(mo, so);
                    ++fused;
                } else {
                    ++absorbed;
                }
            }
            for (uint32_t t = 0; t < napp && !taken; ++t) {
                const float2 p = app[j0 + t];
                if (!dm_mls_gate(p.x, p.y, 0.0f, wz, var)) continue;
                taken = true;
                float mo, so;
                if (dm_lm_fuse(p.x, p.y, wz, var, &mo, &so)) {
                    app[j0 + t] = make_float2(mo, so);
                    ++fused;
                } else {
                    ++absorbed;
                }
            }
            if (!taken) {
                app[j0 + napp] = make_float2((float)wz, (float)dm_sqrt(var));
                ++napp;
                ++inserted;
            }
        }
        add[cell] = napp;
        segpos[cell] = (uint32_t)j0;
        cells += touched[cell] == 0u;
        touched[cell] = 1u;
    }
    if (fused) atomicAdd((unsigned long long*)&cnt[kSmFused], (unsigned long long)fused);
    if (absorbed) atomicAdd((unsigned long long*)&cnt[kSmAbsorbed], (unsigned long long)absorbed);
    if (inserted) atomicAdd((unsigned long long*)&cnt[kSmInserted], (unsigned long long)inserted);
    if (cells) atomicAdd((unsigned long long*)&cnt[kSmTouched], (unsigned long long)cells);
}

// A sharded run's send buffer: particles [first, first + cnt) of this rank's current buffer as
// 40-byte records {x, y, theta, zPos, zSigma}, one copy per rank (the all_to_all_v sends every
// rank the same block).  One lane per particle: a wave's loads of a column are consecutive.
__global__ void __launch_bounds__(kBlock) k_sm_stage(DevState s0, DevState s1, const Ctl* __restrict__ ctl, uint64_t first,
                                                     uint64_t cnt, uint32_t copies, double* __restrict__ out)
{
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= cnt) return;
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    const uint64_t i = first + t;
    const double x = st.x[i], y = st.y[i], th = st.th[i], z = st.z[i], zs = st.zs[i];
    for (uint32_t c = 0; c < copies; ++c) {
        double* o = out + ((uint64_t)c * cnt + t) * kSmPoseWords;
        o[0] = x; o[1] = y; o[2] = th; o[3] = z; o[4] = zs;
    }
}

// the new cell sizes, ready for the exclusive scan (out[ncell] = 0 receives the total)
__global__ void __launch_bounds__(kBlock) k_sm_counts(const uint32_t* __restrict__ cell_start, const uint32_t* __restrict__ add,
                                                      uint32_t ncell, uint32_t* __restrict__ out)
{
    const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c > ncell) return;
    out[c] = c < ncell ? (cell_start[c + 1] - cell_start[c]) + add[c] : 0u;
}

// the new arrays: per cell its old patches, then the run's appended ones (height 0), the
// 16-byte cell_tab record and, per wave of 64 cells, two words of occupancy bits
__global__ void __launch_bounds__(kBlock) k_sm_rebuild(SmGrid o, SmGrid nw, const uint32_t* __restrict__ add,
                                                       const uint32_t* __restrict__ segpos, const float2* __restrict__ app,
                                                       uint32_t ncell)
{
    const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    bool occ = false;
    if (c < ncell) {
        const uint32_t ob = o.cell_start[c], old = o.cell_start[c + 1] - ob;
        const uint32_t nb = nw.cell_start[c], na = add[c];
        for (uint32_t q = 0; q < old; ++q) {
            nw.patch[nb + q] = o.patch[ob + q];
            if (nw.height) nw.height[nb + q] = o.height[ob + q];
        }
        if (na) {
            const uint32_t j0 = segpos[c];
            for (uint32_t t = 0; t < na; ++t) {
                nw.patch[nb + old + t] = app[j0 + t];
                if (nw.height) nw.height[nb + old + t] = 0.0f;
            }
        }
        const uint32_t total = old + na;
        const float2 f = old ? o.patch[ob] : (na ? app[segpos[c]] : make_float2(0.0f, 0.0f));
        nw.cell_tab[c] = make_uint4(__float_as_uint(f.x), __float_as_uint(f.y), nb, total);
        occ = total != 0;
    }
    const uint64_t bits = __ballot(occ);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwords = ((uint64_t)ncell + 31) / 32;
    if ((lane & 31u) == 0 && (c >> 5) < nwords) nw.occ[c >> 5] = (uint32_t)(bits >> lane);
}

}  // namespace eslam_dev

using namespace eslam_dev;

static uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

// 8-bit passes that order the keys 0 .. ncell
static int sm_passes(uint32_t ncell)
{
    int bits = 1;
    while (bits < 32 && (ncell >> bits)) ++bits;
    return (bits + 7) / 8;
}

extern "C" size_t eslam_sm_sort_bytes(uint64_t records)
{
    size_t b = 0;
    (void)eslam_radix_sort_pairs_passes(nullptr, nullptr, nullptr, nullptr, records, nullptr, &b, 4, nullptr);
    return b;
}

// a sharded run's pose records: this rank's particles [first, first + cnt) (cnt > 0), `copies` times
extern "C" hipError_t eslam_launch_sm_stage(DevState s0, DevState s1, const Ctl* ctl, uint64_t first, uint64_t cnt,
                                            uint32_t copies, double* out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_sm_stage, dim3(blocks_for(cnt)), dim3(kBlock), 0, stream, s0, s1, ctl, first, cnt, copies, out);
    return hipGetLastError();
}

// (a) the records' cells; cnt[kSmRunPlaced] (zeroed here) receives the run's placed count
extern "C" hipError_t eslam_launch_sm_place(DevState s0, DevState s1, const Ctl* ctl, const MapView* map, const SmRun* run,
                                            const SmScratch* s, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(s->cnt + kSmRunPlaced, 0, sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    if (run->gath)
        hipLaunchKernelGGL(k_sm_place<true>, dim3(blocks_for(run->R)), dim3(kBlock), 0, stream, s0, s1, ctl, *map, *run, s->keys,
                           s->vals, s->cnt);
    else
        hipLaunchKernelGGL(k_sm_place<false>, dim3(blocks_for(run->R)), dim3(kBlock), 0, stream, s0, s1, ctl, *map, *run, s->keys,
                           s->vals, s->cnt);
    return hipGetLastError();
}

// (b) - (e) of a run with placed records: sort, heads, apply on `cur` (fuses in place), rebuild
// into `next` (whose patch arrays hold at least cur's patches + the run's placed records)
extern "C" hipError_t eslam_launch_sm_merge(DevState s0, DevState s1, const Ctl* ctl, const SmRun* run, const SmGrid* cur,
                                            const SmGrid* next, const SmScratch* s, hipStream_t stream)
{
    const uint64_t R = run->R;
    const uint32_t ncell = run->ncell;
    hipError_t e = hipMemsetAsync(s->add, 0, (size_t)ncell * 4, stream);
    if (e != hipSuccess) return e;
    size_t tb = s->sort_tmp_bytes;
    e = eslam_radix_sort_pairs_passes(s->keys, s->vals, s->keys_out, s->order, R, s->sort_tmp, &tb, sm_passes(ncell), stream);
    if (e != hipSuccess) return e;
    uint32_t* flag = s->keys;            // the unsorted keys and the record indices are done with
    uint32_t* heads = s->vals;
    hipLaunchKernelGGL(k_sm_flags, dim3(blocks_for(R + 1)), dim3(kBlock), 0, stream, s->keys_out, R, ncell, flag);
    e = eslam_launch_scan_excl(flag, R + 1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sm_heads, dim3(blocks_for(R)), dim3(kBlock), 0, stream, s->keys_out, R, ncell, flag, heads);
    // at most min(R, ncell) segments; the grid is capped and strides over them
    const uint64_t segs = R < ncell ? R : ncell;
    uint64_t ab = (segs + kSmApplyBlock - 1) / kSmApplyBlock;
    ab = ab < 1 ? 1 : (ab > 4096 ? 4096 : ab);
    if (run->gath)
        hipLaunchKernelGGL(k_sm_apply<true>, dim3((uint32_t)ab), dim3(kSmApplyBlock), 0, stream, s0, s1, ctl, *run, *cur,
                           s->keys_out, s->order, heads, flag + R, s->app, s->add, s->segpos, s->touched, s->cnt);
    else
        hipLaunchKernelGGL(k_sm_apply<false>, dim3((uint32_t)ab), dim3(kSmApplyBlock), 0, stream, s0, s1, ctl, *run, *cur,
                           s->keys_out, s->order, heads, flag + R, s->app, s->add, s->segpos, s->touched, s->cnt);
    hipLaunchKernelGGL(k_sm_counts, dim3(blocks_for((uint64_t)ncell + 1)), dim3(kBlock), 0, stream, cur->cell_start, s->add,
                       ncell, next->cell_start);
    e = eslam_launch_scan_excl(next->cell_start, (uint64_t)ncell + 1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sm_rebuild, dim3(blocks_for(ncell)), dim3(kBlock), 0, stream, *cur, *next, s->add, s->segpos, s->app,
                       ncell);
    return hipGetLastError();
}
