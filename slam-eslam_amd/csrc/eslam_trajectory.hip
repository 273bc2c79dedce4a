// eslam_trajectory.hip -- gfx950 kernels of the trajectory log: the particles'
// poses and ancestry per step, kept on the device, and the two queries over them.
//
// The log is a ring of entries, each SoA for up to max_particles particles: x, y, z, yaw, zsigma
// (fp64) and parent (uint32), the slot of the particle's ancestor in the previous held entry:
// 44 bytes per particle per entry, 185 MB per entry at 4M particles.  Beside it one array
// link[max_particles]: link[i] is the slot, in the newest entry, of the ancestor of the current
// particle i (the identity right after a record).  It has two buffers: a composition reads
// link[anc[i]] for arbitrary anc, so it never runs in place.
//
//   k_traj_iota      link[i] = i (enable, clear)
//   k_traj_record    the end of a step: the particles as they stand into an entry, parent[i] =
//                    link[anc[i]] when this update resampled (Ctl::resample, read here), else
//                    link[i]; the other link buffer becomes the identity.  Streaming, four
//                    particles per lane: 16-byte loads and stores
//   k_traj_compose   a resample outside the step: link'[i] = link[anc[i]] over its outputs
//   k_traj_trace     one lane per leaf: from link[index] in the newest entry along parent to the
//                    oldest entry asked for; the nodes land oldest first
//   k_traj_level     the smoothed trajectory's sweep, one level: the ancestors' five columns into
//                    a scratch state (a 4-byte index chase with 8-byte loads), the ancestors' bits
//                    marked in a bitmap (its population count, eslam_kld.hip's, is the level's
//                    distinct ancestors), then a[i] = parent[a[i]] in place for the next level.
//                    Stratified ancestors are non-decreasing and composition keeps that, so the
//                    loads are near-sequential in the common case and a wave's bits share a few
//                    words; nothing here assumes it (multinomial draws come in draw order)
//
// A slot that lies outside its entry (kTrajNone, or anything a sound log never holds) ends the
// walk: it is never used as an index.  The moments of a level are eslam_moments.hip's passes over
// the scratch state.
#include <hip/hip_runtime.h>

#include "eslam_internal.h"
#include "eslam_launch.h"

namespace eslam_dev {

__global__ void __launch_bounds__(kBlock) k_traj_iota(uint32_t* __restrict__ link, uint64_t n)
{
    const uint64_t i0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (i0 + 4 <= n) {
        const uint32_t b = (uint32_t)i0;
        *reinterpret_cast<uint4*>(link + i0) = make_uint4(b, b + 1u, b + 2u, b + 3u);
    } else {
        for (uint64_t i = i0; i < n; ++i) link[i] = (uint32_t)i;
    }
}

// link[a], or kTrajNone for an a outside the link's nlink entries
__device__ __forceinline__ uint32_t traj_link(const uint32_t* __restrict__ link, uint64_t nlink, uint32_t a)
{
    return a < nlink ? link[a] : kTrajNone;
}

__device__ __forceinline__ void traj_copy4(double* __restrict__ dst, const double* __restrict__ src, uint64_t i0)
{
    const double2 lo = *reinterpret_cast<const double2*>(src + i0), hi = *reinterpret_cast<const double2*>(src + i0 + 2);
    *reinterpret_cast<double2*>(dst + i0) = lo;
    *reinterpret_cast<double2*>(dst + i0 + 2) = hi;
}

// Four particles per lane.  Every array starts on a 256-byte boundary (the state's and the log's
// carve-outs, hipMalloc's blocks) and i0 is a multiple of 4, so the 16-byte accesses are aligned.
__global__ void __launch_bounds__(kBlock) k_traj_record(DevState s0, DevState s1, const Ctl* __restrict__ ctl, uint64_t n,
                                                        uint32_t updated, const uint32_t* __restrict__ anc,
                                                        const uint32_t* __restrict__ link, uint64_t nlink,
                                                        uint32_t* __restrict__ link_next, TrajEntry e)
{
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    const bool resampled = updated && ctl->resample != 0;
    const uint64_t i0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (i0 >= n) return;
    if (i0 + 4 <= n) {
        traj_copy4(e.x, st.x, i0);
        traj_copy4(e.y, st.y, i0);
        traj_copy4(e.z, st.z, i0);
        traj_copy4(e.yaw, st.th, i0);
        traj_copy4(e.zs, st.zs, i0);
        const uint32_t b = (uint32_t)i0;
        uint4 a = make_uint4(b, b + 1u, b + 2u, b + 3u);
        if (resampled) a = *reinterpret_cast<const uint4*>(anc + i0);
        uint4 p;
        if (!resampled && i0 + 4 <= nlink) {
            p = *reinterpret_cast<const uint4*>(link + i0);
        } else {
            p.x = traj_link(link, nlink, a.x);
            p.y = traj_link(link, nlink, a.y);
            p.z = traj_link(link, nlink, a.z);
            p.w = traj_link(link, nlink, a.w);
        }
        *reinterpret_cast<uint4*>(e.parent + i0) = p;
        *reinterpret_cast<uint4*>(link_next + i0) = make_uint4(b, b + 1u, b + 2u, b + 3u);
        return;
    }
    for (uint64_t i = i0; i < n; ++i) {
        e.x[i] = st.x[i];
        e.y[i] = st.y[i];
        e.z[i] = st.z[i];
        e.yaw[i] = st.th[i];
        e.zs[i] = st.zs[i];
        e.parent[i] = traj_link(link, nlink, resampled ? anc[i] : (uint32_t)i);
        link_next[i] = (uint32_t)i;
    }
}

__global__ void __launch_bounds__(kBlock) k_traj_compose(const uint32_t* __restrict__ anc, const uint32_t* __restrict__ link,
                                                         uint64_t nlink, uint32_t* __restrict__ link_next, uint64_t n)
{
    const uint64_t i0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (i0 + 4 <= n) {
        const uint4 a = *reinterpret_cast<const uint4*>(anc + i0);
        uint4 p;
        p.x = traj_link(link, nlink, a.x);
        p.y = traj_link(link, nlink, a.y);
        p.z = traj_link(link, nlink, a.z);
        p.w = traj_link(link, nlink, a.w);
        *reinterpret_cast<uint4*>(link_next + i0) = p;
    } else {
        for (uint64_t i = i0; i < n; ++i) link_next[i] = traj_link(link, nlink, anc[i]);
    }
}

// lv[0 .. steps): the entries newest first (uniform over the wave: scalar loads); leaf k's nodes
// at out[k * steps ..], oldest first
__global__ void __launch_bounds__(kBlock) k_traj_trace(const uint32_t* __restrict__ leaf, uint64_t count,
                                                       const uint32_t* __restrict__ link, uint64_t nlink,
                                                       const TrajLevel* __restrict__ lv, uint32_t steps, TrajNode* __restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    const double nan_ = dm_from_bits(0x7ff8000000000000ull);
    uint32_t a = traj_link(link, nlink, leaf[k]);
    for (uint32_t j = 0; j < steps; ++j) {
        const TrajEntry& e = lv[j].e;
        TrajNode o{kTrajNone, 0u, nan_, nan_, nan_, nan_, nan_};
        if (a < lv[j].count) {
            o = TrajNode{a, 0u, e.x[a], e.y[a], e.z[a], e.yaw[a], e.zs[a]};
            a = e.parent[a];
        } else {
            a = kTrajNone;
        }
        out[k * steps + (steps - 1u - j)] = o;
    }
}

// particles [first, n).  Whole waves take every trip: mark_bits_wave's shuffles need all 64 lanes.
__global__ void __launch_bounds__(kBlock) k_traj_level(uint64_t first, uint64_t n, TrajLevel L, uint32_t* __restrict__ a, DevState out,
                                                       uint64_t* __restrict__ bits)
{
    const double nan_ = dm_from_bits(0x7ff8000000000000ull);
    for (uint64_t b = first + (uint64_t)blockIdx.x * kBlock; b < n; b += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = b + threadIdx.x;
        bool need = false;
        uint64_t wi = 0, m = 0;
        if (i < n) {
            const uint32_t ai = a[i];
            if (ai < L.count) {
                out.x[i] = L.e.x[ai];
                out.y[i] = L.e.y[ai];
                out.z[i] = L.e.z[ai];
                out.th[i] = L.e.yaw[ai];
                out.zs[i] = L.e.zs[ai];
                a[i] = L.e.parent[ai];
                need = true;                 // ai < count: its word lies inside the bitmap of count bits
                wi = ai >> 6;
                m = 1ull << (ai & 63u);
            } else {
                // no ancestor in this entry: not a valid particle for the moments (dm_mom_valid)
                out.x[i] = out.y[i] = out.z[i] = out.th[i] = out.zs[i] = nan_;
                a[i] = kTrajNone;
            }
        }
        mark_bits_wave(bits, need, wi, m);
    }
}

static uint32_t traj_blocks4(uint64_t n) { return (uint32_t)((n + 4ull * kBlock - 1) / (4ull * kBlock)); }

}  // namespace eslam_dev

extern "C" hipError_t eslam_launch_traj_iota(uint32_t* link, uint64_t n, hipStream_t stream)
{
    if (n) hipLaunchKernelGGL(k_traj_iota, dim3(traj_blocks4(n)), dim3(kBlock), 0, stream, link, n);
    return hipGetLastError();
}

// the n particles as they stand into entry e; `updated`: the step ran an update, whose resample
// decision the device reads.  link has nlink entries; link_next (another buffer) becomes the identity
extern "C" hipError_t eslam_launch_traj_record(DevState s0, DevState s1, const Ctl* ctl, uint64_t n, int updated, const uint32_t* anc,
                                               const uint32_t* link, uint64_t nlink, uint32_t* link_next, const TrajEntry* e,
                                               hipStream_t stream)
{
    if (n)
        hipLaunchKernelGGL(k_traj_record, dim3(traj_blocks4(n)), dim3(kBlock), 0, stream, s0, s1, ctl, n, updated ? 1u : 0u, anc, link,
                           nlink, link_next, *e);
    return hipGetLastError();
}

// link_next[i] = link[anc[i]] for the n outputs of a resample outside the step
extern "C" hipError_t eslam_launch_traj_compose(const uint32_t* anc, const uint32_t* link, uint64_t nlink, uint32_t* link_next,
                                                uint64_t n, hipStream_t stream)
{
    if (n) hipLaunchKernelGGL(k_traj_compose, dim3(traj_blocks4(n)), dim3(kBlock), 0, stream, anc, link, nlink, link_next, n);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_traj_trace(const uint32_t* leaf, uint64_t count, const uint32_t* link, uint64_t nlink,
                                              const TrajLevel* lv, uint32_t steps, TrajNode* out, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)((count + kBlock - 1) / kBlock);
    if (blocks && steps) hipLaunchKernelGGL(k_traj_trace, dim3(blocks), dim3(kBlock), 0, stream, leaf, count, link, nlink, lv, steps, out);
    return hipGetLastError();
}

// one level of the smoothed sweep over n leaves: the bitmap of (L->count + 63) / 64 words is
// zeroed, the ancestors' columns go to `out` (x, y, th, z, zs; w is the caller's), their bits are
// set and a moves on to the entry before.  As k_kld_mark, a small head launch first: on a
// coalesced lineage the launch over the rest then finds its bits set
extern "C" hipError_t eslam_launch_traj_level(uint64_t n, const TrajLevel* L, uint32_t* a, DevState out, uint64_t* bits,
                                              hipStream_t stream)
{
    const hipError_t e = hipMemsetAsync(bits, 0, (((uint64_t)L->count + 63) / 64) * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    constexpr uint64_t kHead = 16384;
    auto blocks = [](uint64_t items) {
        const uint64_t b = (items + kBlock - 1) / kBlock;
        return (uint32_t)(b > (uint64_t)kKldBlocks ? (uint64_t)kKldBlocks : b);
    };
    const uint64_t head = n < kHead ? n : kHead;
    if (head) hipLaunchKernelGGL(k_traj_level, dim3(blocks(head)), dim3(kBlock), 0, stream, (uint64_t)0, head, *L, a, out, bits);
    if (n > head) hipLaunchKernelGGL(k_traj_level, dim3(blocks(n - head)), dim3(kBlock), 0, stream, head, n, *L, a, out, bits);
    return hipGetLastError();
}
