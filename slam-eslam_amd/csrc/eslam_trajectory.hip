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
// On a sharded filter (eslam_gpu_trajectory_enable_sharded) every slot is global and a rank holds
// its shard of every entry and of link.  The items of an entry are fetched from their owners:
//
//   k_traj_bucket_*  the slots other ranks own, packed by owner in position order: a per-block LDS
//                    histogram from wave ballots, the blocks' exclusive offsets, a stable pack
//   k_traj_serve     the owner writes the items asked for: its own positions in place, the
//                    requests received for the way back; the smoothed sweep's bits are set here
//   k_traj_scatter   the answers to the positions kept
//   k_traj_record_sharded, k_traj_sources, k_traj_trace_take, k_traj_level_take
//                    the record with global parents, and what the queries do with a level's items
//
// A slot that lies outside its entry (kTrajNone, or anything a sound log never holds) ends the
// walk: it is never used as an index.  The moments of a level are eslam_moments.hip's passes over
// the scratch state.
#include <hip/hip_runtime.h>

#include "eslam_internal.h"
#include "eslam_launch.h"

namespace eslam_dev {

__global__ void __launch_bounds__(kBlock) k_traj_iota(uint32_t* __restrict__ link, uint64_t n, uint32_t first)
{
    const uint64_t i0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (i0 + 4 <= n) {
        const uint32_t b = first + (uint32_t)i0;
        *reinterpret_cast<uint4*>(link + i0) = make_uint4(b, b + 1u, b + 2u, b + 3u);
    } else {
        for (uint64_t i = i0; i < n; ++i) link[i] = first + (uint32_t)i;
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

// ---------------------------------------------------------------------------------------
// the log of a sharded filter: slots are global, an entry's items are fetched from their owners
// ---------------------------------------------------------------------------------------
// the rank that owns global slot s under table T, or T.G for a slot outside the entry.  T is a
// kernel argument: its bounds sit in scalar registers and the loop's trip count is uniform
__device__ __forceinline__ uint32_t traj_owner(const TrajTable& T, uint32_t s)
{
    uint32_t o = 0;
    for (uint32_t r = 1; r <= T.G; ++r) o += s >= T.b[r] ? 1u : 0u;
    return o;
}

// the owner a request goes to: another rank's, or T.G for a slot served here (own, or outside the entry)
__device__ __forceinline__ uint32_t traj_dest(const TrajTable& T, uint32_t s)
{
    const uint32_t o = traj_owner(T, s);
    return o == T.me ? T.G : o;
}

__device__ __forceinline__ void traj_put(TrajItem* out, const TrajItem& v)
{
    uint4* o = reinterpret_cast<uint4*>(out);
    const uint4* i = reinterpret_cast<const uint4*>(&v);
    o[0] = i[0];
    o[1] = i[1];
    o[2] = i[2];
}

// Bucketing, pass 1.  Block b takes the requests [b * per, (b + 1) * per) (per: a multiple of
// kBlock, so whole waves take every trip) and counts those of every other owner: a ballot per
// owner, one LDS add per wave and owner.  cnt[b * kMaxRanks + r]: the block's requests to rank r.
__global__ void __launch_bounds__(kBlock) k_traj_bucket_count(const uint32_t* __restrict__ slots, uint64_t count, uint64_t per,
                                                              TrajTable T, uint32_t* __restrict__ cnt)
{
    __shared__ uint32_t hist[kMaxRanks];
    if (threadIdx.x < kMaxRanks) hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < count ? lo + per : count;
    for (uint64_t b = lo; b < hi; b += kBlock) {
        const uint64_t p = b + threadIdx.x;
        const uint32_t o = p < hi ? traj_dest(T, slots[p]) : T.G;
        for (uint32_t r = 0; r < T.G; ++r) {
            const unsigned long long m = __ballot(o == r);
            if (m && (threadIdx.x & 63u) == 0) atomicAdd(&hist[r], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    if (threadIdx.x < kMaxRanks) cnt[(uint64_t)blockIdx.x * kMaxRanks + threadIdx.x] = hist[threadIdx.x];
}

// Pass 2, one wave: lane r turns the blocks' counts for owner r into exclusive offsets in place;
// tot[r] is the owner's total, tot[kMaxRanks + r] the first of its requests in the packed array
__global__ void __launch_bounds__(64) k_traj_bucket_scan(uint32_t* __restrict__ cnt, uint32_t nblocks, uint32_t* __restrict__ tot)
{
    __shared__ uint32_t sum[kMaxRanks];
    const uint32_t r = threadIdx.x;
    if (r < kMaxRanks) {
        uint32_t run = 0;
        for (uint32_t b = 0; b < nblocks; ++b) {
            const uint32_t c = cnt[(uint64_t)b * kMaxRanks + r];
            cnt[(uint64_t)b * kMaxRanks + r] = run;
            run += c;
        }
        sum[r] = run;
        tot[r] = run;
    }
    __syncthreads();
    if (r == 0) {
        uint32_t run = 0;
        for (int q = 0; q < kMaxRanks; ++q) {
            tot[kMaxRanks + q] = run;
            run += sum[q];
        }
        tot[2 * kMaxRanks] = run;
    }
}

// Pass 3, the stable pack: the requests of every owner in the order of their positions.  A
// request's place: its owner's first, the blocks before (cnt), the trips and waves before in this
// block (base, wcnt), the lanes before in this wave (the ballot below the lane).  req: the slots
// asked for, pos: where each answer goes.
__global__ void __launch_bounds__(kBlock) k_traj_bucket_pack(const uint32_t* __restrict__ slots, uint64_t count, uint64_t per, TrajTable T,
                                                             const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ tot,
                                                             uint32_t* __restrict__ req, uint32_t* __restrict__ pos)
{
    __shared__ uint32_t base[kMaxRanks];
    __shared__ uint32_t wcnt[kWaves][kMaxRanks];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < kMaxRanks) base[threadIdx.x] = tot[kMaxRanks + threadIdx.x] + cnt[(uint64_t)blockIdx.x * kMaxRanks + threadIdx.x];
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < count ? lo + per : count;
    for (uint64_t b = lo; b < hi; b += kBlock) {
        const uint64_t p = b + threadIdx.x;
        const uint32_t s = p < hi ? slots[p] : kTrajNone;
        const uint32_t o = p < hi ? traj_dest(T, s) : T.G;
        uint32_t before = 0;
        for (uint32_t r = 0; r < T.G; ++r) {
            const unsigned long long m = __ballot(o == r);
            if (lane == 0) wcnt[wave][r] = (uint32_t)__popcll(m);
            if (o == r) before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        }
        __syncthreads();
        if (o < T.G) {
            uint32_t q = base[o] + before;
            for (uint32_t w = 0; w < wave; ++w) q += wcnt[w][o];
            req[q] = s;
            pos[q] = (uint32_t)p;
        }
        __syncthreads();
        if (threadIdx.x < T.G) {
            uint32_t add = 0;
            for (int w = 0; w < kWaves; ++w) add += wcnt[w][threadIdx.x];
            base[threadIdx.x] += add;
        }
        __syncthreads();
    }
}

// The owner serves.  own_only: the caller's own positions, in place: the slots this rank owns
// and those outside the entry (kTrajNone / NaN items); the others are left to the exchange.
// Otherwise the requests received: every one answered.  NODE: the items are TrajItem, else
// words.  Whole waves take every trip (mark_bits_wave).
template <bool NODE, typename Out>
__global__ void __launch_bounds__(kBlock) k_traj_serve(const uint32_t* __restrict__ slots, uint64_t n, uint32_t own_only, TrajTable T,
                                                       TrajSrc src, Out* __restrict__ out)
{
    const double nan_ = dm_from_bits(0x7ff8000000000000ull);
    for (uint64_t b = (uint64_t)blockIdx.x * kBlock; b < n; b += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = b + threadIdx.x;
        bool need = false;
        uint64_t wi = 0, m = 0;
        if (i < n) {
            const uint32_t s = slots[i], l = s - src.first;
            const bool here = s >= src.first && l < src.count;
            if (here) {
                if constexpr (NODE) {
                    traj_put(out + i, TrajItem{src.e.x[l], src.e.y[l], src.e.z[l], src.e.yaw[l], src.e.zs[l], src.e.parent[l], 0u});
                    need = src.bits != nullptr;          // l < count: its word lies inside the bitmap of count bits
                    wi = l >> 6;
                    m = 1ull << (l & 63u);
                } else {
                    out[i] = src.word[l];
                }
            } else {
                const uint32_t o = own_only ? traj_owner(T, s) : T.G;
                if (o >= T.G || o == T.me) {
                    if constexpr (NODE) traj_put(out + i, TrajItem{nan_, nan_, nan_, nan_, nan_, kTrajNone, 0u});
                    else out[i] = kTrajNone;
                }
            }
        }
        if constexpr (NODE) {
            if (src.bits) mark_bits_wave(src.bits, need, wi, m);
        }
    }
}

// the answers to their positions
template <typename Item>
__global__ void __launch_bounds__(kBlock) k_traj_scatter(const Item* __restrict__ in, const uint32_t* __restrict__ pos, uint64_t n,
                                                         Item* __restrict__ out)
{
    const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    if constexpr (sizeof(Item) == sizeof(TrajItem)) {
        const uint4* i = reinterpret_cast<const uint4*>(in + q);
        uint4* o = reinterpret_cast<uint4*>(out + pos[q]);
        const uint4 v0 = i[0], v1 = i[1], v2 = i[2];
        o[0] = v0;
        o[1] = v1;
        o[2] = v2;
    } else {
        out[pos[q]] = in[q];
    }
}

// the slot of the previous layout each of this rank's n particles descends from: its ancestor
// when this update resampled, else itself (global slots)
__global__ void __launch_bounds__(kBlock) k_traj_sources(const Ctl* __restrict__ ctl, uint32_t updated, const uint32_t* __restrict__ anc,
                                                         uint32_t first, uint64_t n, uint32_t* __restrict__ out)
{
    const bool resampled = updated && ctl->resample != 0;
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = resampled ? anc[i] : first + (uint32_t)i;
}

// k_traj_record on a sharded filter, the same four particles per lane.  parent: `pre` where the
// host fetched link[source] across the ranks; without it the link is the identity and the parent
// is the source itself: the ancestor (an old global index) after a resample, else first + i.
// link_next becomes first + i.
__global__ void __launch_bounds__(kBlock) k_traj_record_sharded(DevState s0, DevState s1, const Ctl* __restrict__ ctl, uint64_t n,
                                                                uint32_t updated, const uint32_t* __restrict__ anc,
                                                                const uint32_t* __restrict__ pre, uint32_t first,
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
        const uint32_t b = first + (uint32_t)i0;
        const uint4 id = make_uint4(b, b + 1u, b + 2u, b + 3u);
        uint4 p = id;
        if (pre) p = *reinterpret_cast<const uint4*>(pre + i0);
        else if (resampled) p = *reinterpret_cast<const uint4*>(anc + i0);
        *reinterpret_cast<uint4*>(e.parent + i0) = p;
        *reinterpret_cast<uint4*>(link_next + i0) = id;
        return;
    }
    for (uint64_t i = i0; i < n; ++i) {
        e.x[i] = st.x[i];
        e.y[i] = st.y[i];
        e.z[i] = st.z[i];
        e.yaw[i] = st.th[i];
        e.zs[i] = st.zs[i];
        e.parent[i] = pre ? pre[i] : resampled ? anc[i] : first + (uint32_t)i;
        link_next[i] = first + (uint32_t)i;
    }
}

// a trace's level: leaf k's item of the entry (fetched by its slot a[k]) into its node, oldest
// first, and a[k] moves on to the parent.  gcount: the entry's global count
__global__ void __launch_bounds__(kBlock) k_traj_trace_take(const TrajItem* __restrict__ items, uint64_t count, uint32_t gcount,
                                                            uint32_t* __restrict__ a, uint32_t steps, uint32_t j,
                                                            TrajNode* __restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    const TrajItem it = items[k];
    const bool in = a[k] < gcount;
    out[k * steps + (steps - 1u - j)] = TrajNode{in ? a[k] : kTrajNone, 0u, it.x, it.y, it.z, it.yaw, it.zs};
    a[k] = in ? it.parent : kTrajNone;
}

// the smoothed sweep's level: particle i's item into the scratch state, a[i] moves on
__global__ void __launch_bounds__(kBlock) k_traj_level_take(const TrajItem* __restrict__ items, uint64_t n, uint32_t* __restrict__ a,
                                                            DevState out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const TrajItem it = items[i];
    out.x[i] = it.x;
    out.y[i] = it.y;
    out.z[i] = it.z;
    out.th[i] = it.yaw;
    out.zs[i] = it.zs;
    a[i] = it.parent;
}

static uint32_t traj_blocks4(uint64_t n) { return (uint32_t)((n + 4ull * kBlock - 1) / (4ull * kBlock)); }
static uint32_t traj_blocks1(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }
static uint32_t traj_blocks_capped(uint64_t n)
{
    const uint64_t b = (n + kBlock - 1) / kBlock;
    return (uint32_t)(b > (uint64_t)kKldBlocks ? (uint64_t)kKldBlocks : b);
}

}  // namespace eslam_dev

// the bucketing's grid for `count` requests: the blocks and the requests of each (a multiple of kBlock)
extern "C" void eslam_traj_bucket_shape(uint64_t count, uint32_t* nblocks, uint64_t* per)
{
    const uint64_t trips = (count + kBlock - 1) / kBlock;
    const uint64_t nb = trips < (uint64_t)kTrajBucketBlocks ? (trips ? trips : 1) : (uint64_t)kTrajBucketBlocks;
    *per = (trips + nb - 1) / nb * kBlock;
    *nblocks = (uint32_t)nb;
}

// the requests among slots[0 .. count) that other ranks own, packed by owner in position order:
// req / pos (room for count each), cnt (nblocks x kMaxRanks), tot (kTrajTotWords)
extern "C" hipError_t eslam_launch_traj_bucket(const uint32_t* slots, uint64_t count, const TrajTable* T, uint32_t* cnt, uint32_t* tot,
                                               uint32_t* req, uint32_t* pos, hipStream_t stream)
{
    uint32_t nb;
    uint64_t per;
    eslam_traj_bucket_shape(count, &nb, &per);
    hipLaunchKernelGGL(k_traj_bucket_count, dim3(nb), dim3(kBlock), 0, stream, slots, count, per, *T, cnt);
    hipLaunchKernelGGL(k_traj_bucket_scan, dim3(1), dim3(64), 0, stream, cnt, nb, tot);
    hipLaunchKernelGGL(k_traj_bucket_pack, dim3(nb), dim3(kBlock), 0, stream, slots, count, per, *T, cnt, tot, req, pos);
    return hipGetLastError();
}

// node: out is TrajItem[n], else uint32_t[n].  A bitmap in src->bits gains the served slots' bits
extern "C" hipError_t eslam_launch_traj_serve(int node, const uint32_t* slots, uint64_t n, int own_only, const TrajTable* T,
                                              const TrajSrc* src, void* out, hipStream_t stream)
{
    if (!n) return hipSuccess;
    const dim3 grid(traj_blocks_capped(n));
    if (node)
        hipLaunchKernelGGL((k_traj_serve<true, TrajItem>), grid, dim3(kBlock), 0, stream, slots, n, own_only ? 1u : 0u, *T, *src,
                           static_cast<TrajItem*>(out));
    else
        hipLaunchKernelGGL((k_traj_serve<false, uint32_t>), grid, dim3(kBlock), 0, stream, slots, n, own_only ? 1u : 0u, *T, *src,
                           static_cast<uint32_t*>(out));
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_traj_scatter(int node, const void* in, const uint32_t* pos, uint64_t n, void* out, hipStream_t stream)
{
    if (!n) return hipSuccess;
    if (node)
        hipLaunchKernelGGL(k_traj_scatter<TrajItem>, dim3(traj_blocks1(n)), dim3(kBlock), 0, stream, static_cast<const TrajItem*>(in), pos,
                           n, static_cast<TrajItem*>(out));
    else
        hipLaunchKernelGGL(k_traj_scatter<uint32_t>, dim3(traj_blocks1(n)), dim3(kBlock), 0, stream, static_cast<const uint32_t*>(in), pos,
                           n, static_cast<uint32_t*>(out));
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_traj_sources(const Ctl* ctl, int updated, const uint32_t* anc, uint32_t first, uint64_t n,
                                                uint32_t* out, hipStream_t stream)
{
    if (n) hipLaunchKernelGGL(k_traj_sources, dim3(traj_blocks1(n)), dim3(kBlock), 0, stream, ctl, updated ? 1u : 0u, anc, first, n, out);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_traj_record_sharded(DevState s0, DevState s1, const Ctl* ctl, uint64_t n, int updated,
                                                       const uint32_t* anc, const uint32_t* pre, uint32_t first, uint32_t* link_next,
                                                       const TrajEntry* e, hipStream_t stream)
{
    if (n)
        hipLaunchKernelGGL(k_traj_record_sharded, dim3(traj_blocks4(n)), dim3(kBlock), 0, stream, s0, s1, ctl, n, updated ? 1u : 0u, anc,
                           pre, first, link_next, *e);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_traj_trace_take(const TrajItem* items, uint64_t count, uint32_t gcount, uint32_t* a, uint32_t steps,
                                                   uint32_t j, TrajNode* out, hipStream_t stream)
{
    if (count) hipLaunchKernelGGL(k_traj_trace_take, dim3(traj_blocks1(count)), dim3(kBlock), 0, stream, items, count, gcount, a, steps, j, out);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_traj_level_take(const TrajItem* items, uint64_t n, uint32_t* a, DevState out, hipStream_t stream)
{
    if (n) hipLaunchKernelGGL(k_traj_level_take, dim3(traj_blocks1(n)), dim3(kBlock), 0, stream, items, n, a, out);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_traj_iota(uint32_t* link, uint64_t n, hipStream_t stream)
{
    if (n) hipLaunchKernelGGL(k_traj_iota, dim3(traj_blocks4(n)), dim3(kBlock), 0, stream, link, n, 0u);
    return hipGetLastError();
}

// a sharded filter's identity: link[i] = first + i, the global slot of this rank's particle i
extern "C" hipError_t eslam_launch_traj_iota_from(uint32_t* link, uint64_t n, uint32_t first, hipStream_t stream)
{
    if (n) hipLaunchKernelGGL(k_traj_iota, dim3(traj_blocks4(n)), dim3(kBlock), 0, stream, link, n, first);
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
