// eslam_snapshot.hip -- the device side of eslam_gpu_save / eslam_gpu_load.
//
// A snapshot names tables and pages by compact ids in a canonical order, so its bytes depend
// on the filter's logical state only and not on the pool entries history happened to use:
//   tables  in the order of the lowest particle index that names them,
//   pages   in the order of their first reference, walking the tables in that order: the
//           window's slots ascending, then the trail's used entries ascending.
// The census (two compactions with the map update's tile size and exclusive scan) finds the
// ranks; the pack kernels write contiguous ranges of ranks into a staging buffer, the unpack
// kernels read them back into pool entries [k0, k1).  A save reads the pool and the particles
// and writes only its own scratch.
// A sharded filter's ranks write one blob between them: the packs add the ids of the ranks
// below (tbase, pbase).  A sharded load takes the subset its particles name: two bitmaps over
// the snapshot's ids, ranked by popcount (k_snap_mark_*, k_snap_popc, k_snap_rank_sid,
// k_snap_renumber_tables, k_snap_unpack_owner_subset).
#include <hip/hip_runtime.h>
#include <string.h>
#include "eslam_internal.h"
#include "eslam_launch.h"

using namespace eslam_dev;

namespace {

__device__ __forceinline__ uint32_t hw_of(uint32_t w) { return w == DM_LM_NONE ? 0u : w; }

struct SnapArgs {
    LocalMaps lm;
    SnapCensus c;
    const uint32_t* sid;                 // the current state buffer's table names
    uint64_t n;                          // particles
    uint64_t T;                          // live tables (the page census and the packs)
    uint32_t W, K, toff;                 // window slots; keys per table (W + V); trail offset
    uint32_t tbase, pbase;               // a sharded save: the compact ids of this rank's first table and page
};

// the page of key s of a table row (DM_LM_NONE: none, or an entry past the high-water mark)
__device__ __forceinline__ uint32_t row_page(const SnapArgs& a, const uint32_t* row, uint32_t s)
{
    if (s < a.W) return row[s];
    const uint32_t e = s - a.W;
    if (e >= hw_of(row[a.toff - 1u])) return DM_LM_NONE;
    return row[a.toff + 4u * e + 2u];
}

// first[t] = the lowest particle index naming table t
__global__ void __launch_bounds__(kBlock) k_snap_first(SnapArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t t = a.sid[i];
    if (t < a.lm.ntables) atomicMin(&a.c.first[t], (uint32_t)i);
}

// firstref[p] = the lowest key r * K + s that references page p: one wave per ranked table
// walks its window slots and its used trail entries only (not the row's padding words).
// The key is 64 bits (16M tables x 148 words pass 2^32) and goes through the 64-bit atomic
// minimum; r < 2^32 and K < 2^14, so it stays below 2^46.
__global__ void __launch_bounds__(kBlock) k_snap_pgfirst(SnapArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    for (uint64_t r = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < a.T; r += nw) {
        const uint32_t* row = a.lm.slot + (uint64_t)a.c.tlist[r] * a.lm.S;
        const uint32_t cnt = a.W + hw_of(row[a.toff - 1u]);
        for (uint32_t s = lane; s < cnt && s < a.K; s += 64u) {
            const uint32_t p = row_page(a, row, s);
            if (p == DM_LM_NONE || p >= a.lm.npages) continue;
            // copies of a table share its pages, and the ranks run roughly in order: most keys
            // find a lower one already there, so look before the atomic (the word only falls; a
            // stale read costs one atomic that changes nothing)
            const unsigned long long key = (unsigned long long)(r * a.K + s);
            unsigned long long* w = (unsigned long long*)&a.c.firstref[p];
            if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(w, key);
        }
    }
}

// the census' two compactions.  MODE 0, over the particles: particle i is the first to name
// its table (id: the table).  MODE 1, over the keys of the ranked tables: key k is the first
// reference of its page (id: the page).
template <int MODE>
__device__ __forceinline__ bool snap_sel(const SnapArgs& a, uint64_t i, uint32_t& id)
{
    if (MODE == 0) {
        if (i >= a.n) return false;
        id = a.sid[i];
        return id < a.lm.ntables && a.c.first[id] == (uint32_t)i;
    }
    if (i >= a.T * a.K) return false;
    const uint64_t r = i / a.K;
    const uint32_t s = (uint32_t)(i - r * a.K);
    const uint32_t* row = a.lm.slot + (uint64_t)a.c.tlist[r] * a.lm.S;
    id = row_page(a, row, s);
    return id != DM_LM_NONE && id < a.lm.npages && a.c.firstref[id] == i;
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) k_snap_count(SnapArgs a)
{
    __shared__ uint32_t s_w[kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kCompactTileItems;
    uint32_t c = 0, id;
    for (int r = 0; r < kCompactItems; ++r) {
        const uint64_t i = base + (uint64_t)r * kBlock + threadIdx.x;
        c += (uint32_t)__popcll(__ballot(snap_sel<MODE>(a, i, id)));
    }
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = c;       // every lane holds its wave's count
    __syncthreads();
    if (threadIdx.x == 0) a.c.counts[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// counts: the exclusive prefix of the tile counts; the selected item of rank q gives
// list[q] = id and rank[id] = q
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_snap_write(SnapArgs a)
{
    __shared__ uint32_t s_w[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kCompactTileItems;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t* list = MODE == 0 ? a.c.tlist : a.c.plist;
    uint32_t* rank = MODE == 0 ? a.c.trank : a.c.prank;
    uint32_t run = a.c.counts[blockIdx.x];
    for (int r = 0; r < kCompactItems; ++r) {
        const uint64_t i = base + (uint64_t)r * kBlock + threadIdx.x;
        uint32_t id = 0;
        const bool sel = snap_sel<MODE>(a, i, id);
        const uint64_t b = __ballot(sel);
        if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pos = run + (uint32_t)__popcll(b & below);
        for (uint32_t w = 0; w < wave; ++w) pos += s_w[w];
        if (sel) {
            list[pos] = id;
            rank[id] = pos;
        }
        run += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

// ---- pack: ranks [k0, k0 + cnt) into the staging buffer ------------------------------------
__global__ void __launch_bounds__(kBlock) k_snap_pack_sid(SnapArgs a, uint64_t i0, uint64_t cnt, uint32_t* __restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    const uint32_t t = a.sid[i0 + j];
    out[j] = t < a.lm.ntables ? a.c.trank[t] + a.tbase : DM_LM_NONE;
}

// a wave per table: the row {centre x, y, shadow, hw, W slots, V x {a, b, page}} padded to
// rw words, page ids renumbered; trail entries that hold no page read {0, 0, none}
__global__ void __launch_bounds__(kBlock) k_snap_pack_tables(SnapArgs a, uint64_t k0, uint64_t cnt, uint32_t rw,
                                                            uint32_t* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t j = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (j >= cnt) return;
    const uint32_t t = a.c.tlist[k0 + j];
    const uint32_t* row = a.lm.slot + (uint64_t)t * a.lm.S;
    const uint32_t hw = hw_of(row[a.toff - 1u]);
    const int2 ctr = a.lm.ctr[t];
    uint32_t* o = out + j * rw;
    for (uint32_t q = lane; q < rw; q += 64u) {
        uint32_t v = 0u;
        if (q == 0u) v = (uint32_t)ctr.x;
        else if (q == 1u) v = (uint32_t)ctr.y;
        else if (q == 2u) v = row[a.toff - 2u] == kLmShadow ? 1u : 0u;
        else if (q == 3u) v = hw;
        else if (q < 4u + a.W) {
            const uint32_t p = row[q - 4u];
            v = (p != DM_LM_NONE && p < a.lm.npages) ? a.c.prank[p] + a.pbase : DM_LM_NONE;
        } else if (q < 4u + a.W + 3u * a.lm.V) {
            const uint32_t e = (q - 4u - a.W) / 3u, f = (q - 4u - a.W) - 3u * e;
            const uint32_t p = e < hw ? row[a.toff + 4u * e + 2u] : DM_LM_NONE;
            const bool live = p != DM_LM_NONE && p < a.lm.npages;
            if (f == 2u) v = live ? a.c.prank[p] + a.pbase : DM_LM_NONE;
            else v = live ? row[a.toff + 4u * e + f] : 0u;
        }
        o[q] = v;
    }
}

// the compact id of the table that may still write page k in place (a live table t with
// owner == tgen[t] << 32 | t), else none
__global__ void __launch_bounds__(kBlock) k_snap_pack_owner(SnapArgs a, uint64_t k0, uint64_t cnt, uint32_t* __restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    const uint64_t o = a.lm.owner[a.c.plist[k0 + j]];
    const uint32_t t = (uint32_t)o;
    uint32_t v = DM_LM_NONE;
    if (t < a.lm.ntables && a.c.first[t] != 0xffffffffu && (uint32_t)(o >> 32) == a.lm.tgen[t]) v = a.c.trank[t] + a.tbase;
    out[j] = v;
}

// 32 lanes x 16 bytes move one 512-byte page: two pages per wave instruction, coalesced on
// both sides
__global__ void __launch_bounds__(kBlock) k_snap_pack_pages(SnapArgs a, uint64_t k0, uint64_t cnt, uint4* __restrict__ out)
{
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t j = g >> 5;
    if (j >= cnt) return;
    const uint4* src = reinterpret_cast<const uint4*>(a.lm.page + (uint64_t)a.c.plist[k0 + j] * DM_LM_PAGE_CELLS);
    out[g] = src[g & 31u];
}

// ---- unpack: the staging buffer into pool entries [k0, k0 + cnt) (the host has checked
// every id of the chunk) ---------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_snap_unpack_tables(SnapArgs a, uint64_t k0, uint64_t cnt, uint32_t rw,
                                                              const uint32_t* __restrict__ in)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t j = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (j >= cnt) return;
    const uint64_t t = k0 + j;
    const uint32_t* r = in + j * rw;
    const uint32_t hw = r[3];
    uint32_t* row = a.lm.slot + t * a.lm.S;
    if (lane == 0) a.lm.ctr[t] = make_int2((int32_t)r[0], (int32_t)r[1]);
    for (uint32_t q = lane; q < a.lm.S; q += 64u) {
        uint32_t v = DM_LM_NONE;
        if (q < a.W) v = r[4u + q];
        else if (q < a.toff) {
            if (q == a.toff - 1u) v = hw ? hw : DM_LM_NONE;
            else if (q == a.toff - 2u) v = r[2] ? kLmShadow : DM_LM_NONE;
        } else {
            const uint32_t e = (q - a.toff) >> 2, f = (q - a.toff) & 3u;
            if (e < hw && f < 3u) v = r[4u + a.W + 3u * e + f];
        }
        row[q] = v;
    }
}

__global__ void __launch_bounds__(kBlock) k_snap_unpack_owner(SnapArgs a, uint64_t k0, uint64_t cnt, const uint32_t* __restrict__ in)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    const uint32_t t = in[j];
    a.lm.owner[k0 + j] = t == DM_LM_NONE ? ~0ull : (uint64_t)t;      // generation 0
}

// after the last chunk, over the whole pool: tables and pages past the loaded ones empty and
// unowned, every generation 0, no marks, the free list = the remaining pages in page order
__global__ void __launch_bounds__(kBlock) k_snap_finish(LocalMaps lm, uint64_t T, uint64_t P, uint64_t items)
{
    const uint64_t slots = lm.ntables * lm.S;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < items; i += (uint64_t)gridDim.x * kBlock) {
        if (i < slots && i >= T * lm.S) lm.slot[i] = DM_LM_NONE;
        if (i < lm.ntables) {
            lm.tgen[i] = 0u;
            if (i >= T) lm.ctr[i] = make_int2(DM_LM_UNSET, DM_LM_UNSET);
        }
        if (i < lm.npages) {
            lm.mark[i] = 0u;
            if (i >= P) lm.owner[i] = ~0ull;
            if (i < lm.npages - P) lm.frees[i] = (uint32_t)(P + i);
        }
    }
}

// ---- a sharded load's subset ("Sharded filters"): bitmaps over the snapshot's
// compact ids, ranked by popcount ------------------------------------------------------------
// Copies of one table (or tables sharing a page) hammer one word: look before the atomic, as
// k_snap_pgfirst does (the word only gains bits; a stale read costs one atomic that changes nothing).
__device__ __forceinline__ void mark_bit(uint32_t* bits, uint32_t id)
{
    uint32_t* w = bits + (id >> 5);
    const uint32_t m = 1u << (id & 31u);
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m)) atomicOr(w, m);
}

__device__ __forceinline__ bool bit_set(const uint32_t* bits, uint32_t id) { return (bits[id >> 5] >> (id & 31u)) & 1u; }

__device__ __forceinline__ uint32_t bit_rank(const uint32_t* bits, const uint32_t* pre, uint32_t id)
{
    return pre[id >> 5] + (uint32_t)__popc(bits[id >> 5] & ((1u << (id & 31u)) - 1u));
}

// one lane per id (a particle's table): bit id of the bitmap of `limit` bits
__global__ void __launch_bounds__(kBlock) k_snap_mark_bits(const uint32_t* __restrict__ ids, uint64_t n, uint32_t* bits, uint64_t limit)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = ids[i];
    if (t < limit) mark_bit(bits, t);
}

// a wave per pool table [0, T): the pages of its window slots and its used trail entries
__global__ void __launch_bounds__(kBlock) k_snap_mark_rows(SnapArgs a, uint32_t* bits, uint64_t limit)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    for (uint64_t r = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < a.T; r += nw) {
        const uint32_t* row = a.lm.slot + r * a.lm.S;
        const uint32_t cnt = a.W + hw_of(row[a.toff - 1u]);
        for (uint32_t s = lane; s < cnt && s < a.K; s += 64u) {
            const uint32_t p = row_page(a, row, s);
            if (p != DM_LM_NONE && p < limit) mark_bit(bits, p);
        }
    }
}

// pre[w] = popc(bits[w]), pre[words] = 0: the exclusive scan then leaves the total there
__global__ void __launch_bounds__(kBlock) k_snap_popc(const uint32_t* __restrict__ bits, uint64_t words, uint32_t* __restrict__ pre)
{
    const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (w > words) return;
    pre[w] = w < words ? (uint32_t)__popc(bits[w]) : 0u;
}

__global__ void __launch_bounds__(kBlock) k_snap_rank_sid(uint32_t* sid, uint64_t n, SnapSubset s)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = sid[i];
    if (t < s.tables) sid[i] = bit_rank(s.tbits, s.tpre, t);
}

// a wave per pool table [0, T): the snapshot's page ids of its row become this rank's
__global__ void __launch_bounds__(kBlock) k_snap_renumber_tables(SnapArgs a, SnapSubset s)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    for (uint64_t r = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < a.T; r += nw) {
        uint32_t* row = a.lm.slot + r * a.lm.S;
        const uint32_t hw = hw_of(row[a.toff - 1u]);
        for (uint32_t q = lane; q < a.lm.S; q += 64u) {
            const bool slot = q < a.W;
            const bool trail = q >= a.toff && ((q - a.toff) & 3u) == 2u && ((q - a.toff) >> 2) < hw;
            if (!slot && !trail) continue;
            const uint32_t p = row[q];
            if (p != DM_LM_NONE && p < s.pages) row[q] = bit_rank(s.pbits, s.ppre, p);
        }
    }
}

// owner words of pages [k0, k0 + cnt) of this rank: a table this rank holds by its local id,
// any other table as none (nobody here writes the page in place)
__global__ void __launch_bounds__(kBlock) k_snap_unpack_owner_subset(SnapArgs a, uint64_t k0, uint64_t cnt, SnapSubset s,
                                                                    const uint32_t* __restrict__ in)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    const uint32_t t = in[j];
    uint64_t v = ~0ull;
    if (t != DM_LM_NONE && t < s.tables && bit_set(s.tbits, t)) v = (uint64_t)bit_rank(s.tbits, s.tpre, t);   // generation 0
    a.lm.owner[k0 + j] = v;
}

SnapArgs snap_args(const LocalMaps* lm, const SnapCensus* c, const uint32_t* sid, uint64_t n, uint64_t T)
{
    SnapArgs a;
    memset(&a, 0, sizeof(a));
    a.lm = *lm;
    if (c) a.c = *c;
    a.sid = sid;
    a.n = n;
    a.T = T;
    a.W = lm->wx * lm->wy;
    a.K = a.W + lm->V;
    a.toff = lm->S - 4u * lm->V;
    return a;
}

template <int MODE>
hipError_t snap_compact(const SnapArgs& a, uint64_t items, hipStream_t stream)
{
    const uint32_t tiles = (uint32_t)((items + kCompactTileItems - 1) / kCompactTileItems);
    hipError_t e = hipMemsetAsync(a.c.counts + tiles, 0, 4, stream);
    if (e != hipSuccess) return e;
    if (tiles) hipLaunchKernelGGL(k_snap_count<MODE>, dim3(tiles), dim3(kBlock), 0, stream, a);
    e = eslam_launch_scan_excl(a.c.counts, (uint64_t)tiles + 1, stream);
    if (e != hipSuccess) return e;
    if (tiles) hipLaunchKernelGGL(k_snap_write<MODE>, dim3(tiles), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

inline dim3 blocks_for(uint64_t threads) { return dim3((uint32_t)((threads + kBlock - 1) / kBlock)); }

}  // namespace

// the table census: c->tlist / c->trank, the count in c->counts[snap_tiles(n)]
extern "C" hipError_t eslam_launch_snap_census_tables(const LocalMaps* lm, const SnapCensus* c, const uint32_t* sid, uint64_t n,
                                                      hipStream_t stream)
{
    const SnapArgs a = snap_args(lm, c, sid, n, 0);
    hipError_t e = hipMemsetAsync(c->first, 0xff, lm->ntables * 4, stream);
    if (e != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(k_snap_first, blocks_for(n), dim3(kBlock), 0, stream, a);
    return snap_compact<0>(a, n, stream);
}

// the page census of the T ranked tables: c->plist / c->prank, the count in
// c->counts[snap_tiles(T * (W + V))]
extern "C" hipError_t eslam_launch_snap_census_pages(const LocalMaps* lm, const SnapCensus* c, uint64_t T, hipStream_t stream)
{
    const SnapArgs a = snap_args(lm, c, nullptr, 0, T);
    hipError_t e = hipMemsetAsync(c->firstref, 0xff, lm->npages * 8, stream);
    if (e != hipSuccess) return e;
    const uint64_t gm = (T + kWaves - 1) / kWaves;
    if (T) hipLaunchKernelGGL(k_snap_pgfirst, dim3((uint32_t)(gm < 65536 ? gm : 65536)), dim3(kBlock), 0, stream, a);
    return snap_compact<1>(a, T * a.K, stream);
}

// what: 0 the particles' compact table ids, 1 table rows (rw words each), 2 owner words, 3 pages
// tbase, pbase: added to every table and page id written (a sharded save: the ids of the ranks below; else 0)
extern "C" hipError_t eslam_launch_snap_pack(int what, const LocalMaps* lm, const SnapCensus* c, const uint32_t* sid, uint64_t T,
                                             uint32_t tbase, uint32_t pbase, uint64_t k0, uint64_t cnt, uint32_t rw, void* out,
                                             hipStream_t stream)
{
    if (!cnt) return hipSuccess;
    SnapArgs a = snap_args(lm, c, sid, 0, T);
    a.tbase = tbase;
    a.pbase = pbase;
    if (what == 0) hipLaunchKernelGGL(k_snap_pack_sid, blocks_for(cnt), dim3(kBlock), 0, stream, a, k0, cnt, (uint32_t*)out);
    else if (what == 1) hipLaunchKernelGGL(k_snap_pack_tables, blocks_for(cnt * 64), dim3(kBlock), 0, stream, a, k0, cnt, rw, (uint32_t*)out);
    else if (what == 2) hipLaunchKernelGGL(k_snap_pack_owner, blocks_for(cnt), dim3(kBlock), 0, stream, a, k0, cnt, (uint32_t*)out);
    else hipLaunchKernelGGL(k_snap_pack_pages, blocks_for(cnt * 32), dim3(kBlock), 0, stream, a, k0, cnt, (uint4*)out);
    return hipGetLastError();
}

// what: 1 table rows, 2 owner words (the particles' ids and the pages are plain copies)
extern "C" hipError_t eslam_launch_snap_unpack(int what, const LocalMaps* lm, uint64_t k0, uint64_t cnt, uint32_t rw, const void* in,
                                               hipStream_t stream)
{
    if (!cnt) return hipSuccess;
    const SnapArgs a = snap_args(lm, nullptr, nullptr, 0, 0);
    if (what == 1) hipLaunchKernelGGL(k_snap_unpack_tables, blocks_for(cnt * 64), dim3(kBlock), 0, stream, a, k0, cnt, rw, (const uint32_t*)in);
    else hipLaunchKernelGGL(k_snap_unpack_owner, blocks_for(cnt), dim3(kBlock), 0, stream, a, k0, cnt, (const uint32_t*)in);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_snap_finish(const LocalMaps* lm, uint64_t T, uint64_t P, hipStream_t stream)
{
    uint64_t items = lm->ntables * lm->S;
    if (lm->npages > items) items = lm->npages;
    const uint64_t want = (items + kBlock - 1) / kBlock;
    if (items) hipLaunchKernelGGL(k_snap_finish, dim3((uint32_t)(want < 65536 ? want : 65536)), dim3(kBlock), 0, stream, *lm, T, P, items);
    return hipGetLastError();
}

// ---- a sharded load's subset ------------------------------------------------------------------
namespace {
inline dim3 waves_for(uint64_t rows)
{
    const uint64_t gm = (rows + kWaves - 1) / kWaves;
    return dim3((uint32_t)(gm < 65536 ? gm : 65536));
}
}  // namespace

// bit ids[i] of `bits` (bits bits, cleared by the caller), i < n
extern "C" hipError_t eslam_launch_snap_mark_ids(const uint32_t* ids, uint64_t n, uint32_t* bits, uint64_t limit, hipStream_t stream)
{
    if (n) hipLaunchKernelGGL(k_snap_mark_bits, blocks_for(n), dim3(kBlock), 0, stream, ids, n, bits, limit);
    return hipGetLastError();
}

// the bits of the pages that pool tables [0, T) name (rows as unpacked: the snapshot's page ids)
extern "C" hipError_t eslam_launch_snap_mark_rows(const LocalMaps* lm, uint64_t T, uint32_t* bits, uint64_t limit, hipStream_t stream)
{
    const SnapArgs a = snap_args(lm, nullptr, nullptr, 0, T);
    if (T) hipLaunchKernelGGL(k_snap_mark_rows, waves_for(T), dim3(kBlock), 0, stream, a, bits, limit);
    return hipGetLastError();
}

// pre[0 .. words]: the exclusive prefix of the words' popcounts, pre[words] the number of set bits
extern "C" hipError_t eslam_launch_snap_rank_bits(const uint32_t* bits, uint64_t words, uint32_t* pre, hipStream_t stream)
{
    hipLaunchKernelGGL(k_snap_popc, blocks_for(words + 1), dim3(kBlock), 0, stream, bits, words, pre);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : eslam_launch_scan_excl(pre, words + 1, stream);
}

extern "C" hipError_t eslam_launch_snap_rank_sid(uint32_t* sid, uint64_t n, const SnapSubset* s, hipStream_t stream)
{
    if (n) hipLaunchKernelGGL(k_snap_rank_sid, blocks_for(n), dim3(kBlock), 0, stream, sid, n, *s);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_snap_renumber_tables(const LocalMaps* lm, uint64_t T, const SnapSubset* s, hipStream_t stream)
{
    const SnapArgs a = snap_args(lm, nullptr, nullptr, 0, T);
    if (T) hipLaunchKernelGGL(k_snap_renumber_tables, waves_for(T), dim3(kBlock), 0, stream, a, *s);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_snap_unpack_owner_subset(const LocalMaps* lm, uint64_t k0, uint64_t cnt, const SnapSubset* s,
                                                            const void* in, hipStream_t stream)
{
    if (!cnt) return hipSuccess;
    const SnapArgs a = snap_args(lm, nullptr, nullptr, 0, 0);
    hipLaunchKernelGGL(k_snap_unpack_owner_subset, blocks_for(cnt), dim3(kBlock), 0, stream, a, k0, cnt, *s, (const uint32_t*)in);
    return hipGetLastError();
}
