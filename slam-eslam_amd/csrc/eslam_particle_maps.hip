// eslam_particle_maps.hip -- per-particle local maps (useSharedMap = false; SURVEY.md 8f row 3;
// DESIGN.md 5c): processMap's merge of a scan into every particle's map
// (src/EmbodiedSlamFilter.cpp:179-232) and cloneMaps' independent copies
// (src/PoseEstimator.cpp:31-47) as copy on write of tables and pages (eslam_internal.h
// LocalMaps): the stores' reference counts and compaction, the page budget and collection, the
// plan, the merge, the scan match, and, for sharded filters, the maps that travel with
// migrating particles (k_pay_*, k_recv_*).
#include <hip/hip_runtime.h>
#include <type_traits>
#include <string.h>

#include "eslam_internal.h"
#include "eslam_launch.h"
#include "eslam_wave.h"
#include "eslam_stamps.h"

namespace eslam_dev {

#ifdef ESLAM_STAMPS
ESLAM_STAMP_ARRAY(g_stamps_mg);              // the map merge (its first group)
#endif

// fresh maps: particle i names table i (sid: both state buffers' names, 2 x n), every table
// empty, every page free and unowned
__global__ void __launch_bounds__(kBlock) k_store_init(uint32_t* __restrict__ sid, LocalMaps lm, uint64_t n, uint64_t pool,
                                                      uint64_t items)
{
    const uint64_t slots = pool * lm.S;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < items; i += (uint64_t)gridDim.x * kBlock) {
        if (i < slots) lm.slot[i] = DM_LM_NONE;
        if (i < pool) {
            lm.ctr[i] = make_int2(DM_LM_UNSET, DM_LM_UNSET);
            lm.tgen[i] = 0u;
            if (i < n) {                     // both state buffers' names (n = cap here)
                sid[i] = (uint32_t)i;
                sid[n + i] = (uint32_t)i;
            }
        }
        if (i < lm.npages) {
            lm.frees[i] = (uint32_t)i;
            lm.owner[i] = ~0ull;
        }
    }
}

__device__ __forceinline__ uint32_t* cur_sid(const SidRef& r) { return (r.ctl->base ^ r.ctl->flip) ? r.s1 : r.s0; }

// ref[s]: 0, 1 or >= 2 particles name table s (received particles name none yet; the map merge
// only asks "free", "own" or "shared").  A resample hands the copies of a particle out as
// consecutive outputs, so equal names come in runs: the first lane of a run within the wave
// raises ref to 2 with a plain store when the run is longer than one (no atomic: as sharing
// grows, long runs span many waves and one hot atomic per wave serialised at 0.6 ms per 8M),
// and adds 1 atomically otherwise.  Any interleaving ends at the right class.  A table found
// shared moves to its next generation: its pages are frozen (the copies will name them too).
__global__ void __launch_bounds__(kBlock) k_store_ref(SidRef sr, uint64_t n, uint32_t* __restrict__ ref, GatherView gv,
                                                     uint32_t fuse, uint32_t* __restrict__ tgen)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t s;
    if (fuse && sr.ctl->gather) {
        // a pending resample gather that the map merge runs (MergeParams::fuse): output i will
        // name its ancestor's table (the marks expanded as in K1, state[base] read)
        const uint64_t row0 = i & ~(uint64_t)(kRow - 1);          // a row past n has no row_first entry
        const uint32_t carry = row0 < n ? gv.row_first[row0 / kRow] + 1u : 0u;
        uint32_t mk = i < n ? gv.marks[i] : 0u;
        mk = wave_incl_max_u32(mk);
        const uint32_t src = (mk > carry ? mk : carry) - 1u;
        const uint32_t* sin = sr.ctl->base ? sr.s1 : sr.s0;
        s = i < n ? sin[src] : 0xffffffffu;
    } else {
        const uint32_t* sid = cur_sid(sr);
        s = i < n ? sid[i] : 0xffffffffu;
    }
    const uint32_t prev = (uint32_t)__shfl_up((int)s, 1, 64);
    const bool head = lane == 0 || prev != s;
    const uint64_t heads = __ballot(head);
    const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
    const uint32_t len = above ? (uint32_t)__builtin_ctzll(above) + 1u : 64u - lane;
    if (head && !(s & kSidRecord)) {                               // 0xffffffff has the record bit
        if (len >= 2u) {
            if (ref[s] < 2u) ref[s] = 2u;
            tgen[s] += 1u;                   // racing bumps of one table only move it further
        } else if (atomicAdd(&ref[s], 1u) >= 1u) {
            tgen[s] += 1u;
        }
    }
}

// compaction, mode 0: the free tables (ref 0) in table order, over the pool; mode 1: the
// particles received from another rank (sid = kSidRecord | record), in particle order;
// mode 2: the free pages (mark 0) in page order.  gate (device word, may be null): when 0
// the launch does nothing (the collection runs only when a map update needs it)
__device__ __forceinline__ bool compact_pred(int mode, uint64_t i, const uint32_t* ref, const uint32_t* sid)
{
    if (mode == 2) return reinterpret_cast<const uint8_t*>(ref)[i] == 0u;
    return mode == 0 ? ref[i] == 0u : (sid[i] & kSidRecord) != 0u;
}

constexpr int kCompactTile = kCompactTileItems;

__global__ void __launch_bounds__(kBlock) k_compact_count(int mode, uint64_t n, const uint32_t* __restrict__ ref,
                                                          SidRef sr, uint32_t* __restrict__ counts,
                                                          const uint32_t* __restrict__ gate)
{
    if (gate && !*gate) return;
    const uint32_t* sid = mode == 1 ? cur_sid(sr) : nullptr;
    __shared__ uint32_t s_w[kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kCompactTile;
    uint32_t c = 0;
    for (int r = 0; r < kCompactItems; ++r) {
        const uint64_t i = base + (uint64_t)r * kBlock + threadIdx.x;
        if (i < n && compact_pred(mode, i, ref, sid)) ++c;
    }
    c = wave_sum_u32(c);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// offs: exclusive prefix of counts; each selected i goes to out[offs[b] + its rank in the tile]
__global__ void __launch_bounds__(kBlock) k_compact_write(int mode, uint64_t n, const uint32_t* __restrict__ ref,
                                                          SidRef sr, const uint32_t* __restrict__ offs,
                                                          uint32_t* __restrict__ out, const uint32_t* __restrict__ gate)
{
    if (gate && !*gate) return;
    const uint32_t* sid = mode == 1 ? cur_sid(sr) : nullptr;
    __shared__ uint32_t s_w[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kCompactTile;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t run = offs[blockIdx.x];
    for (int r = 0; r < kCompactItems; ++r) {       // rounds of 256 consecutive items, in order
        const uint64_t i = base + (uint64_t)r * kBlock + threadIdx.x;
        const bool sel = i < n && compact_pred(mode, i, ref, sid);
        const uint64_t b = __ballot(sel);
        if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pos = run + (uint32_t)__popcll(b & below);
        for (uint32_t w = 0; w < wave; ++w) pos += s_w[w];
        if (sel) out[pos] = (uint32_t)i;
        run += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

// ---- the window arithmetic (eslam_detmath.h DM_LM_*, the oracle's or_map_update) -------
__device__ __forceinline__ uint32_t lm_div(uint32_t a, uint64_t m) { return (uint32_t)(((uint64_t)a * m) >> kLmMagicShift); }
__device__ __forceinline__ uint32_t lm_mod(uint32_t a, uint32_t w, uint64_t m) { return a - w * lm_div(a, m); }
// the tile of slot column s in the window [c - h, c + h] (= dm_lm_tile_of): lo + ((s - lo) mod w)
// evaluated on s + (b - lo) with b a multiple of w >= 2^29, so the residue's argument is positive
__device__ __forceinline__ int32_t lm_tile(uint32_t s, int32_t c, uint32_t h, uint32_t w, uint64_t m, uint32_t b)
{
    const int32_t lo = c - (int32_t)h;
    return lo + (int32_t)lm_mod(s + (uint32_t)((int32_t)b - lo), w, m);
}
__device__ __forceinline__ bool lm_in(int32_t a, int32_t c, uint32_t h)
{
    const int32_t d = a - c;
    return d <= (int32_t)h && -d <= (int32_t)h;
}

// ---- the trail (eslam_internal.h LocalMaps; the oracle's lm_trail_* and lm_recentre): a
// table's tiles outside its window, V entries {a, b, page, -} closing its row.  The last word
// before them holds the trail's high-water mark hw (DM_LM_NONE: 0): entries from hw on are
// empty and are neither read nor copied (their words may be stale).  The word before that is
// the shadow flag.  Neither is a window slot: dm_lm_row_words reserves both after the
// (2 hx + 1)(2 hy + 1) slots whatever the parities of hx and hy
__device__ __forceinline__ uint32_t lm_trail_off(const LocalMaps& lm) { return lm.S - 4u * lm.V; }
__device__ __forceinline__ uint32_t lm_hw_word(uint32_t w) { return w == DM_LM_NONE ? 0u : w; }
__device__ __forceinline__ int32_t lm_cheb(int32_t a, int32_t b, int32_t na, int32_t nb)
{
    const int32_t da = a > na ? a - na : na - a, db = b > nb ? b - nb : nb - b;
    return da > db ? da : db;
}
// tile (a, b) into the trail of row: the first empty entry, else in place of the entry farthest
// from (na, nb) (the first such) when that one is farther than the tile; 1 when a tile was forgotten
__device__ __forceinline__ uint32_t lm_trail_push(const LocalMaps& lm, uint32_t* row, int32_t na, int32_t nb, int32_t a, int32_t b,
                                                  uint32_t pg)
{
    uint4* t = reinterpret_cast<uint4*>(row + lm_trail_off(lm));
    const uint32_t hw = lm_hw_word(row[lm_trail_off(lm) - 1u]);
    int32_t far = -1;
    uint32_t fe = 0;
    for (uint32_t e = 0; e < hw; ++e) {
        const uint4 v = t[e];
        if (v.z == DM_LM_NONE) {
            t[e] = make_uint4((uint32_t)a, (uint32_t)b, pg, DM_LM_NONE);
            return 0u;
        }
        const int32_t d = lm_cheb((int32_t)v.x, (int32_t)v.y, na, nb);
        if (d > far) { far = d; fe = e; }
    }
    if (hw < lm.V) {                                     // the first entry never used
        t[hw] = make_uint4((uint32_t)a, (uint32_t)b, pg, DM_LM_NONE);
        row[lm_trail_off(lm) - 1u] = hw + 1u;
        return 0u;
    }
    if (lm.V && far > lm_cheb(a, b, na, nb)) t[fe] = make_uint4((uint32_t)a, (uint32_t)b, pg, DM_LM_NONE);
    return 1u;
}

constexpr uint32_t kLmList = 8;                 // tiles one pass of the merge handles
constexpr uint16_t kCodeSkip = 0xffffu;
constexpr uint32_t kLmNoList = 0xffffffffu;

// one particle as a map update sees it: its table, its pose, the window's new centre
struct LmPart {
    uint32_t X;                          // the table it names
    bool shared;                         // another particle names X too
    bool placed;                         // finite x, y, theta (else the update skips it)
    double x, y, th, z, zs;
    double sn, co;
    int32_t na, nb;                      // the new centre
};

__device__ __forceinline__ void lm_centre(const MapView& map, const MergeParams& mp, const LmPart& q, int32_t& na, int32_t& nb)
{
    if (mp.is_id) {
        na = dm_lm_centre(q.x, map.offset_x, map.inv_scale_x);
        nb = dm_lm_centre(q.y, map.offset_y, map.inv_scale_y);
    } else {
        const double* A = map.g2l;
        const double lx = ((A[0] * q.x + A[1] * q.y) + A[2] * q.z) + A[3];
        const double ly = ((A[4] * q.x + A[5] * q.y) + A[6] * q.z) + A[7];
        na = dm_lm_centre(lx, map.offset_x, map.inv_scale_x);
        nb = dm_lm_centre(ly, map.offset_y, map.inv_scale_y);
    }
}

// scan patch k's code for this particle: (slot << 6) | cell in the tile, or kCodeSkip (off
// the grid or outside the window).  Counts the dropped patches; cell_out: the grid cell
// (0xffffffff off the grid), whose occupancy bit the callers test eight patches at a time
// (a cell the shared grid covers: merged into the particle's own copy of it, which the
// merge starts from the grid's patch)
__device__ __forceinline__ uint16_t lm_code(const MapView& map, const LocalMaps& lm, const MergeParams& mp, const LmPart& q,
                                            uint32_t k, uint32_t& cell_out, uint32_t& dropped)
{
    const double bx = q.x - map.offset_x, by = q.y - map.offset_y;
    {
        const ScanPatch sp = mp.sp[k];
        uint32_t cell, cm, cn;
        if (mp.is_id) {
            cell = dm_merge_cell_mn(bx, by, q.co, q.sn, sp.x, sp.y, map.inv_scale_x, map.inv_scale_y, map.width,
                                    map.height_cells, &cm, &cn);
        } else {
            const double wx = (q.co * sp.x + (-q.sn) * sp.y) + q.x;
            const double wy = (q.sn * sp.x + q.co * sp.y) + q.y;
            const double wz = sp.z + q.z;
            const double* A = map.g2l;
            const double lx = ((A[0] * wx + A[1] * wy) + A[2] * wz) + A[3];
            const double ly = ((A[4] * wx + A[5] * wy) + A[6] * wz) + A[7];
            const double fm = floor((lx - map.offset_x) * map.inv_scale_x);
            const double fn = floor((ly - map.offset_y) * map.inv_scale_y);
            const bool in = (fm >= 0.0) & (fm < (double)map.width) & (fn >= 0.0) & (fn < (double)map.height_cells);
            cm = in ? (uint32_t)fm : 0u;
            cn = in ? (uint32_t)fn : 0u;
            cell = in ? cn * map.width + cm : 0xffffffffu;
        }
        uint16_t code = kCodeSkip;
        cell_out = cell;
        if (cell != 0xffffffffu) {
            const uint32_t a = cm >> DM_LM_TILE_BITS, b = cn >> DM_LM_TILE_BITS;
            if (dm_lm_inside(a, q.na, lm.hx, lm.wx) && dm_lm_inside(b, q.nb, lm.hy, lm.wy)) {
                const uint32_t s = lm_mod(a, lm.wx, lm.mx) + lm.wx * lm_mod(b, lm.wy, lm.my);
                code = (uint16_t)((s << 6) | ((cm & 7u) + 8u * (cn & 7u)));
            } else {
                ++dropped;                   // beyond maxSensorRange: outside the window
            }
        }
        return code;
    }
}

// how many of eight cells the shared grid covers: the eight occupancy words in one round trip
__device__ __forceinline__ uint32_t lm_covered8(const MapView& map, const uint32_t (&cell)[8])
{
    uint32_t w[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) w[j] = cell[j] != 0xffffffffu ? map.occ[cell[j] >> 5] : 0u;
    uint32_t n = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) n += (w[j] >> (cell[j] & 31u)) & 1u;
    return n;
}

// every scan patch's code into LDS (patch-major, thread-minor: a part of kScanPartSmall)
__device__ __forceinline__ void lm_codes(const MapView& map, const LocalMaps& lm, const MergeParams& mp, const LmPart& q,
                                         uint16_t* codes, uint32_t& covered, uint32_t& dropped)
{
    for (uint32_t k0 = 0; k0 < mp.m; k0 += 8) {
        uint32_t cell[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            cell[j] = 0xffffffffu;
            if (k0 + j < mp.m) codes[(k0 + j) * kLmBlock] = lm_code(map, lm, mp, q, k0 + j, cell[j], dropped);
        }
        covered += lm_covered8(map, cell);
    }
}

// slot s into the sorted list of the kLmList smallest distinct slots; more: a slot fell off
__device__ __forceinline__ void lm_insert(uint32_t (&L)[kLmList], uint32_t s, bool& more)
{
    bool dup = false;
#pragma unroll
    for (uint32_t r = 0; r < kLmList; ++r) dup |= L[r] == s;
    if (dup) return;
    more |= L[kLmList - 1] != kLmNoList;
#pragma unroll
    for (uint32_t r = kLmList - 1; r >= 1; --r) L[r] = L[r - 1] > s ? L[r - 1] : (L[r] > s ? s : L[r]);
    L[0] = L[0] > s ? s : L[0];
}

// a large part: every code straight to the particle's row of the codes buffer (eight per
// 16-byte store), and the first pass's tiles collected on the way (L; more: further tiles)
__device__ __forceinline__ void lm_codes_row(const MapView& map, const LocalMaps& lm, const MergeParams& mp, const LmPart& q,
                                             uint4* row, uint32_t (&L)[kLmList], bool& more, uint32_t& covered, uint32_t& dropped)
{
#pragma unroll
    for (uint32_t r = 0; r < kLmList; ++r) L[r] = kLmNoList;
    more = false;
    for (uint32_t k0 = 0; k0 < mp.m; k0 += 8) {
        uint32_t w[4], cell[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t k = k0 + j;
            cell[j] = 0xffffffffu;
            const uint32_t c = k < mp.m ? (uint32_t)lm_code(map, lm, mp, q, k, cell[j], dropped) : (uint32_t)kCodeSkip;
            if (c != kCodeSkip) lm_insert(L, c >> 6, more);
            w[j >> 1] = (j & 1) ? (w[j >> 1] | (c << 16)) : c;
        }
        row[k0 >> 3] = make_uint4(w[0], w[1], w[2], w[3]);
        covered += lm_covered8(map, cell);
    }
}

// the up to kLmList smallest distinct slots above t of a particle's codes row
__device__ __forceinline__ void lm_collect_row(const uint4* row, uint32_t m, uint32_t t, uint32_t (&L)[kLmList])
{
#pragma unroll
    for (uint32_t r = 0; r < kLmList; ++r) L[r] = kLmNoList;
    bool more = false;
    for (uint32_t k0 = 0; k0 < m; k0 += 8) {
        const uint4 v = row[k0 >> 3];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t c = (w[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
            if (k0 + j >= m || c == kCodeSkip) continue;
            const uint32_t s = c >> 6;
            if (s > t) lm_insert(L, s, more);
        }
    }
}

// the up to kLmList smallest distinct slots above t (sorted; free entries kLmNoList)
__device__ __forceinline__ void lm_collect(const uint16_t* codes, uint32_t m, uint32_t t, uint32_t (&L)[kLmList])
{
#pragma unroll
    for (uint32_t r = 0; r < kLmList; ++r) L[r] = kLmNoList;
    for (uint32_t k = 0; k < m; ++k) {
        const uint16_t c = codes[k * kLmBlock];
        if (c == kCodeSkip) continue;
        const uint32_t s = (uint32_t)c >> 6;
        if (t != kLmNoList && s <= t) continue;
        bool dup = false;
#pragma unroll
        for (uint32_t r = 0; r < kLmList; ++r) dup |= L[r] == s;
        if (dup) continue;
#pragma unroll
        for (uint32_t r = kLmList - 1; r >= 1; --r) L[r] = L[r - 1] > s ? L[r - 1] : (L[r] > s ? s : L[r]);
        L[0] = L[0] > s ? s : L[0];
    }
}

__device__ __forceinline__ uint32_t lm_find(const uint32_t (&L)[kLmList], uint32_t s)
{
    uint32_t idx = kLmNoList;
#pragma unroll
    for (uint32_t r = 0; r < kLmList; ++r) idx = L[r] == s ? r : idx;
    return idx;
}

// the plan's table step (the oracle's lm_recentre; copy on write): table T's row and centre
// from X's, the window moved to (na, nb): (1) the tiles leaving it go to the trail in slot
// order, (2) the trail's tiles inside the new window go back to their slots.  T != X: X is
// shared, T a free table written whole.  A lane per particle; returns the tiles forgotten.
__device__ uint32_t lm_rewrite(const LocalMaps& lm, uint32_t X, uint32_t T, int2 oc, int32_t na, int32_t nb)
{
    uint32_t* row = lm.slot + (uint64_t)T * lm.S;
    const uint32_t toff = lm_trail_off(lm);
    if (X != T) {                                        // the window's words and the trail's used entries
        const uint4* src = reinterpret_cast<const uint4*>(lm.slot + (uint64_t)X * lm.S);
        uint4* dst = reinterpret_cast<uint4*>(row);
        const uint32_t nq = toff / 4u + lm_hw_word(lm.slot[(uint64_t)X * lm.S + toff - 1u]);
        for (uint32_t q = 0; q < nq; ++q) dst[q] = src[q];
    }
    uint32_t forgot = 0;
    if (oc.x != DM_LM_UNSET && (oc.x != na || oc.y != nb)) {
        // the window's columns and rows whose tiles leave it (bit sa / sb), then their slots in
        // slot order
        uint32_t colx = 0, rowx = 0;
        for (uint32_t sa = 0; sa < lm.wx; ++sa)
            colx |= lm_in(lm_tile(sa, oc.x, lm.hx, lm.wx, lm.mx, lm.bx), na, lm.hx) ? 0u : 1u << sa;
        for (uint32_t sb = 0; sb < lm.wy; ++sb)
            rowx |= lm_in(lm_tile(sb, oc.y, lm.hy, lm.wy, lm.my, lm.by), nb, lm.hy) ? 0u : 1u << sb;
        const uint32_t all = lm.wx >= 32u ? ~0u : (1u << lm.wx) - 1u;
        for (uint32_t sb = 0; sb < lm.wy; ++sb) {
            const int32_t b = lm_tile(sb, oc.y, lm.hy, lm.wy, lm.my, lm.by);
            for (uint32_t cols = ((rowx >> sb) & 1u) ? all : colx; cols; cols &= cols - 1u) {
                const uint32_t sa = (uint32_t)__builtin_ctz(cols);
                const uint32_t s = sa + lm.wx * sb, p = row[s];
                if (p == DM_LM_NONE) continue;
                forgot += lm_trail_push(lm, row, na, nb, lm_tile(sa, oc.x, lm.hx, lm.wx, lm.mx, lm.bx), b, p);
                row[s] = DM_LM_NONE;
            }
        }
        uint4* t = reinterpret_cast<uint4*>(row + toff);
        const uint32_t hw = lm_hw_word(row[toff - 1u]);
        for (uint32_t e = 0; e < hw; ++e) {
            const uint4 v = t[e];
            if (v.z == DM_LM_NONE || !lm_in((int32_t)v.x, na, lm.hx) || !lm_in((int32_t)v.y, nb, lm.hy)) continue;
            row[lm_mod(v.x, lm.wx, lm.mx) + lm.wx * lm_mod(v.y, lm.wy, lm.my)] = v.z;
            t[e] = make_uint4(v.x, v.y, DM_LM_NONE, DM_LM_NONE);
        }
    }
    lm.ctr[T] = make_int2(na, nb);
    return forgot;
}

// the particle of a map update: output i reads its ancestor through the marks when the merge
// runs the pending resample gather (fused), else itself
__device__ __forceinline__ uint32_t lm_source(const MergeParams& mp, uint64_t i, bool gath)
{
    uint32_t src = (uint32_t)i;
    if (gath) {
        const uint64_t row0 = i & ~(uint64_t)(kRow - 1);
        const uint32_t carry = row0 < mp.n ? mp.gv.row_first[row0 / kRow] + 1u : 0u;
        uint32_t mk = i < mp.n ? mp.gv.marks[i] : 0u;
        mk = wave_incl_max_u32(mk);
        src = (mk > carry ? mk : carry) - 1u;
    }
    return src;
}

__device__ __forceinline__ void lm_load(const DevState& in, uint32_t src, const MapView& map, const MergeParams& mp,
                                        const uint32_t* ref, LmPart& q)
{
    q.X = in.sid[src];
    q.shared = ref[q.X] > 1u;
    q.x = in.x[src]; q.y = in.y[src]; q.th = in.th[src]; q.z = in.z[src]; q.zs = in.zs[src];
    dm_sincos(q.th, &q.sn, &q.co);
    q.placed = dm_isfinite(q.x - map.offset_x) && dm_isfinite(q.y - map.offset_y) && dm_isfinite(q.th);
    q.na = q.nb = 0;
    if (q.placed) lm_centre(map, mp, q, q.na, q.nb);
}

// the exclusive prefix of the blocks' per-thread needs (off[t], thread t of the block) and the
// block's sum (*sum); s_w: kLmBlock / 64 words of LDS
__device__ __forceinline__ void block_offsets(uint32_t need, bool valid, uint32_t* off, uint32_t* sum, uint32_t* s_w)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t pfx = need;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)pfx, o, 64);
        pfx += lane >= (uint32_t)o ? v : 0u;
    }
    if (lane == 63) s_w[tid >> 6] = pfx;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < (tid >> 6); ++w) base += s_w[w];
    if (valid) off[tid] = base + pfx - need;
    if (tid == kLmBlock - 1) *sum = base + pfx;
}

// after the scan of the plan's block sums: whether the free list holds this update's pages
// (else the collection runs first)
__global__ void k_page_budget(Ctl* __restrict__ ctl, const uint32_t* __restrict__ poff, uint32_t nblocks)
{
    const uint64_t total = poff[nblocks];
    ctl->pg_total = total;
    ctl->pg_gc = ctl->pg_cursor + total > ctl->pg_nfree ? 1u : 0u;
}

// the collection: clear the marks, mark every page a live table (ref >= 1) names, compact the
// unmarked pages into LocalMaps::frees (k_compact_* mode 2), then k_page_budget2
__global__ void __launch_bounds__(kBlock) k_pg_clear(uint8_t* __restrict__ mark, uint64_t npages, const uint32_t* __restrict__ gate)
{
    if (!*gate) return;
    uint4* m4 = reinterpret_cast<uint4*>(mark);
    const uint64_t n16 = (npages + 15) / 16;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * kBlock)
        m4[i] = make_uint4(0u, 0u, 0u, 0u);
}

// one wave per table (grid-stride): its lanes walk the window's wx * wy slots (not the
// bookkeeping words after them, which are no page ids), then the trail's pages
__global__ void __launch_bounds__(kBlock) k_pg_mark(LocalMaps lm, const uint32_t* __restrict__ ref, const uint32_t* __restrict__ gate)
{
    if (!*gate) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    const uint32_t W = lm.wx * lm.wy, toff = lm.S - 4u * lm.V;
    for (uint64_t t = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); t < lm.ntables; t += nw) {
        if (ref[t] == 0u) continue;
        const uint32_t* sl = lm.slot + t * lm.S;
        for (uint32_t s = lane; s < W; s += 64u) {
            const uint32_t p = sl[s];
            if (p != DM_LM_NONE) lm.mark[p] = 1u;
        }
        const uint32_t hw = lm_hw_word(sl[toff - 1u]);
        for (uint32_t e = lane; e < hw; e += 64u) {
            const uint32_t p = sl[toff + 4u * e + 2u];
            if (p != DM_LM_NONE) lm.mark[p] = 1u;
        }
    }
}

__global__ void k_page_budget2(Ctl* __restrict__ ctl, const uint32_t* __restrict__ counts, uint32_t tiles,
                               uint32_t* fault)
{
    if (!ctl->pg_gc) return;
    ctl->pg_nfree = counts[tiles];
    ctl->pg_cursor = 0;
    if (ctl->pg_total > ctl->pg_nfree) {
        atomicOr((unsigned long long*)&ctl->err, (unsigned long long)kFaultPages);
        if (fault) __hip_atomic_fetch_or(fault, kFaultPages, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// processMap(scanMap, match = false, update = true) per particle (the oracle's or_map_update):
// the window moves to the tile under the particle (tiles that leave it are forgotten), then
// every scan patch, placed at the particle's pose (Translation(x, y, 0) * Rz(theta); the
// offset patch adds zPos and zSigma^2, src/EmbodiedSlamFilter.cpp:186-189, 213-214), merges
// into the cell it lands in: inserted into an empty cell (test/testMap.cpp:307-316) or fused
// (dm_lm_fuse) with the patch there.  The table the particle writes is its own (ref 1: in
// place) or, when shared, the free table frees[i] it then names.
// Two kernels.  k_map_plan (a lane per particle) does the lookups: the codes of the scan's
// cells, the tiles, their pages, whether the table owns them.  k_map_merge moves the data, a
// group of kLmLanes lanes per particle (four particles a wave), so that every access of the
// maps is a whole table or page moved by the group together (a lane per particle touching
// 8-byte cells scattered over 64 pages missed the caches on two of three accesses: r05h).
// Per particle:
//   1. the plan's record, the codes (PART / kLmLanes a lane, two to a register) and the allocation offset arrive in one
//      round trip; each patch is ranked among the earlier patches on its cell;
//   2. lane r of the group takes tile r of the first pass: a new page when the plan says the
//      table does not own it; a table copied on write or whose window moved is rewritten by
//      the group (evictions, the pass's new pages folded in);
//   3. kLmStage pages at a time are staged in LDS (each lane loads 32 B: whole 512-B pages),
//      the patches applied there rank by rank (scan order on every cell), and the changed or
//      new pages stored whole.  Tiles beyond kLmList (a later pass) are looked up by the group.
// A tile whose patches all turn out no-ops keeps the copy it got: the same values.
// 8 lanes per particle, 2 staged pages each, at most 128 VGPRs: 11.8 ms per merge at 8M against
// 12.4 for 16 lanes with 4 pages (r05 A/B, profiles/r05/ab_merge_lanes.log)
#ifndef ESLAM_LM_LANES
#define ESLAM_LM_LANES 8
#endif
#ifndef ESLAM_LM_STAGE
#define ESLAM_LM_STAGE 2
#endif
#ifndef ESLAM_LM_WPE
#define ESLAM_LM_WPE 4
#endif
constexpr uint32_t kLmLanes = ESLAM_LM_LANES;                       // lanes per particle: 8 or 16
constexpr uint32_t kLmMergeBlock = 128;
constexpr uint32_t kLmPpb = kLmMergeBlock / kLmLanes;               // particles per block
constexpr uint32_t kLmStage = ESLAM_LM_STAGE;                        // pages in LDS per particle
static_assert(kLmList <= kLmLanes && (kLmLanes == 8 || kLmLanes == 16) && kLmStage <= 4,
              "a lane per tile of a pass; 8 or 16 lanes; row masks of 8 bits per staged page in a word");
constexpr uint32_t kLmChunk = kLmLanes * 16;                         // bytes of a page a group moves per instruction
constexpr uint32_t kLmNq = DM_LM_PAGE_CELLS * 8 / kLmChunk;           // such chunks per page

// the lanes of a wave see each other's LDS writes (in-order LDS; no code motion across)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t grp_min(uint32_t v)
{
#pragma unroll
    for (int o = kLmLanes / 2; o >= 1; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, kLmLanes));
    return v;
}
__device__ __forceinline__ uint32_t grp_max(uint32_t v)
{
#pragma unroll
    for (int o = kLmLanes / 2; o >= 1; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, kLmLanes));
    return v;
}
__device__ __forceinline__ uint32_t grp_or(uint32_t v)
{
#pragma unroll
    for (int o = kLmLanes / 2; o >= 1; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, kLmLanes);
    return v;
}
__device__ __forceinline__ uint32_t grp_get(uint32_t v, uint32_t l) { return (uint32_t)__shfl((int)v, (int)l, kLmLanes); }

// the first patch of shared-grid cell ct (its MapView::cell_tab record) passing getPatch's
// 3-sigma gate against the local height lz (the oracle's or_mls_cell_patch); its stdev in *sd
__device__ __forceinline__ bool grid_cell_patch(const MapView& map, uint4 ct, double lz, double qv, double& mean,
                                                double* sd = nullptr)
{
    for (uint32_t k = ct.z; k < ct.z + ct.w; ++k) {
        const float2 pf = k == ct.z ? make_float2(__uint_as_float(ct.x), __uint_as_float(ct.y)) : map.patch[k];
        const double pm = (double)pf.x, ps = (double)pf.y;
        const double ph = map.height ? (double)map.height[k] : 0.0;
        double diff;
        if (ph > 0.0) {
            if (lz > pm) diff = lz - pm;
            else if (lz < pm - ph) diff = (pm - ph) - lz;
            else diff = 0.0;
        } else {
            diff = dm_fabs(pm - lz);
        }
        if (diff * diff < 9.0 * (ps * ps + qv)) {
            mean = pm;
            if (sd) *sd = ps;
            return true;
        }
    }
    return false;
}

// k_map_plan: per particle (a lane each: kLmBlock particles a block, so the latency of its
// chain of lookups -- state, table, page, owner -- overlaps across many particles) the cell
// codes of its scan (MergeParams::codes), the first pass's tiles with their pages and whether
// the table owns them (the MergeJob record), and the pages its merge takes: one per tile its
// scan reaches that its table cannot write in place (a new tile, or a page it does not own).
// The block sums give the allocation offsets (k_scan_excl).  A tile whose writes all turn out
// no-ops leaves its page unused (free again at the next collection).
template <uint32_t PART>
__global__ void __launch_bounds__(kLmBlock) k_map_plan(DevState s0, DevState s1, const Ctl* __restrict__ ctl, MapView map,
                                                       LocalMaps lm, MergeParams mp)
{
    // a small part's codes leave through LDS (then the records); a large part's go straight to
    // the rows (their LDS would cost the kernel its occupancy)
    __shared__ __attribute__((aligned(16))) uint16_t s_code[kScanPartSmall * kLmBlock];
    // the block sums' words alias the codes: the block holds exactly 16 KiB of LDS (a 17th
    // granule cost it a block per CU)
    uint32_t* s_w = reinterpret_cast<uint32_t*>(s_code);
    static_assert(sizeof(MergeJob) * kLmBlock <= sizeof(uint16_t) * kScanPartSmall * kLmBlock, "records in s_code");
    constexpr bool kSmall = PART == kScanPartSmall;
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kLmBlock, i = base + tid;
    const uint32_t nb = (uint32_t)(mp.n - base < kLmBlock ? mp.n - base : kLmBlock);     // particles of the block
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    const bool gath = mp.fuse && ctl->gather;
    const DevState in = gath ? (ctl->base ? s1 : s0) : st;
    const uint32_t src = lm_source(mp, i, gath);
    uint32_t need = 0, covered = 0, dropped = 0, forgot = 0;
    MergeJob jb;
    if (i < mp.n) {
        LmPart q;
        lm_load(in, src, map, mp, mp.ref, q);
        jb.X = q.X;
        jb.T = q.X;
        jb.gT = 0;
        jb.na = q.na;
        jb.nb = q.nb;
        jb.ox = jb.oy = DM_LM_UNSET;
        jb.flags = 0;
        jb.need = 0;
        jb.z = q.z;
        jb.zs = q.zs;
        jb.src = src;
#pragma unroll
        for (uint32_t r = 0; r < kLmList; ++r) { jb.L[r] = 0; jb.P[r] = DM_LM_NONE; }
        if (q.placed) {
            uint16_t* codes = s_code + tid;
            uint4* crow = reinterpret_cast<uint4*>(mp.codes + i * PART);
            uint32_t L[kLmList];
            bool more1 = false;
            const uint32_t cov0 = covered;
            if constexpr (kSmall) {
                lm_codes(map, lm, mp, q, codes, covered, dropped);
                lm_collect(codes, mp.m, kLmNoList, L);
            } else {
                lm_codes_row(map, lm, mp, q, crow, L, more1, covered, dropped);
            }
            const int2 oc = lm.ctr[q.X];
            const uint32_t T = q.shared ? mp.frees[i] : q.X;
            // the window moves to the particle (into T: a shared table is copied): from here on
            // every tile the scan reaches is in T's slots.  A shared table whose window stays is
            // copied by the merge (a group of lanes per particle moves the row coalesced); its
            // tiles are X's slots
            const bool moved = oc.x != q.na || oc.y != q.nb;
            if (moved) forgot = lm_rewrite(lm, q.X, T, oc, q.na, q.nb);
            const uint32_t* trow = lm.slot + (uint64_t)(moved ? T : q.X) * lm.S;
            const uint64_t gT = ((uint64_t)lm.tgen[T] << 32) | T;
            uint32_t nt = 0, bits = 0;
#pragma unroll
            for (uint32_t r = 0; r < kLmList; ++r) {
                if (L[r] == kLmNoList) continue;
                const uint32_t P = trow[L[r]];
                const bool mine = !q.shared && P != DM_LM_NONE && lm.owner[P] == gT;
                bits |= mine ? 0u : 1u << r;
                jb.L[r] = (uint16_t)L[r];
                jb.P[r] = P;
                ++nt;
            }
            need = __builtin_popcount(bits);
            // later passes (a scan reaching more than kLmList tiles): counted here, resolved by the merge
            bool more = false;
            for (uint32_t t = L[kLmList - 1]; t != kLmNoList && (kSmall || more1); t = L[kLmList - 1]) {
                if constexpr (kSmall) lm_collect(codes, mp.m, t, L);
                else lm_collect_row(crow, mp.m, t, L);
                if (L[0] == kLmNoList) break;
                more = true;
#pragma unroll
                for (uint32_t r = 0; r < kLmList; ++r) {
                    if (L[r] == kLmNoList) continue;
                    const uint32_t P = trow[L[r]];
                    need += (!q.shared && P != DM_LM_NONE && lm.owner[P] == gT) ? 0u : 1u;
                }
            }
            jb.T = T;
            jb.gT = gT;
            jb.ox = oc.x;
            jb.oy = oc.y;
            jb.need = bits;
            jb.flags = kJobPlaced | (q.shared ? kJobShared : 0u) | (more ? kJobMore : 0u) | (moved ? kJobMoved : 0u) |
                       (covered != cov0 ? kJobCovered : 0u) | (nt << 8);
        }
    }
    // the codes rows and the records leave through LDS, so every store is a whole 1-KiB line of
    // the wave (a lane per particle storing its own 128-byte record wrote 64 lines partially)
    __syncthreads();
    uint4* rows = reinterpret_cast<uint4*>(mp.codes + base * kScanPartSmall);
    for (uint32_t c = tid; kSmall && c < nb * (kScanPartSmall / 8); c += kLmBlock) {
        const uint32_t p = c / (kScanPartSmall / 8), k0 = (c % (kScanPartSmall / 8)) * 8;
        if (k0 >= mp.m) continue;
        uint32_t w[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t a = k0 + 2 * j < mp.m ? s_code[(k0 + 2 * j) * kLmBlock + p] : kCodeSkip;
            const uint32_t b = k0 + 2 * j + 1 < mp.m ? s_code[(k0 + 2 * j + 1) * kLmBlock + p] : kCodeSkip;
            w[j] = a | (b << 16);
        }
        rows[c] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
    uint4* srec = reinterpret_cast<uint4*>(s_code);
    if (i < mp.n) {
        const uint4* r = reinterpret_cast<const uint4*>(&jb);
#pragma unroll
        for (uint32_t k = 0; k < sizeof(MergeJob) / 16; ++k) srec[tid * (sizeof(MergeJob) / 16) + k] = r[k];
    }
    __syncthreads();
    uint4* jobs = reinterpret_cast<uint4*>(mp.job + base);
    for (uint32_t c = tid; c < nb * (sizeof(MergeJob) / 16); c += kLmBlock) jobs[c] = srec[c];
    covered = wave_sum_u32(covered);
    dropped = wave_sum_u32(dropped);
    forgot = wave_sum_u32(forgot);
    if ((tid & 63u) == 0) {                   // the update's dropped / covered patches, forgotten tiles (k_merge_counts)
        const uint32_t slot_c = (uint32_t)((blockIdx.x * (kLmBlock / 64) + (tid >> 6)) % kMergeCounterSlots);
        if (dropped) atomicAdd((unsigned long long*)&mp.cnt[slot_c], (unsigned long long)dropped);
        if (covered) atomicAdd((unsigned long long*)&mp.cnt[3 * kMergeCounterSlots + slot_c], (unsigned long long)covered);
        if (forgot) atomicAdd((unsigned long long*)&mp.cnt[6 * kMergeCounterSlots + slot_c], (unsigned long long)forgot);
    }
    __syncthreads();                          // every record has left s_code (s_w aliases it)
    block_offsets(need, i < mp.n, mp.off + (i - tid), mp.poff + blockIdx.x, s_w);
}

// the number of lower lanes of the 16-lane row holding the same code (c == 0xffffffff never
// matches): DPP row shifts, the group's lanes all active
template <int D>
__device__ __forceinline__ uint32_t row_same(uint32_t c, uint32_t l)
{
    if constexpr (D >= (int)kLmLanes) {
        return 0u;
    } else {
        const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)0xffffffff, (int)c, 0x110 + D, 0xf, 0xf, false);
        return (o == c && l >= (uint32_t)D) ? 1u : 0u;     // l >= D: the lane D lower is in the group
    }
}
__device__ __forceinline__ uint32_t row_rank(uint32_t c, uint32_t l)
{
    return row_same<1>(c, l) + row_same<2>(c, l) + row_same<3>(c, l) + row_same<4>(c, l) + row_same<5>(c, l) +
           row_same<6>(c, l) + row_same<7>(c, l) + row_same<8>(c, l) + row_same<9>(c, l) + row_same<10>(c, l) +
           row_same<11>(c, l) + row_same<12>(c, l) + row_same<13>(c, l) + row_same<14>(c, l) + row_same<15>(c, l);
}

// the staged pages of a wave: for stage page rr, chunk q (kLmChunk bytes) the groups' chunks
// lie side by side (one 16-byte LDS-DMA per lane fills [rr][q] for the whole wave: 1 KiB)
constexpr uint32_t kLmWaveStage = kLmStage * kLmNq * 1024;          // bytes per wave
__device__ __forceinline__ uint32_t lm_stage_off(uint32_t rr, uint32_t ci, uint32_t g)
{
    constexpr uint32_t cpc = kLmChunk / 8;                           // cells per chunk
    return (rr * kLmNq + ci / cpc) * 1024 + g * kLmChunk + (ci % cpc) * 8;
}
// a large part's 32 codes a lane: three waves a SIMD (168 VGPRs)
#define LM_MERGE_ATTR __attribute__((amdgpu_waves_per_eu(PART == kScanPartSmall ? ESLAM_LM_WPE : ESLAM_LM_WPE_LARGE)))
#ifndef ESLAM_LM_WPE_LARGE
#define ESLAM_LM_WPE_LARGE 3
#endif
template <uint32_t PART>
__global__ void __launch_bounds__(kLmMergeBlock) LM_MERGE_ATTR k_map_merge(DevState s0, DevState s1, Ctl* __restrict__ ctl, MapView map,
                                                             LocalMaps lm, MergeParams mp)
{
    constexpr uint32_t PER = PART / kLmLanes;                       // codes a lane holds
    constexpr uint32_t NCH = PART / 8 / kLmLanes;                   // 16-byte chunks of codes a lane loads
    static_assert(PART <= 256 && NCH >= 1 && kLmStage <= 4, "a list entry holds k (8 bits), the page (2) and the cell (6)");
    __shared__ __attribute__((aligned(16))) uint16_t s_code[kLmPpb][PART];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[kLmMergeBlock / 64][kLmWaveStage];
    static_assert(PART * 2 >= 2 * kLmList * 4, "pass 0's slot / new page pairs fit a particle's s_code");
    // a small part's patch heights and deviations, read by every round (a large part's come
    // from memory: their 4 KiB would cost the kernel a block per CU)
    constexpr bool kSpLds = PART <= kScanPartSmall;
    __shared__ double2 s_sp[kSpLds ? PART : 1];
    const uint32_t tid = threadIdx.x, l = tid & (kLmLanes - 1), pl = tid / kLmLanes, g = pl % (64 / kLmLanes), wv = tid >> 6;
    // once the codes are in registers (cpk), the particle's s_code holds pass 0's (slot, new
    // page) pairs of a copied table and then each stage's list of patches
    uint32_t* const s_np = reinterpret_cast<uint32_t*>(&s_code[pl][0]);
    uint16_t* const s_lst = &s_code[pl][0];
    const uint64_t i = (uint64_t)blockIdx.x * kLmPpb + pl;
    if (ctl->err & kFaultPages) return;       // the pool could not hold the plan: nothing is written
    const bool valid = i < mp.n;
    ESLAM_STAMP(g_stamps_mg, 0);
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;      // by value: no private copy of the arguments
    // a pending resample gather (mp.fuse, one GPU) runs here instead of in its own launch:
    // output i reads its ancestor (the plan's src) in state[base] and the merge writes the
    // whole particle, its table name included, to st = state[base ^ 1]
    const bool gath = mp.fuse && ctl->gather;
    const DevState in = gath ? (ctl->base ? s1 : s0) : st;
    // the plan's record, the codes and this particle's first page: one round trip
    uint32_t X = 0, T = 0, flags = 0, needb = 0, src = 0, Lr = kLmNoList, Pr = DM_LM_NONE;
    uint64_t gT = 0, alloc = 0;
    int32_t na = 0, nb = 0;
    double z = 0.0, zs = 0.0;
    uint4 c4[NCH];                            // chunks l, l + kLmLanes, ... of the row (8 codes each)
#pragma unroll
    for (uint32_t q = 0; q < NCH; ++q) c4[q] = make_uint4(0u, 0u, 0u, 0u);
    if (valid) {
        const MergeJob* J = mp.job + i;
        X = J->X; T = J->T; gT = J->gT;
        flags = J->flags; needb = J->need;
        na = J->na; nb = J->nb;
        z = J->z; zs = J->zs; src = J->src;
        if (l < kLmList) { Lr = J->L[l]; Pr = J->P[l]; }
        const uint4* crow = reinterpret_cast<const uint4*>(mp.codes + i * PART);
#pragma unroll
        for (uint32_t q = 0; q < NCH; ++q)
            if ((l + kLmLanes * q) * 8 < mp.m) c4[q] = crow[l + kLmLanes * q];
        if constexpr (NCH > 1) {              // a large part's codes to LDS at once (no registers held)
#pragma unroll
            for (uint32_t q = 0; q < NCH; ++q) reinterpret_cast<uint4*>(&s_code[pl][0])[l + kLmLanes * q] = c4[q];
        }
        alloc = ctl->pg_cursor + mp.poff[i / kLmBlock] + mp.off[i];
    }
    for (uint32_t k = tid; kSpLds && k < mp.m && k < PART; k += kLmMergeBlock) s_sp[k] = make_double2(mp.sp[k].z, mp.sp[k].stdev);
    if (gath && valid) {                      // the gather's copies: a field a lane
        for (uint32_t f = l; f < 10; f += kLmLanes) switch (f) {
        case 0: st.w[i] = in.w[src]; break;
        case 1: if (mp.aux) st.mprob[i] = in.mprob[src]; break;
        case 2: if (mp.aux) st.flags[i] = in.flags[src]; break;
        case 3: if (mp.gv.record) mp.gv.anc[i] = (uint32_t)(mp.gbase + src); break;
        case 4: if (mp.gv.marks[i]) mp.gv.marks[i] = 0u; break;
        case 5: st.x[i] = in.x[src]; break;
        case 6: st.y[i] = in.y[src]; break;
        case 7: st.th[i] = in.th[src]; break;
        case 8: st.z[i] = in.z[src]; break;
        case 9: st.zs[i] = in.zs[src]; break;
        default: break;
        }
    }
    bool dirty = false, moved = false, covw = false;
    uint32_t written = 0, taken = 0;
    const bool shared = (flags & kJobShared) != 0;
    if constexpr (kSpLds) __syncthreads();    // s_sp
    if (valid && (flags & kJobPlaced)) {      // group-uniform from here on
        // ---- 1. the codes: patch k = l + kLmLanes u in lane l (round u precedes round u + 1 in
        // the scan, so the rounds apply in order and only a round's own duplicates need ranks)
        if constexpr (NCH == 1) reinterpret_cast<uint4*>(&s_code[pl][0])[l] = c4[0];
        wave_sync();
        ESLAM_STAMP(g_stamps_mg, 1);
        // two 16-bit codes a register: code(u) is patch l + kLmLanes u (round 6: against one
        // code a register and against reading them from LDS, profiles/r06/ab/ab_r06k*, ab_r06l*)
        uint32_t cpk[(PER + 1) / 2];
#pragma unroll
        for (uint32_t v = 0; v < (PER + 1) / 2; ++v) {
            const uint32_t k0 = l + kLmLanes * (2 * v), k1 = k0 + kLmLanes;
            const uint32_t c0 = k0 < mp.m ? (uint32_t)s_code[pl][k0] : (uint32_t)kCodeSkip;
            const uint32_t c1 = (2 * v + 1 < PER && k1 < mp.m) ? (uint32_t)s_code[pl][k1] : (uint32_t)kCodeSkip;
            cpk[v] = c0 | (c1 << 16);
        }
        auto code = [&](uint32_t u) -> uint32_t { return (cpk[u >> 1] >> ((u & 1u) * 16u)) & 0xffffu; };
        // the plan has moved T's window (a moved shared X copied to T): every tile of the scan is
        // in T's slots, and the merge only adds the new pages -- but a shared X whose window
        // stays is copied to T here, the pass's new pages folded in
        const bool copy = shared && !(flags & kJobMoved);
        uint32_t* tsl = lm.slot + (uint64_t)T * lm.S;
        const uint32_t* xsl = lm.slot + (uint64_t)X * lm.S;
        const uint32_t gshift = (tid & 63u) & ~(kLmLanes - 1u);
        const double zvar = zs * zs;
        uint8_t* stage = &s_stage[wv][0];
        // stage: lane l moves bytes [16 l, 16 l + 16) of each chunk of the pages, straight into LDS
        auto stage_pages = [&](const uint32_t (&Ls)[kLmStage], const uint32_t (&Ps)[kLmStage]) {
#pragma unroll
            for (uint32_t rr = 0; rr < kLmStage; ++rr) {
#pragma unroll
                for (uint32_t h = 0; h < kLmNq; ++h) {
                    uint8_t* dst = stage + (rr * kLmNq + h) * 1024;
                    if (Ls[rr] != kLmNoList && Ps[rr] != DM_LM_NONE) {
                        const uint8_t* srcp = reinterpret_cast<const uint8_t*>(lm.page + (uint64_t)Ps[rr] * DM_LM_PAGE_CELLS) +
                                              h * kLmChunk + l * 16;
                        __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)srcp,
                                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
                    } else {
                        *reinterpret_cast<uint4*>(dst + (tid & 63u) * 16) =
                            make_uint4(0u, __float_as_uint(-1.0f), 0u, __float_as_uint(-1.0f));
                    }
                }
            }
        };
        uint32_t cnt = (flags >> 8) & 0xffu;
        int32_t lo = -1;
        for (uint32_t pass = 0;; ++pass) {
            // lane r: tile r of the pass, its page P, whether it takes a new page NP
            bool need = false;
            uint32_t P = DM_LM_NONE, NP = DM_LM_NONE;
            bool more;
            if (pass == 0) {
                if (l >= cnt) Lr = kLmNoList;
                P = Pr;
                need = l < cnt && ((needb >> l) & 1u);
                more = (flags & kJobMore) != 0;
                lo = cnt ? (int32_t)grp_get(Lr, cnt - 1) : -1;
                // the first stage's pages are known from the record: their loads overlap the
                // allocation and the table rewrite below
                uint32_t Ls0[kLmStage], Ps0[kLmStage];
#pragma unroll
                for (uint32_t rr = 0; rr < kLmStage; ++rr) {
                    Ls0[rr] = grp_get(Lr, rr);
                    Ps0[rr] = grp_get(P, rr);
                }
                stage_pages(Ls0, Ps0);
            } else {
                Lr = kLmNoList;
                for (cnt = 0; cnt < kLmList; ++cnt) {
                    uint32_t mn = kLmNoList;
#pragma unroll
                    for (uint32_t u = 0; u < PER; ++u) {
                        const uint32_t s = code(u) >> 6;
                        if (code(u) != kCodeSkip && (int32_t)s > lo) mn = min(mn, s);
                    }
                    mn = grp_min(mn);
                    if (mn == kLmNoList) break;
                    if (l == cnt) Lr = mn;
                    lo = (int32_t)mn;
                }
                uint32_t nx = kLmNoList;
#pragma unroll
                for (uint32_t u = 0; u < PER; ++u)
                    if (code(u) != kCodeSkip && (int32_t)(code(u) >> 6) > lo) nx = min(nx, code(u) >> 6);
                more = cnt == kLmList && grp_min(nx) != kLmNoList;
                if (l < cnt) {
                    __builtin_amdgcn_s_waitcnt(0);   // the group's stores of T's row (pass 0) have landed
                    P = tsl[Lr];
                    need = !(!shared && P != DM_LM_NONE && lm.owner[P] == gT);
                }
            }
            const uint32_t gmask = (uint32_t)(__ballot(need) >> gshift) & ((1u << kLmLanes) - 1u);
            if (need) {
                NP = lm.frees[alloc + __builtin_popcount(gmask & ((1u << l) - 1u))];
                lm.owner[NP] = gT;
                ++taken;
            }
            alloc += __builtin_popcount(gmask);
            // ---- 2. the table: the new pages into T's slots (a later pass: T's slot may have
            // been written by this group above -- the same wave, in order)
            if (pass == 0 && copy) {
                // X's row to T, four words a lane (each group instruction moves 128 contiguous
                // bytes), with this pass's new pages; the trail's words as they are
                if (l < kLmList) {
                    s_np[2 * l] = Lr;
                    s_np[2 * l + 1] = NP;
                }
                const uint32_t lmin = cnt ? grp_get(Lr, 0) : 1u, lmax = cnt ? grp_get(Lr, cnt - 1) : 0u;
                const uint32_t toff = lm_trail_off(lm), nq = toff / 4u + lm_hw_word(xsl[toff - 1u]);
                wave_sync();
                for (uint32_t q = l; q < nq; q += kLmLanes) {
                    uint4 w4 = reinterpret_cast<const uint4*>(xsl)[q];
                    if (4 * q + 3 >= lmin && 4 * q <= lmax) {
                        uint32_t v[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                        for (uint32_t e = 0; e < 4; ++e)
                            for (uint32_t r = 0; r < cnt; ++r)
                                if (s_np[2 * r] == 4 * q + e && s_np[2 * r + 1] != DM_LM_NONE) v[e] = s_np[2 * r + 1];
                        w4 = make_uint4(v[0], v[1], v[2], v[3]);
                    }
                    reinterpret_cast<uint4*>(tsl)[q] = w4;
                }
                if (l == 0) lm.ctr[T] = lm.ctr[X];
            } else if (need) {
                if (pass != 0) __builtin_amdgcn_s_waitcnt(0);
                tsl[Lr] = NP;
            }
            if (pass == 0) dirty = (flags & kJobMoved) != 0;
            // ---- 3. the pass's pages, kLmStage at a time through LDS
            for (uint32_t r0 = 0; r0 < cnt; r0 += kLmStage) {
                uint32_t Ls[kLmStage], Ps[kLmStage], Ds[kLmStage];
#pragma unroll
                for (uint32_t rr = 0; rr < kLmStage; ++rr) {
                    Ls[rr] = grp_get(Lr, r0 + rr);                 // kLmNoList beyond cnt
                    Ps[rr] = grp_get(P, r0 + rr);
                    const uint32_t npr = grp_get(NP, r0 + rr);
                    Ds[rr] = npr != DM_LM_NONE ? npr : Ps[rr];
                }
                if (pass != 0 || r0 != 0) {   // (pass 0's first stage was issued with the record)
                    wave_sync();              // the previous stage's stores have read LDS
                    stage_pages(Ls, Ps);
                }
                __builtin_amdgcn_s_waitcnt(0);
                wave_sync();
                if (pass == 0 && r0 == 0) ESLAM_STAMP(g_stamps_mg, 2);
                uint32_t wbits = 0;           // bit 8 rr + row: this lane wrote that 64-byte row of page rr
                // the stage's patches listed in scan order (k = l + kLmLanes u is u-major), then
                // applied kLmLanes at a time: a round's lanes on one cell go by rank (DPP row
                // compare), rounds in order -- every cell sees its patches in scan order
                // an entry: patch k, its staged page rr and its cell ci (k | rr << 8 | ci << 10)
                uint32_t nst = 0;
#pragma unroll
                for (uint32_t u = 0; u < PER; ++u) {
                    const uint32_t cu = code(u);
                    bool in = false;
                    uint32_t ru = 0;
#pragma unroll
                    for (uint32_t w = 0; w < kLmStage; ++w) {
                        const bool m = cu != kCodeSkip && Ls[w] == (cu >> 6);
                        in |= m;
                        ru = m ? w : ru;
                    }
                    const uint32_t gm = (uint32_t)(__ballot(in) >> gshift) & ((1u << kLmLanes) - 1u);
                    if (in)
                        s_lst[nst + __builtin_popcount(gm & ((1u << l) - 1u))] =
                            (uint16_t)((l + kLmLanes * u) | (ru << 8) | ((cu & 63u) << 10));
                    nst += __builtin_popcount(gm);
                }
                wave_sync();
                for (uint32_t j0 = 0; j0 < nst; j0 += kLmLanes) {
                    const bool act = j0 + l < nst;
                    const uint32_t e = act ? (uint32_t)s_lst[j0 + l] : 0u;
                    const uint32_t k = e & 0xffu;
                    // the patch first (every lane: k = 0 is a patch of the part), so a large part's
                    // load overlaps the ranking below
                    double2 sp;
                    if constexpr (kSpLds) {
                        sp = s_sp[k];
                    } else {
                        const ScanPatch* spk = mp.sp + k;
                        sp = make_double2(spk->z, spk->stdev);
                    }
                    const uint32_t c = act ? (e >> 8) : 0xfffffffeu - l;   // page and cell; idle lanes never match
                    const uint32_t rank = row_rank(c, l);
                    const uint32_t maxr = grp_max(act ? rank : 0u);
                    const uint32_t rr = (e >> 8) & 3u, ci = e >> 10;
                    // the patch, and for an empty cell the shared grid covers its occupancy word
                    // and record, are loaded together ahead of the ranks (cells are never emptied)
                    uint4 gct = make_uint4(0u, 0u, 0u, 0u);
                    uint32_t gocc = 0;
                    if (act) {
                        const float2 cv0 = *reinterpret_cast<const float2*>(stage + lm_stage_off(rr, ci, g));
                        if ((flags & kJobCovered) && !dm_lm_holds(cv0.y)) {
                            uint32_t sl = Ls[0];
#pragma unroll
                            for (uint32_t w = 1; w < kLmStage; ++w) sl = rr == w ? Ls[w] : sl;
                            const uint32_t sb = lm_div(sl, lm.mx), sa = sl - lm.wx * sb;
                            const uint32_t cm = 8u * (uint32_t)lm_tile(sa, na, lm.hx, lm.wx, lm.mx, lm.bx) + (ci & 7u);
                            const uint32_t cn = 8u * (uint32_t)lm_tile(sb, nb, lm.hy, lm.wy, lm.my, lm.by) + (ci >> 3);
                            const uint64_t cell = (uint64_t)cn * map.width + cm;
                            gocc = (map.occ[cell >> 5] >> (cell & 31u)) & 1u;
                            gct = map.cell_tab[cell];
                        }
                    }
                    for (uint32_t rk = 0; rk <= maxr; ++rk) {
                        if (act && rank == rk) {
                            float2* cp = reinterpret_cast<float2*>(stage + lm_stage_off(rr, ci, g));
                            const float2 cv = *cp;
                            const double wz = sp.x + z;
                            const double var = sp.y * sp.y + zvar;
                            float mo = cv.x, so = cv.y;
                            bool w = true, ins = true;
                            if (dm_lm_holds(cv.y)) {
                                w = dm_lm_fuse(cv.x, cv.y, wz, var, &mo, &so);
                                ins = false;
                            } else if (gocc) {
                                // a cell the shared grid covers: the particle's copy starts from
                                // the grid's patch the 3-sigma gate picks (the oracle alike)
                                double gm, gs;
                                if (grid_cell_patch(map, gct, wz, var, gm, &gs) &&
                                    dm_lm_fuse((float)gm, (float)gs, wz, var, &mo, &so)) {
                                    ins = false;
                                    covw = true;
                                }
                            }
                            if (ins) { mo = (float)wz; so = (float)dm_sqrt(var); }
                            if (w) {
                                *cp = make_float2(mo, so);
                                wbits |= 1u << (8u * rr + (ci >> 3));
                                ++written;
                            }
                        }
                        wave_sync();
                    }
                }
                wbits = grp_or(wbits);
                if (pass == 0 && r0 == 0) ESLAM_STAMP(g_stamps_mg, 3);
                static_assert(kLmStage <= 4 && kLmChunk == 128, "a lane's 16 bytes of a chunk lie in row 2 h + l / 4");
                // a new page goes back whole; a page the table owns, only the rows the patches changed
#pragma unroll
                for (uint32_t rr = 0; rr < kLmStage; ++rr) {
                    const uint32_t rows = (wbits >> (8u * rr)) & 0xffu;
                    const bool fresh = Ds[rr] != Ps[rr];
                    if (Ls[rr] == kLmNoList || (!fresh && !rows)) continue;
                    uint4* dp = reinterpret_cast<uint4*>(lm.page + (uint64_t)Ds[rr] * DM_LM_PAGE_CELLS);
#pragma unroll
                    for (uint32_t h = 0; h < kLmNq; ++h)
                        if (fresh || ((rows >> (2u * h + (l >> 2))) & 1u))
                            dp[kLmLanes * h + l] = *reinterpret_cast<const uint4*>(stage + (rr * kLmNq + h) * 1024 + (tid & 63u) * 16);
                }
                dirty = dirty || wbits != 0;
            }
            if (!more) break;
        }
        ESLAM_STAMP(g_stamps_mg, 4);
        if (shared && dirty) moved = true;
        if ((gath || moved) && l == 0) st.sid[i] = moved ? T : X;
        // the map now holds a copy of a shared-grid cell: its lookups ask its own cells first
        // (after T's row words have landed: the copy above may have written this word)
        if (grp_or(covw ? 1u : 0u) && l == 0) {
            __builtin_amdgcn_s_waitcnt(0);
            tsl[lm_trail_off(lm) - 2u] = kLmShadow;
        }
    } else if (valid && gath && l == 0) {
        st.sid[i] = X;
    }
    // the counters: particles once (the group's lane 0), cell writes and pages from every lane
    // (the plan counted the dropped and covered patches)
    const bool lead = l == 0;
    written = wave_sum_u32(written);
    taken = wave_sum_u32(taken);
    const uint64_t dmask = __ballot(lead && dirty), mmask = __ballot(lead && moved);
    if ((tid & 63u) == 0) {                   // one address per counter slot: no single hot atomic
        const uint32_t slot_c = (uint32_t)((blockIdx.x * (kLmMergeBlock / 64) + (tid >> 6)) % kMergeCounterSlots);
        if (written) atomicAdd((unsigned long long*)&mp.cnt[4 * kMergeCounterSlots + slot_c], (unsigned long long)written);
        if (taken) atomicAdd((unsigned long long*)&mp.cnt[5 * kMergeCounterSlots + slot_c], (unsigned long long)taken);
        if (dmask) atomicAdd((unsigned long long*)&mp.cnt[kMergeCounterSlots + slot_c], (unsigned long long)__popcll(dmask));
        if (mmask) atomicAdd((unsigned long long*)&mp.cnt[2 * kMergeCounterSlots + slot_c], (unsigned long long)__popcll(mmask));
    }
    ESLAM_STAMP(g_stamps_mg, 5);
}

// processMap(scanMap, match = true) per particle (the oracle's or_map_match; the rule is the
// build's own, envire's MLSGrid::match not being in the reference): every 10th scan patch,
// placed like the merge, scores on the cell it lands in -- a cell of the shared grid: the
// patch getPatch's 3-sigma gate picks (0 when none passes); with per-particle maps (PMAPS) an
// empty grid cell of the particle's own map, in a tile inside the window the update centres on
// the particle (from the window or the trail): its cell -- exp(-d^2 / (2 sigma^2)), sigma 0.2f
// (src/EmbodiedSlamFilter.cpp:217); the particle's weight is multiplied by pow(weight, 0.1f),
// weight the float mean score (1 when no patch counts).  A lane per particle; the sampled
// patches from the kernel arguments (scalar loads), kMatchBatch at a time: their grid records
// and table slots in one round trip, then the cells.
template <bool PMAPS>
__global__ void __launch_bounds__(kBlock) k_map_match(DevState s0, DevState s1, const Ctl* __restrict__ ctl, MapView map,
                                                      LocalMaps lm, MatchParams mp)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= mp.n) return;
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    const uint32_t X = PMAPS ? st.sid[i] : 0u;
    const double x = st.x[i], y = st.y[i], th = st.th[i], z = st.z[i], zs = st.zs[i], w = st.w[i];
    const double bx = x - map.offset_x, by = y - map.offset_y;
    if (!(dm_isfinite(bx) && dm_isfinite(by) && dm_isfinite(th))) return;
    double sn, co;
    dm_sincos(th, &sn, &co);
    const double zvar = zs * zs;
    const double* A = map.g2l;
    int32_t na = 0, nb = 0;
    int2 c = make_int2(0, 0);
    const uint32_t* row = nullptr;
    if constexpr (PMAPS) {
        if (mp.is_id) {
            na = dm_lm_centre(x, map.offset_x, map.inv_scale_x);
            nb = dm_lm_centre(y, map.offset_y, map.inv_scale_y);
        } else {
            na = dm_lm_centre(((A[0] * x + A[1] * y) + A[2] * z) + A[3], map.offset_x, map.inv_scale_x);
            nb = dm_lm_centre(((A[4] * x + A[5] * y) + A[6] * z) + A[7], map.offset_y, map.inv_scale_y);
        }
        c = lm.ctr[X];
        row = lm.slot + (uint64_t)X * lm.S;
    }
    double sum = 0.0;
    uint32_t cnt = 0;
    constexpr uint32_t kMatchBatch = 8;
    for (uint32_t k0 = 0; k0 < mp.m; k0 += kMatchBatch) {
        uint4 ct[kMatchBatch];
        uint32_t pg[kMatchBatch], cj[kMatchBatch], sl[kMatchBatch];
        double wzs[kMatchBatch], lzs[kMatchBatch], var[kMatchBatch];
        bool on[kMatchBatch], own[kMatchBatch];
#pragma unroll
        for (uint32_t q = 0; q < kMatchBatch; ++q) {
            const uint32_t k = k0 + q;
            on[q] = own[q] = false;
            ct[q] = make_uint4(0u, 0u, 0u, 0u);
            pg[q] = DM_LM_NONE;
            cj[q] = sl[q] = 0;
            wzs[q] = lzs[q] = var[q] = 0.0;
            if (k >= mp.m) continue;
            const ScanPatch sp = mp.sp ? mp.sp[k] : mp.spi[k];
            const double wz = sp.z + z;
            double lz = wz;
            uint32_t cm, cn;
            if (mp.is_id) {
                if (dm_merge_cell_mn(bx, by, co, sn, sp.x, sp.y, map.inv_scale_x, map.inv_scale_y, map.width,
                                     map.height_cells, &cm, &cn) == 0xffffffffu)
                    continue;
            } else {
                const double wx = (co * sp.x + (-sn) * sp.y) + x;
                const double wy = (sn * sp.x + co * sp.y) + y;
                const double lx = ((A[0] * wx + A[1] * wy) + A[2] * wz) + A[3];
                const double ly = ((A[4] * wx + A[5] * wy) + A[6] * wz) + A[7];
                lz = ((A[8] * wx + A[9] * wy) + A[10] * wz) + A[11];
                const double fm = floor((lx - map.offset_x) * map.inv_scale_x);
                const double fn = floor((ly - map.offset_y) * map.inv_scale_y);
                if (!((fm >= 0.0) & (fm < (double)map.width) & (fn >= 0.0) & (fn < (double)map.height_cells))) continue;
                cm = (uint32_t)fm;
                cn = (uint32_t)fn;
            }
            on[q] = true;
            wzs[q] = wz;
            lzs[q] = lz;
            var[q] = sp.stdev * sp.stdev + zvar;
            ct[q] = map.cell_tab[(uint64_t)cn * map.width + cm];
            if constexpr (PMAPS) {
                const uint32_t a = cm >> DM_LM_TILE_BITS, b = cn >> DM_LM_TILE_BITS;
                if (dm_lm_inside(a, na, lm.hx, lm.wx) && dm_lm_inside(b, nb, lm.hy, lm.wy)) {
                    own[q] = true;
                    cj[q] = (cm & 7u) + 8u * (cn & 7u);
                    const bool inw = dm_lm_inside(a, c.x, lm.hx, lm.wx) && dm_lm_inside(b, c.y, lm.hy, lm.wy);
                    sl[q] = inw ? row[lm_mod(a, lm.wx, lm.mx) + lm.wx * lm_mod(b, lm.wy, lm.my)] : DM_LM_NONE;
                    if (!inw) {                  // a tile the window has left: the trail (rare)
                        const uint4* t = reinterpret_cast<const uint4*>(row + lm_trail_off(lm));
                        const uint32_t hw = lm_hw_word(row[lm_trail_off(lm) - 1u]);
                        for (uint32_t e = 0; e < hw; ++e) {
                            const uint4 v = t[e];
                            if (v.z != DM_LM_NONE && v.x == a && v.y == b) sl[q] = v.z;
                        }
                    }
                }
            }
        }
        float2 cv[kMatchBatch];
#pragma unroll
        for (uint32_t q = 0; q < kMatchBatch; ++q) {
            pg[q] = (PMAPS && own[q]) ? sl[q] : DM_LM_NONE;
            cv[q] = pg[q] != DM_LM_NONE ? lm.page[(uint64_t)pg[q] * DM_LM_PAGE_CELLS + cj[q]] : make_float2(0.0f, -1.0f);
        }
#pragma unroll
        for (uint32_t q = 0; q < kMatchBatch; ++q) {
            if (!on[q]) continue;
            if (pg[q] != DM_LM_NONE && dm_lm_holds(cv[q].y)) {     // the particle's own cell first
                const double d = wzs[q] - (double)cv[q].x;
                sum += dm_exp(-(d * d) / (2.0 * kMatchSigma * kMatchSigma));
                ++cnt;
            } else if (ct[q].w != 0u) {          // a cell of the shared grid
                double mean;
                if (grid_cell_patch(map, ct[q], lzs[q], var[q], mean)) {
                    const double d = lzs[q] - mean;
                    sum += dm_exp(-(d * d) / (2.0 * kMatchSigma * kMatchSigma));
                }
                ++cnt;
            }
        }
    }
    const float wf = cnt ? (float)(sum / (double)cnt) : 1.0f;
    st.w[i] = w * dm_pow((double)wf, (double)0.1f);
}

// the merge's statistics slots -> ctl (one block of kMergeCounterSlots threads); the free
// list's cursor moves past this update's plan
__global__ void __launch_bounds__(kMergeCounterSlots) k_merge_counts(const uint64_t* __restrict__ cnt, Ctl* __restrict__ ctl,
                                                                      uint32_t acc)
{
    __shared__ uint64_t s[kMergeCounters][kMergeCounterSlots / 64];
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (uint32_t g = 0; g < kMergeCounters; ++g) {
        const uint64_t v = wave_sum_u64(cnt[g * kMergeCounterSlots + t]);
        if ((t & 63u) == 0) s[g][t >> 6] = v;
    }
    __syncthreads();
    if (t == 0) {
        uint64_t r[kMergeCounters] = {0, 0, 0, 0, 0, 0, 0};
        for (uint32_t g = 0; g < kMergeCounters; ++g)
            for (uint32_t w = 0; w < kMergeCounterSlots / 64; ++w) r[g] += s[g][w];
        // acc: a later part of a scan merged 64 patches at a time (eslam_gpu_map_update) adds
        if (acc) {
            ctl->map_dropped += r[0]; ctl->map_changed += r[1]; ctl->map_copied += r[2];
            ctl->map_covered += r[3]; ctl->map_written += r[4]; ctl->map_taken += r[5];
            ctl->map_evicted += r[6];
        } else {
            ctl->map_dropped = r[0]; ctl->map_changed = r[1]; ctl->map_copied = r[2];
            ctl->map_covered = r[3]; ctl->map_written = r[4]; ctl->map_taken = r[5];
            ctl->map_evicted = r[6];
        }
        if (!(ctl->err & kFaultPages)) ctl->pg_cursor += ctl->pg_total;
    }
}

// the free list's cursor moves past a plan (the received maps' pages)
__global__ void k_pg_advance(Ctl* __restrict__ ctl)
{
    if (!(ctl->err & kFaultPages)) ctl->pg_cursor += ctl->pg_total;
}

}  // namespace eslam_dev

// ---------------------------------------------------------------------------------------
// launchers (called by the host side, eslam_ctx.hip and eslam_host_*.hip)
// ---------------------------------------------------------------------------------------
using namespace eslam_dev;

extern "C" hipError_t eslam_launch_store_init(uint32_t* sid, const LocalMaps* lm, uint64_t n, uint64_t pool, hipStream_t stream)
{
    uint64_t items = pool * lm->S;
    if (lm->npages > items) items = lm->npages;
    const uint64_t want = (items + kBlock - 1) / kBlock;
    if (items) hipLaunchKernelGGL(k_store_init, dim3((uint32_t)(want < 65536 ? want : 65536)), dim3(kBlock), 0, stream, sid, *lm, n,
                                  pool, items);
    return hipGetLastError();
}

// one compaction (k_compact_count, the exclusive prefix over tiles + 1 entries -- entry tiles
// becomes the total, copied to *total when total is not null -- and k_compact_write) of the
// items [0, items); gate: see k_compact_count
static hipError_t compact(int mode, uint64_t items, const uint32_t* ref, SidRef sid, uint32_t* counts, uint32_t* out,
                          uint32_t* total, hipStream_t stream, const uint32_t* gate = nullptr)
{
    const uint32_t tiles = (uint32_t)((items + kCompactTile - 1) / kCompactTile);
    hipError_t e = hipMemsetAsync(counts + tiles, 0, 4, stream);
    if (e != hipSuccess) return e;
    if (tiles) hipLaunchKernelGGL(k_compact_count, dim3(tiles), dim3(kBlock), 0, stream, mode, items, ref, sid, counts, gate);
    e = eslam_launch_scan_excl(counts, (uint64_t)tiles + 1, stream);
    if (e != hipSuccess) return e;
    if (tiles) hipLaunchKernelGGL(k_compact_write, dim3(tiles), dim3(kBlock), 0, stream, mode, items, ref, sid, counts, out, gate);
    return total ? hipMemcpyAsync(total, counts + tiles, 4, hipMemcpyDeviceToDevice, stream) : hipGetLastError();
}

// the tables' reference counts (and generations) and the free-table list of the pool (before a
// map merge or a copy on write): cs.ref, cs.frees, *cs.nfree
extern "C" hipError_t eslam_launch_store_refs(SidRef sid, uint64_t n, uint64_t pool, const CowScratch* cs, const GatherView* gv,
                                              uint32_t* tgen, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(cs->ref, 0, pool * 4, stream);
    if (e != hipSuccess) return e;
    GatherView g;
    memset(&g, 0, sizeof(g));
    if (gv) g = *gv;
    if (n) hipLaunchKernelGGL(k_store_ref, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, sid, n, cs->ref,
                              g, gv ? 1u : 0u, tgen);
    e = compact(0, pool, cs->ref, sid, cs->counts, cs->frees, cs->nfree, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

// the page budget of a plan (mp->poff holds the block sums of mp->need over nblocks blocks):
// the offsets, and a collection when the free list runs short (the gated kernels return at
// once otherwise).  pgc: the collection's compaction counts (npages / kCompactTile + 1 words)
static hipError_t page_budget(Ctl* ctl, const LocalMaps* lm, const MergeParams* mp, uint32_t nblocks, uint32_t* pgc,
                              hipStream_t stream)
{
    hipError_t e = eslam_launch_scan_excl(mp->poff, (uint64_t)nblocks + 1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_page_budget, dim3(1), dim3(1), 0, stream, ctl, mp->poff, nblocks);
    const uint32_t* gate = &ctl->pg_gc;
    const uint64_t n16 = (lm->npages + 15) / 16;
    const uint64_t gcl = (n16 + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_pg_clear, dim3((uint32_t)(gcl < 8192 ? gcl : 8192)), dim3(kBlock), 0, stream, lm->mark, lm->npages, gate);
    const uint64_t gm = (lm->ntables + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(k_pg_mark, dim3((uint32_t)(gm < 16384 ? gm : 16384)), dim3(kBlock), 0, stream, *lm, mp->ref, gate);
    const SidRef none{nullptr, nullptr, nullptr};
    e = compact(2, lm->npages, reinterpret_cast<const uint32_t*>(lm->mark), none, pgc, lm->frees, nullptr, stream, gate);
    if (e != hipSuccess) return e;
    const uint32_t tiles = (uint32_t)((lm->npages + kCompactTile - 1) / kCompactTile);
    hipLaunchKernelGGL(k_page_budget2, dim3(1), dim3(1), 0, stream, ctl, pgc, tiles, mp->fault);
    return hipGetLastError();
}

// a map update in two halves (timed apart): the plan (k_map_plan, the page budget and, when
// the free list runs short, the collection), then the merge and its counters
extern "C" hipError_t eslam_launch_map_plan(DevState s0, DevState s1, Ctl* ctl, const MapView* map, const LocalMaps* lm,
                                            const MergeParams* mp, uint32_t* pgc, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(mp->cnt, 0, kMergeCounters * kMergeCounterSlots * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t nb = (uint32_t)((mp->n + kLmBlock - 1) / kLmBlock);
    e = hipMemsetAsync(mp->poff + nb, 0, 4, stream);
    if (e != hipSuccess) return e;
    if (nb && mp->m > kScanPartSmall)
        hipLaunchKernelGGL(k_map_plan<kScanPartLarge>, dim3(nb), dim3(kLmBlock), 0, stream, s0, s1, ctl, *map, *lm, *mp);
    else if (nb)
        hipLaunchKernelGGL(k_map_plan<kScanPartSmall>, dim3(nb), dim3(kLmBlock), 0, stream, s0, s1, ctl, *map, *lm, *mp);
    return page_budget(ctl, lm, mp, nb, pgc, stream);
}

extern "C" hipError_t eslam_launch_map_match(DevState s0, DevState s1, const Ctl* ctl, const MapView* map, const LocalMaps* lm,
                                             const MatchParams* mp, hipStream_t stream)
{
    const uint64_t blocks = (mp->n + kBlock - 1) / kBlock;
    if (blocks && lm) hipLaunchKernelGGL(k_map_match<true>, dim3((uint32_t)blocks), dim3(kBlock), 0, stream, s0, s1, ctl, *map, *lm, *mp);
    if (blocks && !lm) {
        LocalMaps none;
        memset(&none, 0, sizeof(none));
        hipLaunchKernelGGL(k_map_match<false>, dim3((uint32_t)blocks), dim3(kBlock), 0, stream, s0, s1, ctl, *map, none, *mp);
    }
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_map_merge(DevState s0, DevState s1, Ctl* ctl, const MapView* map, const LocalMaps* lm,
                                             const MergeParams* mp, hipStream_t stream)
{
    const uint32_t nb = (uint32_t)((mp->n + kLmPpb - 1) / kLmPpb);
    if (nb && mp->m > kScanPartSmall)
        hipLaunchKernelGGL(k_map_merge<kScanPartLarge>, dim3(nb), dim3(kLmMergeBlock), 0, stream, s0, s1, ctl, *map, *lm, *mp);
    else if (nb)
        hipLaunchKernelGGL(k_map_merge<kScanPartSmall>, dim3(nb), dim3(kLmMergeBlock), 0, stream, s0, s1, ctl, *map, *lm, *mp);
    hipLaunchKernelGGL(k_merge_counts, dim3(1), dim3(kMergeCounterSlots), 0, stream, mp->cnt, ctl, mp->acc);
    return hipGetLastError();
}

// ---- sharded filters: the maps travel with the migrating particles -----------------------
// k_pack's companion: each record's map header (its source's table centre and page count).
// A record is one output; the copies of one source that go to one rank are consecutive
// records, and only the first of them carries the map (the others share it: one table and one
// set of pages on the receiver, as the copies share them here)
__device__ __forceinline__ bool pay_shares(const Rec* send, uint64_t j, const PaySeg& seg)
{
    if (j == 0 || (send[j].src >> 8) != (send[j - 1].src >> 8)) return false;
    for (int32_t d = 0; d <= seg.n; ++d)
        if (seg.off[d] == j) return false;               // the first record for a destination
    return true;
}

__global__ void __launch_bounds__(kBlock) k_pay_hdr(const DevState s0, const DevState s1, const Ctl* __restrict__ ctl,
                                                   const Rec* __restrict__ send, uint64_t nsend, uint64_t gbase, LocalMaps lm,
                                                   PaySeg seg, MapPayHdr* __restrict__ hdr)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    const DevState st = ctl->base ? s1 : s0;
    for (uint64_t j = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); j < nsend; j += nw) {
        const uint64_t i = (send[j].src >> 8) - gbase;
        const uint32_t X = st.sid[i];
        const bool share = pay_shares(send, j, seg);
        const uint32_t* row = lm.slot + (uint64_t)X * lm.S;
        const uint32_t W = lm.wx * lm.wy, toff = lm.S - 4u * lm.V;
        uint32_t c = 0;
        if (!share) {                                    // the window's slots and the trail's used entries
            for (uint32_t s = lane; s < W; s += 64u) c += row[s] != DM_LM_NONE ? 1u : 0u;
            const uint32_t hw = lm_hw_word(row[toff - 1u]);
            for (uint32_t e = lane; e < hw; e += 64u) c += row[toff + 4u * e + 2u] != DM_LM_NONE ? 1u : 0u;
            c = wave_sum_u32(c);
        }
        if (lane == 0) {
            MapPayHdr h;
            h.ctr = lm.ctr[X];
            h.npg = c;
            h.share = (share ? 1u : 0u) | (row[toff - 2u] == kLmShadow ? 2u : 0u);
            hdr[j] = h;
        }
    }
}

// the records' pages in the records' order (off: exclusive prefix of the headers' npg), the
// window's in slot order then the trail's in entry order; one wave per record: its lanes copy
// each page's 64 cells
__global__ void __launch_bounds__(kBlock) k_pay_pack(const DevState s0, const DevState s1, const Ctl* __restrict__ ctl,
                                                    const Rec* __restrict__ send, uint64_t nsend, uint64_t gbase, LocalMaps lm,
                                                    const MapPayHdr* __restrict__ hdr, const uint32_t* __restrict__ off,
                                                    MapPayPage* __restrict__ pay)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    const DevState st = ctl->base ? s1 : s0;
    for (uint64_t j = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); j < nsend; j += nw) {
        if (hdr[j].share & 1u) continue;                 // the previous record carries the map
        const uint64_t i = (send[j].src >> 8) - gbase;
        const uint32_t X = st.sid[i];
        const uint32_t* row = lm.slot + (uint64_t)X * lm.S;
        const uint32_t W = lm.wx * lm.wy, toff = lm.S - 4u * lm.V;
        uint64_t q = off[j];
        const uint32_t hw = lm_hw_word(row[toff - 1u]);
        for (uint32_t s = 0; s < W + hw; ++s) {          // k_pay_hdr's walk: npg pages
            const bool tr = s >= W;
            const uint32_t p = tr ? row[toff + 4u * (s - W) + 2u] : row[s];
            if (p == DM_LM_NONE) continue;
            if (lane == 0) {
                pay[q].slot = tr ? (kPayTrail | (s - W)) : s;
                pay[q].a = tr ? (int32_t)row[toff + 4u * (s - W)] : 0;
                pay[q].b = tr ? (int32_t)row[toff + 4u * (s - W) + 1u] : 0;
                pay[q].pad = 0;
            }
            pay[q].cell[lane] = lm.page[(uint64_t)p * DM_LM_PAGE_CELLS + lane];
            ++q;
        }
    }
}

// exclusive prefix of the headers' page counts (one block; out: m + 1 words)
__global__ void __launch_bounds__(1024) k_pay_prefix(const MapPayHdr* __restrict__ hdr, uint64_t m, uint32_t* __restrict__ out)
{
    __shared__ uint32_t s_sum[1024];
    const uint64_t per = (m + 1023) / 1024;
    const uint64_t lo = threadIdx.x * per, hi = lo + per < m ? lo + per : m;
    uint32_t t = 0;
    for (uint64_t i = lo; i < hi; ++i) t += hdr[i].npg;
    s_sum[threadIdx.x] = t;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t v = threadIdx.x >= (uint32_t)o ? s_sum[threadIdx.x - o] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = s_sum[threadIdx.x] - t;
    for (uint64_t i = lo; i < hi; ++i) {
        out[i] = run;
        run += hdr[i].npg;
    }
    if (threadIdx.x == 1023) out[m] = s_sum[1023];
}

// the received records' map owners: head[r] = the last record at or before r that carries a
// map (the copies of one source that came together share it); one block, ranges per thread
__global__ void __launch_bounds__(1024) k_recv_heads(const MapPayHdr* __restrict__ hdr, uint64_t m, uint32_t* __restrict__ head)
{
    __shared__ uint32_t s_h[1024];
    const uint64_t per = (m + 1023) / 1024;
    const uint64_t lo = threadIdx.x * per, hi = lo + per < m ? lo + per : m;
    uint32_t h = 0;                                      // 1 + the last head of the range (0: none)
    for (uint64_t i = lo; i < hi; ++i)
        if (!(hdr[i].share & 1u)) h = (uint32_t)i + 1u;
    s_h[threadIdx.x] = h;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                 // inclusive max-scan over the threads
        const uint32_t v = threadIdx.x >= (uint32_t)o ? s_h[threadIdx.x - o] : 0u;
        __syncthreads();
        s_h[threadIdx.x] = max(s_h[threadIdx.x], v);
        __syncthreads();
    }
    uint32_t run = threadIdx.x ? s_h[threadIdx.x - 1] : 0u;
    for (uint64_t i = lo; i < hi; ++i) {
        if (!(hdr[i].share & 1u)) run = (uint32_t)i + 1u;
        head[i] = run ? run - 1u : 0u;                   // record 0 always carries its map
    }
}

// the received records' maps: a record r that carries one takes free table frees[r] and its
// pages at hoff[r] past the free list's cursor, filled from the payload; the records sharing it
// (and every output of them) name that table, which their next map update then finds shared --
// copy on write, as the copies of a one-GPU resample.  One wave per record: its lanes copy
// each page's cells, then write the table's row (window slots, then the trail's entries
// {a, b, page, -})
__global__ void __launch_bounds__(kLmBlock) k_recv_maps(uint64_t nrec, const uint32_t* __restrict__ frees, Ctl* __restrict__ ctl,
                                                        const MapPayHdr* __restrict__ hdr, const uint32_t* __restrict__ hoff,
                                                        const MapPayPage* __restrict__ pay, LocalMaps lm)
{
    if (ctl->err & kFaultPages) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * (kLmBlock / 64);
    const uint32_t toff = lm.S - 4u * lm.V;
    for (uint64_t r = (uint64_t)blockIdx.x * (kLmBlock / 64) + (threadIdx.x >> 6); r < nrec; r += nw) {
        if (hdr[r].share & 1u) continue;
        const uint64_t alloc = ctl->pg_cursor + hoff[r];
        const uint32_t T = frees[r];
        const uint64_t gT = ((uint64_t)lm.tgen[T] << 32) | T;
        const uint32_t npg = hdr[r].npg;
        const uint64_t q0 = hoff[r];
        for (uint32_t q = 0; q < npg; ++q) {
            const uint32_t np = lm.frees[alloc + q];
            lm.page[(uint64_t)np * DM_LM_PAGE_CELLS + lane] = pay[q0 + q].cell[lane];
            if (lane == 0) lm.owner[np] = gT;
        }
        uint32_t* tsl = lm.slot + (uint64_t)T * lm.S;
        for (uint32_t s = lane; s < lm.S; s += 64u) {
            uint32_t v = DM_LM_NONE;
            if (s == toff - 2u) {                        // the map's copies of shared-grid cells
                v = (hdr[r].share & 2u) ? kLmShadow : DM_LM_NONE;
            } else if (s == toff - 1u) {                 // the trail's high-water mark
                for (uint32_t q = 0; q < npg; ++q) {
                    const uint32_t sl = pay[q0 + q].slot;
                    if (sl & kPayTrail) v = (v == DM_LM_NONE || (sl & ~kPayTrail) + 1u > v) ? (sl & ~kPayTrail) + 1u : v;
                }
            } else if (s < toff) {
                for (uint32_t q = 0; q < npg; ++q) v = pay[q0 + q].slot == s ? lm.frees[alloc + q] : v;
            } else {
                const uint32_t e = (s - toff) >> 2, k = (s - toff) & 3u;
                for (uint32_t q = 0; q < npg; ++q) {
                    const MapPayPage& pp = pay[q0 + q];
                    if (pp.slot != (kPayTrail | e)) continue;
                    v = k == 0u ? (uint32_t)pp.a : k == 1u ? (uint32_t)pp.b : k == 2u ? lm.frees[alloc + q] : DM_LM_NONE;
                }
            }
            tsl[s] = v;
        }
        if (lane == 0) lm.ctr[T] = hdr[r].ctr;
    }
}

// the particles a sharded resample received from record r (sid = kSidRecord | r) name the
// table of the record carrying r's map, frees[head[r]]
__global__ void __launch_bounds__(kBlock) k_recv_rename(const uint32_t* __restrict__ dups, const uint32_t* __restrict__ frees,
                                                        const uint32_t* __restrict__ head, const uint32_t* __restrict__ ndup_dev,
                                                        SidRef sr)
{
    uint32_t* sid = cur_sid(sr);
    const uint64_t ndup = *ndup_dev;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < ndup; j += (uint64_t)gridDim.x * kBlock)
        sid[dups[j]] = frees[head[sid[dups[j]] & ~kSidRecord]];
}

// the particles a sharded resample received (cs.dups, *cs.ndup, from nrecv records) get their
// records' maps: a free table and pages from the pool per record, filled from the payloads
// (needs eslam_launch_store_refs first): hdr / pay the received headers and pages, hoff
// (nrecv + 1 words) scratch
extern "C" hipError_t eslam_launch_store_receive(SidRef sid, Ctl* ctl, const LocalMaps* lm, const MergeParams* mp, uint64_t n,
                                                 const CowScratch* cs, const void* hdr, uint64_t nrecv, uint32_t* hoff,
                                                 uint32_t* head, const void* pay, uint32_t* pgc, hipStream_t stream)
{
    if (!n) return hipSuccess;
    hipError_t e = compact(1, n, cs->ref, sid, cs->counts + cs->tiles + 1, cs->dups, cs->ndup, stream);
    if (e != hipSuccess) return e;
    const MapPayHdr* h = (const MapPayHdr*)hdr;
    if (nrecv) {
        hipLaunchKernelGGL(k_pay_prefix, dim3(1), dim3(1024), 0, stream, h, nrecv, hoff);
        hipLaunchKernelGGL(k_recv_heads, dim3(1), dim3(1024), 0, stream, h, nrecv, head);
    } else {
        e = hipMemsetAsync(hoff, 0, 4, stream);
        if (e != hipSuccess) return e;
    }
    // the plan is the records' page counts: one "block" whose sum is hoff[nrecv]
    e = hipMemcpyAsync(mp->poff, hoff + nrecv, 4, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(mp->poff + 1, 0, 4, stream);
    if (e != hipSuccess) return e;
    e = page_budget(ctl, lm, mp, 1u, pgc, stream);
    if (e != hipSuccess) return e;
    const uint64_t gw = (nrecv + kLmBlock / 64 - 1) / (kLmBlock / 64);
    if (nrecv)
        hipLaunchKernelGGL(k_recv_maps, dim3((uint32_t)(gw < 8192 ? gw : 8192)), dim3(kLmBlock), 0, stream, nrecv, cs->frees, ctl, h,
                           hoff, (const MapPayPage*)pay, *lm);
    hipLaunchKernelGGL(k_pg_advance, dim3(1), dim3(1), 0, stream, ctl);
    const uint64_t want_r = (n + kBlock - 1) / kBlock;
    const uint32_t gr = (uint32_t)(want_r < 2048 ? want_r : 2048);
    hipLaunchKernelGGL(k_recv_rename, dim3(gr), dim3(kBlock), 0, stream, cs->dups, cs->frees, head, cs->ndup, sid);
    return hipGetLastError();
}

// a sharded resample's map payloads (after k_pack): headers, their prefix (off: nsend + 1
// words; the host reads the per-destination page counts from it), then the pages
extern "C" hipError_t eslam_launch_pay_hdr(DevState s0, DevState s1, const Ctl* ctl, const void* send, uint64_t nsend,
                                           uint64_t gbase, const LocalMaps* lm, const PaySeg* seg, void* hdr, uint32_t* off,
                                           hipStream_t stream)
{
    if (!nsend) return hipMemsetAsync(off, 0, 4, stream);
    const uint64_t g = (nsend + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(k_pay_hdr, dim3((uint32_t)(g < 4096 ? g : 4096)), dim3(kBlock), 0, stream, s0, s1, ctl, (const Rec*)send,
                       nsend, gbase, *lm, *seg, (MapPayHdr*)hdr);
    hipLaunchKernelGGL(k_pay_prefix, dim3(1), dim3(1024), 0, stream, (const MapPayHdr*)hdr, nsend, off);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_pay_pack(DevState s0, DevState s1, const Ctl* ctl, const void* send, uint64_t nsend,
                                            uint64_t gbase, const LocalMaps* lm, const void* hdr, const uint32_t* off, void* pay,
                                            hipStream_t stream)
{
    if (!nsend) return hipSuccess;
    const uint64_t g = (nsend + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(k_pay_pack, dim3((uint32_t)(g < 4096 ? g : 4096)), dim3(kBlock), 0, stream, s0, s1, ctl, (const Rec*)send,
                       nsend, gbase, *lm, (const MapPayHdr*)hdr, off, (MapPayPage*)pay);
    return hipGetLastError();
}

#ifdef ESLAM_STAMPS
int eslam_dev::stamps_mg_clear() { return stamps_clear(g_stamps_mg) | stamps_clear(g_stamps_mg_grid); }
int64_t eslam_dev::stamps_mg_read(uint64_t* out, uint64_t blocks) { return stamps_read(g_stamps_mg, g_stamps_mg_grid, out, blocks * kStampSlots * 8); }
#endif
