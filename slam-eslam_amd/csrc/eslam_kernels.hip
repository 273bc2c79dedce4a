// eslam_kernels.hip -- gfx950 kernels of the eSLAM per-step particle-filter update.
//
// One update of the reference (EmbodiedSlamFilter::update -> PoseEstimator::project +
// PoseEstimator::update, src/EmbodiedSlamFilter.cpp:353-369) runs as four launches with no
// host round trip:
//
//   k_project_weight  predict (src/PoseEstimator.cpp:196-237) fused with updateWeights
//                     phase A (src/PoseEstimator.cpp:276-327: ContactModel::evaluatePose,
//                     evaluateWeight, updateZPositionEstimate + the MLS lookup of
//                     GridAccess::get) and the exact per-bucket statistics
//   k_finalize        one block: floating weight, phase-B factors, normalisation sum,
//                     effective count and the resample decision (src/PoseEstimator.cpp:329,
//                     src/ParticleFilter.hpp:46-70, src/PoseEstimator.cpp:250)
//   k_normalize_scan  phase B + normalisation (src/PoseEstimator.cpp:332-345,
//                     src/ParticleFilter.hpp:46-70) and, when resampling, each tile's exact
//                     fixed-point weight total
//   k_segments        stratified resample (src/ParticleFilter.hpp:85-108): the tile prefix
//                     (sum of the preceding tile totals), a blocked fixed-point scan, the
//                     wave's draws in LDS, and the segment-start marks of every ancestor
//
// The resample gather (expand the marks by a max-scan, copy the ancestor's state) is fused
// into the next step's k_project_weight; k_resample_gather materialises a pending gather
// when the state is read (download, the standalone PoseEstimator API) before that.
//
// This file holds these kernels with what they share: the K1 family (scalar argument loads, the
// LDS map window, the contact model, the contact records) and the weight path (statistics,
// k_finalize, the draws, K3, the sharded scan, commit, init, best particle, centroid,
// k_scan_excl).  The per-particle maps are in eslam_particle_maps.hip, the device self-tests in
// eslam_selftest.hip, the lane and wave primitives in eslam_wave.h.
//
// Everything is wave64: 256-thread blocks, butterfly reductions over 64 lanes (eslam_wave.h),
// ballots as 64-bit masks.  All arithmetic goes through include/eslam_detmath.h and
// the file is compiled with -ffp-contract=off, so results equal the CPU oracle bit for bit.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <string.h>

#include "eslam_internal.h"
#include "eslam_launch.h"
#include "eslam_wave.h"
#include "eslam_stamps.h"

namespace eslam_dev {

#ifdef ESLAM_STAMPS
ESLAM_STAMP_ARRAY(g_stamps_k1);
__device__ uint64_t g_stamps_k1w[kStampBlocks * kWaves][kWaveStampSlots];
ESLAM_STAMP_ARRAY(g_stamps_k3);
#endif
#ifdef ESLAM_DRAW_STATS
__device__ uint32_t g_draw_waves[2];
#endif

// ---------------------------------------------------------------------------------------
// K1 kernel arguments by scalar load at the point of use.  K1 reads ~110 uniform values
// (contacts, sampler, map header, state pointers).  Loaded once at kernel entry they exceed
// the 102 SGPRs, and the compiler parks them in VGPR lanes and fetches them back with
// v_readlane (a VALU instruction) on every row.  A volatile asm load + wait cannot be
// hoisted, so each value occupies SGPRs only where it is used; the scalar cache serves the
// repeats.  Outputs are early-clobber: the loads are in flight while the address is live.
// Blocks that are used together are loaded as one group with one wait (below), and a field is
// fetched once per particle row: 9 waits per row of the bench instantiation instead of 22.
// ---------------------------------------------------------------------------------------
typedef uint32_t su2 __attribute__((ext_vector_type(2)));
typedef uint32_t su4 __attribute__((ext_vector_type(4)));
typedef uint32_t su8 __attribute__((ext_vector_type(8)));
typedef uint32_t su16 __attribute__((ext_vector_type(16)));

#define KOFF(f) ((uint32_t)offsetof(K1Args, f))

__device__ __forceinline__ uint64_t kseg() { return (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr(); }

__device__ __forceinline__ su2 kl2(uint32_t off)
{
    su2 r;
    asm volatile("s_load_dwordx2 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(kseg()), "s"(off));
    return r;
}
__device__ __forceinline__ su4 kl4(uint32_t off)
{
    su4 r;
    asm volatile("s_load_dwordx4 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(kseg()), "s"(off));
    return r;
}
__device__ __forceinline__ su8 kl8(uint32_t off)
{
    su8 r;
    asm volatile("s_load_dwordx8 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(kseg()), "s"(off));
    return r;
}
__device__ __forceinline__ su16 kl16(uint32_t off)
{
    su16 r;
    asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(kseg()), "s"(off));
    return r;
}
// Groups: the blocks of a group are requested together and waited for once, so a wave parks
// once per group and not once per block (scalar loads return out of order: the only wait there
// is is lgkmcnt(0)).  Requests and wait stand in one asm statement.  Split in two statements
// (request now, wait in front of the first use, the blocks passed through the wait as "+s"
// operands) the compiler is free to copy a block's registers between the two, before the
// data has arrived: it did (DESIGN.md 4, K1's waits).
#define ESLAM_KL_GROUP2(name, WA, WB) \
    __device__ __forceinline__ void name(su##WA& a, uint32_t off_a, su##WB& b, uint32_t off_b) \
    { \
        asm volatile("s_load_dwordx" #WA " %0, %2, %3\n\ts_load_dwordx" #WB " %1, %2, %4\n\ts_waitcnt lgkmcnt(0)" \
                     : "=&s"(a), "=&s"(b) : "s"(kseg()), "s"(off_a), "s"(off_b)); \
    }
#define ESLAM_KL_GROUP3(name, WA, WB, WC) \
    __device__ __forceinline__ void name(su##WA& a, uint32_t off_a, su##WB& b, uint32_t off_b, su##WC& c, uint32_t off_c) \
    { \
        asm volatile("s_load_dwordx" #WA " %0, %3, %4\n\ts_load_dwordx" #WB " %1, %3, %5\n\ts_load_dwordx" #WC \
                     " %2, %3, %6\n\ts_waitcnt lgkmcnt(0)" \
                     : "=&s"(a), "=&s"(b), "=&s"(c) : "s"(kseg()), "s"(off_a), "s"(off_b), "s"(off_c)); \
    }
ESLAM_KL_GROUP2(kl8_2, 8, 2)
ESLAM_KL_GROUP2(kl8_4, 8, 4)
ESLAM_KL_GROUP2(kl16_2, 16, 2)
ESLAM_KL_GROUP3(kl8_2_8, 8, 2, 8)
ESLAM_KL_GROUP3(kl8_2_16, 8, 2, 16)
ESLAM_KL_GROUP3(kl16_8_4, 16, 8, 4)
template <class V> __device__ __forceinline__ uint64_t kq(const V& r, int k)
{
    return (uint64_t)r[2 * k] | ((uint64_t)r[2 * k + 1] << 32);
}
template <class V> __device__ __forceinline__ double kd(const V& r, int k) { return dm_from_bits(kq(r, k)); }
// pointers from the kernel arguments are global memory: the explicit address space gives
// global_load/store (SGPR base + 32-bit offset, vmcnt only) instead of flat accesses
template <class T> using gmem = __attribute__((address_space(1))) T;
template <class T, class V> __device__ __forceinline__ gmem<T>* kp(const V& r, int k) { return (gmem<T>*)(uintptr_t)kq(r, k); }

// the state pointers of buffer s[b] (offset KOFF(s[b]))
struct StatePtrs {
    gmem<double> *x, *y, *th, *z, *zs, *w, *mprob;
    gmem<uint8_t>* flags;
};
__device__ __forceinline__ StatePtrs state_ptrs(const su16& r)
{
    return StatePtrs{kp<double>(r, 0), kp<double>(r, 1), kp<double>(r, 2), kp<double>(r, 3),
                     kp<double>(r, 4), kp<double>(r, 5), kp<double>(r, 6), kp<uint8_t>(r, 7)};
}
__device__ __forceinline__ StatePtrs kstate(uint32_t off) { return state_ptrs(kl16(off)); }

static_assert(offsetof(StepParams, mu) == 24 && offsetof(StepParams, L22) == 88 && offsetof(StepParams, z_delta) == 120 &&
                  offsetof(StepParams, me2) == 136 && offsetof(StepParams, use_shape) == 168,
              "K1 scalar-load blocks");
static_assert(offsetof(MapView, width) == 48 && offsetof(MapView, height) == 64, "map lookup header");
static_assert(offsetof(ContactC, pz) == 32 && offsetof(GatherView, record) == 32, "K1 scalar-load blocks");
static_assert(offsetof(LocalMaps, S) == 24 && offsetof(LocalMaps, hy) == 40 && offsetof(LocalMaps, mx) == 48 &&
                  offsetof(LocalMaps, my) == 56, "K1 reads the local maps' first 64 bytes");

// ---------------------------------------------------------------------------------------
// GridAccess::get -> MLSMap::getPatch(C_global2local * p, patch, 3.0)  (src/PoseEstimator.hpp:97-105)
// qv: the query patch variance (measVar).  Cell: floor((x - offset) * (1/scale)); the
// 3-sigma gate |mean_p - z| < 3 sqrt(stdev_p^2 + measVar) is evaluated squared.
// The window part of the grid under the particle cloud may be staged in LDS: identical
// values, so the result never depends on whether a cell came from LDS or global memory.
// ---------------------------------------------------------------------------------------
// One window cell in LDS: its first patch inline + its patch range in global memory, so a
// lookup is one 16-byte LDS read (further patches of multi-patch cells come from global).
struct alignas(16) WinCell {
    float mean0, stdev0;
    uint32_t begin, count;
};

// The window's bounds stay in LDS (k1_win) and are re-read where used: held in registers
// across the particle loop they would be 6 more long-lived SGPRs, which K1 cannot afford.
__shared__ __attribute__((aligned(16))) int k1_win[8];   // on, m0, m1, n0, n1, cols

struct Window {
    int on;                              // staged (block-uniform)
    const WinCell* cells;                // rows x cols (LDS)
};

struct WinBounds {
    int on, m0, m1, n0, n1, cols;        // cell range [m0,m1) x [n0,n1)
};
__device__ __forceinline__ WinBounds win_bounds()
{
    typedef int vi4 __attribute__((ext_vector_type(4)));
    typedef int vi2 __attribute__((ext_vector_type(2)));
    // volatile keeps the reads where they are used; the explicit LDS address space keeps
    // them ds_read (a volatile generic pointer became a flat load + vmcnt(0) wait)
    typedef const volatile __attribute__((address_space(3))) vi4 lds_vi4;
    typedef const volatile __attribute__((address_space(3))) vi2 lds_vi2;
    const vi4 a = *(lds_vi4*)(&k1_win[0]);
    const vi2 b = *(lds_vi2*)(&k1_win[4]);
    return WinBounds{a.x, a.y, a.z, a.w, b.x, b.y};
}

__device__ __forceinline__ bool patch_gate(const gmem<const float>* height, uint32_t k, float pmf, float psf, double lz, double qv,
                                           double& mean, double& stdev)
{
    const double pm = (double)pmf, ps = (double)psf;
    const double ph = height ? (double)height[k] : 0.0;
    double diff;
    if (ph > 0.0) {
        if (lz > pm) diff = lz - pm;
        else if (lz < pm - ph) diff = (pm - ph) - lz;
        else diff = 0.0;
    } else {
        diff = dm_fabs(pm - lz);
    }
    if (diff * diff < 9.0 * (ps * ps + qv)) { mean = pm; stdev = ps; return true; }
    return false;
}

// per-particle maps: the patch of cell (m, n), which the shared grid leaves empty, from the
// particle's table (K1Args::store) with the same 3-sigma gate as a grid patch:
// the table's centre and the tile's slot load together, then the page cell.  A tile outside
// the window comes from the table's trail (rare: the window follows the particle).
__device__ __forceinline__ bool store_patch(uint32_t sid, uint32_t m, uint32_t n, double lz, double qv, double& mean,
                                            double& stdev)
{
    const su16 h = kl16(KOFF(store));                // 64 bytes: ctr, slot, page, {S, wx}, {wy, hx}, {hy, V}, mx, my
    const uint64_t w3 = kq(h, 3), w4 = kq(h, 4), w5 = kq(h, 5);
    const uint32_t S = (uint32_t)w3, wx = (uint32_t)(w3 >> 32), wy = (uint32_t)w4, hx = (uint32_t)(w4 >> 32);
    const uint32_t hy = (uint32_t)w5, V = (uint32_t)(w5 >> 32);
    const uint32_t a = m >> DM_LM_TILE_BITS, b = n >> DM_LM_TILE_BITS;
    const uint32_t qa = (uint32_t)(((uint64_t)a * kq(h, 6)) >> kLmMagicShift);
    const uint32_t qb = (uint32_t)(((uint64_t)b * kq(h, 7)) >> kLmMagicShift);
    const uint32_t s = (a - wx * qa) + wx * (b - wy * qb);
    const uint64_t c = kp<const uint64_t>(h, 0)[sid];   // int2 {x, y}
    const gmem<const uint32_t>* row = kp<const uint32_t>(h, 1) + (uint64_t)sid * S;
    uint32_t pg = row[s];
    if (!dm_lm_inside(a, (int32_t)(uint32_t)c, hx, wx) || !dm_lm_inside(b, (int32_t)(uint32_t)(c >> 32), hy, wy)) {
        pg = DM_LM_NONE;
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        const gmem<const u4>* t = reinterpret_cast<const gmem<const u4>*>(row + (S - 4u * V));
        const uint32_t hwv = row[S - 4u * V - 1u], hw = hwv == DM_LM_NONE ? 0u : hwv;
        for (uint32_t e = 0; e < hw; ++e) {
            const u4 v = t[e];
            if (v.z != DM_LM_NONE && v.x == a && v.y == b) pg = v.z;
        }
    }
    if (pg == DM_LM_NONE) return false;
    const uint64_t pf = reinterpret_cast<const gmem<const uint64_t>*>(kp<const float2>(h, 2))
        [(uint64_t)pg * DM_LM_PAGE_CELLS + (m & 7u) + 8u * (n & 7u)];
    const float sd = __uint_as_float((uint32_t)(pf >> 32));
    if (!dm_lm_holds(sd)) return false;
    return patch_gate(nullptr, 0, __uint_as_float((uint32_t)pf), sd, lz, qv, mean, stdev);
}

// store_patch for up to N feet of one particle at once (the cells get_patch<DELTA, true>
// deferred: dm[i] = ~0 for the others): the table's centre and every foot's slot in one round
// trip, then every page cell in one; the same results as store_patch foot by foot.  A tile
// outside the window (rare) takes store_patch itself.
constexpr uint32_t kStoreTrail = 0xfffffffeu;      // store_patches: a tile outside the window
template <int N>
__device__ __forceinline__ void store_patches(uint32_t sid, const uint32_t (&dm)[N], const uint32_t (&dn)[N],
                                              const double (&lz)[N], double qv, bool (&fnd)[N], double (&mean)[N],
                                              double (&stdev)[N])
{
    const su16 h = kl16(KOFF(store));
    const uint64_t w3 = kq(h, 3), w4 = kq(h, 4), w5 = kq(h, 5);
    const uint32_t S = (uint32_t)w3, wx = (uint32_t)(w3 >> 32), wy = (uint32_t)w4, hx = (uint32_t)(w4 >> 32);
    const uint32_t hy = (uint32_t)w5;
    const gmem<const uint32_t>* row = kp<const uint32_t>(h, 1) + (uint64_t)sid * S;
    bool any = false;
#pragma unroll
    for (int i = 0; i < N; ++i) any |= dm[i] != 0xffffffffu;
    if (!any) return;
    const uint64_t c = kp<const uint64_t>(h, 0)[sid];   // int2 {x, y}
    uint32_t pg[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        pg[i] = DM_LM_NONE;
        if (dm[i] == 0xffffffffu) continue;
        const uint32_t a = dm[i] >> DM_LM_TILE_BITS, b = dn[i] >> DM_LM_TILE_BITS;
        const uint32_t qa = (uint32_t)(((uint64_t)a * kq(h, 6)) >> kLmMagicShift);
        const uint32_t qb = (uint32_t)(((uint64_t)b * kq(h, 7)) >> kLmMagicShift);
        pg[i] = row[(a - wx * qa) + wx * (b - wy * qb)];
    }
    uint64_t pf[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        pf[i] = 0;
        if (dm[i] == 0xffffffffu) continue;
        const uint32_t a = dm[i] >> DM_LM_TILE_BITS, b = dn[i] >> DM_LM_TILE_BITS;
        if (!dm_lm_inside(a, (int32_t)(uint32_t)c, hx, wx) || !dm_lm_inside(b, (int32_t)(uint32_t)(c >> 32), hy, wy)) {
            pg[i] = kStoreTrail;                         // the trail: store_patch below
        } else if (pg[i] != DM_LM_NONE) {
            pf[i] = reinterpret_cast<const gmem<const uint64_t>*>(kp<const float2>(h, 2))
                [(uint64_t)pg[i] * DM_LM_PAGE_CELLS + (dm[i] & 7u) + 8u * (dn[i] & 7u)];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (dm[i] == 0xffffffffu) continue;
        if (pg[i] == kStoreTrail) {
            fnd[i] = store_patch(sid, dm[i], dn[i], lz[i], qv, mean[i], stdev[i]);
        } else if (pg[i] != DM_LM_NONE) {
            const float sd = __uint_as_float((uint32_t)(pf[i] >> 32));
            fnd[i] = dm_lm_holds(sd) && patch_gate(nullptr, 0, __uint_as_float((uint32_t)pf[i]), sd, lz[i], qv, mean[i], stdev[i]);
        }
    }
}

// a particle's table name for get_patch<DELTA>, with bit 31 set when its map holds copies of
// shared-grid cells (kLmShadow in its row): its lookups then ask its own cells first
__device__ __forceinline__ uint32_t store_sid(uint32_t sid)
{
    const su16 h = kl16(KOFF(store));
    const uint64_t w3 = kq(h, 3), w5 = kq(h, 5);
    const uint32_t S = (uint32_t)w3, V = (uint32_t)(w5 >> 32);
    const uint32_t f = kp<const uint32_t>(h, 1)[(uint64_t)sid * S + (S - 4u * V - 2u)];
    return sid | (f == kLmShadow ? 0x80000000u : 0u);
}

// the map is K1Args::map, read by scalar loads (header: 64 bytes per lookup).  DELTA: the
// particle's own map answers for cells the shared grid leaves empty, and first for every cell
// when it holds copies of shared-grid cells (sid bit 31, store_sid).
// DEFER (DELTA, a particle without copies of grid cells): a lookup that needs the particle's
// own map does not make it but returns false with *dm, *dn = its cell (else *dm = ~0), so the
// caller makes the lookups of all its feet together (store_patches)
template <bool DELTA = false, bool DEFER = false>
__device__ __forceinline__ bool get_patch(const Window& win, double px, double py, double pz, double qv, double& mean,
                                          double& stdev, uint32_t sid = 0, uint32_t* dm = nullptr, uint32_t* dn = nullptr,
                                          double* dlz = nullptr, const su16* hin = nullptr)
{
    if constexpr (DEFER) *dm = 0xffffffffu;
    // hin: the lookup header (the first 64 bytes of MapView) where the caller has it already
    const su16 h = hin ? *hin : kl16(KOFF(map));
    const uint32_t width = h[12], hcells = h[13], ident = h[14], has_height = h[15];
    double lx = px, ly = py, lz = pz;    // an identity global2local is applied as the identity
    if (!ident) {
        const su16 a = kl16(KOFF(map.g2l));
        const su8 b = kl8(KOFF(map.g2l[8]));
        lx = ((kd(a, 0) * px + kd(a, 1) * py) + kd(a, 2) * pz) + kd(a, 3);
        ly = ((kd(a, 4) * px + kd(a, 5) * py) + kd(a, 6) * pz) + kd(a, 7);
        lz = ((kd(b, 0) * px + kd(b, 1) * py) + kd(b, 2) * pz) + kd(b, 3);
    }
    const double ux = (lx - kd(h, 4)) * kd(h, 2);
    const double uy = (ly - kd(h, 5)) * kd(h, 3);
    if constexpr (DELTA) {
        if (sid >> 31) {                     // the particle's own cell first (the oracle's particle_map_fn)
            sid &= 0x7fffffffu;
            const double fm = floor(ux), fn = floor(uy);
            if ((fm >= 0.0) & (fm < (double)width) & (fn >= 0.0) & (fn < (double)hcells) &&
                store_patch(sid, (uint32_t)fm, (uint32_t)fn, lz, qv, mean, stdev))
                return true;
        }
    }
    // fast path without branches: an in-window cell whose first patch passes the gate (the
    // window is only staged for maps without heights).  Everything else -- off the window,
    // heights, a failing first patch of a multi-patch cell -- takes the loop below.  The
    // window lies inside the grid and starts at cell 1 in both directions, so the window test
    // needs no floor: v_cvt_i32_f64 truncates (saturating; NaN -> 0), which equals the floor
    // for every value >= 0, and maps every value < 1 -- negatives, NaN -- below the window.
    int im, in;                          // v_cvt_i32_f64 itself: defined for every input
    asm("v_cvt_i32_f64 %0, %1" : "=v"(im) : "v"(ux));
    asm("v_cvt_i32_f64 %0, %1" : "=v"(in) : "v"(uy));
    const WinBounds wb = win_bounds();
    const uint32_t wm = (uint32_t)im - (uint32_t)wb.m0, wn = (uint32_t)in - (uint32_t)wb.n0;
    const bool in_win = (wb.on != 0) & (wm < (uint32_t)wb.cols) & (wn < (uint32_t)(wb.n1 - wb.n0));
    const WinCell wc = win.cells[in_win ? wn * (uint32_t)wb.cols + wm : 0u];
    const double pm = (double)wc.mean0, ps = (double)wc.stdev0;
    const double diff = dm_fabs(pm - lz);
    const bool gate0 = in_win & (wc.count > 0) & (diff * diff < 9.0 * (ps * ps + qv));
    mean = pm;
    stdev = ps;
    if (gate0) return true;
    // the cell by the floor (outside the window trunc and floor differ)
    const double fm = floor(ux), fn = floor(uy);
    asm("v_cvt_i32_f64 %0, %1" : "=v"(im) : "v"(fm));
    asm("v_cvt_i32_f64 %0, %1" : "=v"(in) : "v"(fn));
    const bool in_grid = (fm >= 0.0) & (fm < (double)width) & (fn >= 0.0) & (fn < (double)hcells);
    if constexpr (DELTA) {
        if (!in_grid || (in_win && wc.count == 1)) return false;
        if (in_win && wc.count == 0) {
            if constexpr (DEFER) {
                *dm = (uint32_t)im;
                *dn = (uint32_t)in;
                *dlz = lz;
                return false;
            }
            return store_patch(sid, (uint32_t)im, (uint32_t)in, lz, qv, mean, stdev);
        }
    } else {
        if (!in_grid || (in_win && wc.count <= 1)) return false;
    }
    const gmem<const float>* height = has_height ? kp<const float>(kl2(KOFF(map.height)), 0) : nullptr;
    const gmem<const float2>* patch = kp<const float2>(h, 1);
    uint32_t b, e;
    if (in_win) {
        b = wc.begin + 1;
        e = wc.begin + wc.count;
    } else {
        // the cell's record (MapView::cell_tab): its range and first patch in one load
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        const gmem<const u4>* tab = kp<const u4>(kl2(KOFF(map.cell_tab)), 0);
        const uint64_t cell = (uint64_t)in * width + (uint64_t)im;
        const u4 ct = tab[cell];
        b = ct.z;
        e = ct.z + ct.w;
        if constexpr (DELTA) {
            if (b == e) {
                if constexpr (DEFER) {
                    *dm = (uint32_t)im;
                    *dn = (uint32_t)in;
                    *dlz = lz;
                    return false;
                }
                return store_patch(sid, (uint32_t)im, (uint32_t)in, lz, qv, mean, stdev);
            }
        }
        if (!has_height && b < e) {
            if (patch_gate(nullptr, 0, __uint_as_float(ct.x), __uint_as_float(ct.y), lz, qv, mean, stdev)) return true;
            ++b;
        }
    }
    for (uint32_t k = b; k < e; ++k) {
        const uint64_t pf = reinterpret_cast<const gmem<const uint64_t>*>(patch)[k];   // float2 {mean, stdev}
        if (patch_gate(height, k, __uint_as_float((uint32_t)pf), __uint_as_float((uint32_t)(pf >> 32)), lz, qv, mean,
                       stdev))
            return true;
    }
    return false;
}

__device__ __forceinline__ uint64_t order_key(double w)
{
    const uint64_t b = dm_bits(w);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double key_value(uint64_t k)
{
    return dm_from_bits((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

// Stage the grid cells under last step's particle cloud (+ margin) into LDS.  Every block
// computes the same window from ctl; a window that does not fit is simply not used.
__device__ Window stage_window(const MapView& m, const StepParams& p, const Ctl* ctl, double extra_margin,
                               unsigned char* lds)
{
    int* s_w = k1_win;
    Window w;
    w.on = 0;
    if (threadIdx.x == 0) {
        int on = 0;
        const uint64_t k0 = ctl->bbox[0], k1 = ctl->bbox[1], k2 = ctl->bbox[2], k3 = ctl->bbox[3];
        if (p.use_window && k0 && k1 && k2 && k3 && !m.height) {
            const double mg = p.win_margin + extra_margin;
            const double x0 = key_value(~k0) - mg, x1 = key_value(k1) + mg;
            const double y0 = key_value(~k2) - mg, y1 = key_value(k3) + mg;
            const double* A = m.g2l;
            double lx0 = 1e300, lx1 = -1e300, ly0 = 1e300, ly1 = -1e300;
            for (int c = 0; c < 4; ++c) {
                const double wx = (c & 1) ? x1 : x0, wy = (c & 2) ? y1 : y0;
                const double lx = (A[0] * wx + A[1] * wy) + A[3], ly = (A[4] * wx + A[5] * wy) + A[7];
                lx0 = lx < lx0 ? lx : lx0; lx1 = lx > lx1 ? lx : lx1;
                ly0 = ly < ly0 ? ly : ly0; ly1 = ly > ly1 ? ly : ly1;
            }
            const double fm0 = floor((lx0 - m.offset_x) * m.inv_scale_x) - 1.0;
            const double fm1 = floor((lx1 - m.offset_x) * m.inv_scale_x) + 2.0;
            const double fn0 = floor((ly0 - m.offset_y) * m.inv_scale_y) - 1.0;
            const double fn1 = floor((ly1 - m.offset_y) * m.inv_scale_y) + 2.0;
            if (dm_isfinite(fm0) && dm_isfinite(fm1) && dm_isfinite(fn0) && dm_isfinite(fn1)) {
                // the window starts at cell 1 (get_patch's floor-free window test); cells of
                // column / row 0 take the general path
                const double W = (double)m.width, H = (double)m.height_cells;
                const int m0 = (int)(fm0 < 1 ? 1 : (fm0 > W ? W : fm0));
                const int m1 = (int)(fm1 < 1 ? 1 : (fm1 > W ? W : fm1));
                const int n0 = (int)(fn0 < 1 ? 1 : (fn0 > H ? H : fn0));
                const int n1 = (int)(fn1 < 1 ? 1 : (fn1 > H ? H : fn1));
                const int rows = n1 - n0, cols = m1 - m0;
                if (rows > 0 && cols > 0 && (int64_t)rows * cols * (int64_t)sizeof(WinCell) <= kWindowLds) {
                    on = 1;
                    s_w[1] = m0; s_w[2] = m1; s_w[3] = n0; s_w[4] = n1; s_w[5] = cols;
                }
            }
        }
        s_w[0] = on;
    }
    __syncthreads();
    if (!s_w[0]) return w;
    const int wm0 = s_w[1], wn0 = s_w[3], wn1 = s_w[4], wcols = s_w[5];
    WinCell* cells = reinterpret_cast<WinCell*>(lds);
    const int ncell = (wn1 - wn0) * wcols;
    // one memory round trip per batch of kPer cells per thread: each cell's record in
    // MapView::cell_tab is already the WinCell (range + first patch)
    constexpr int kPer = 4;
    const uint4* tab = m.cell_tab;
    for (int t0 = 0; t0 < ncell; t0 += kPer * kBlock) {
        uint4 v[kPer];
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int t = t0 + (int)threadIdx.x + q * kBlock;
            v[q] = make_uint4(0u, 0u, 0u, 0u);
            if (t < ncell) {
                const int r = t / wcols, c = t - r * wcols;
                v[q] = tab[(uint64_t)(wn0 + r) * m.width + (uint64_t)(wm0 + c)];
            }
        }
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int t = t0 + (int)threadIdx.x + q * kBlock;
            if (t < ncell) {
                WinCell wc;
                wc.mean0 = __uint_as_float(v[q].x);
                wc.stdev0 = __uint_as_float(v[q].y);
                wc.begin = v[q].z;
                wc.count = v[q].w;
                cells[t] = wc;
            }
        }
    }
    __syncthreads();
    w.on = 1;
    w.cells = cells;
    return w;
}

// ---------------------------------------------------------------------------------------
// ContactModel::evaluatePose + evaluateWeight  (src/ContactModel.cpp:117-224, 262-317)
// ---------------------------------------------------------------------------------------
struct CMResult {
    uint32_t ncp;
    bool accepted;
    double weight, zdelta, zvar, posevar, s2;
};

// contactLikelihoodRatio(z, sigma) > 1e-9 guaranteed (exact-arithmetic bounds, wide margin),
// sigma^2 = zvar corr^2: a one-point group's ratio cancels ((zdiff*r)/r = zdiff) and is not
// evaluated (same predicate as the oracle)
__device__ __forceinline__ bool ratio_surely_significant(double z, double zvar, double corr)
{
    const double s2 = zvar * (corr * corr);
    if (z <= 0.0) return s2 < 1e16;
    return s2 < 1600.0 && z * z < 31.36 * s2;
}

// MAXP: bound on the contact points found (group ends); BATCH: p.m <= MAXP contacts;
// UNG (with BATCH): every contact closes its group (groupId -1 or a group of one), so the
// group logic reduces to the Q7 poisoning flag and a push per evaluated, found contact.
// StepParams (p.*) and the contacts come from scalar loads of the kernel arguments.
// lookups in flight per particle in the reduced group logic (BATCH && UNG): all MAXP by
// default; an experiment knob (fewer live registers)
#ifndef ESLAM_K1_LB
#define ESLAM_K1_LB 4
#endif
constexpr int kK1LookupBatch = ESLAM_K1_LB;

template <int MAXP, bool BATCH, bool DELTA = false, bool UNG = false>
__device__ __forceinline__ CMResult evaluate_pose(const Window& win, double co, double s, double r22, double x, double y,
                                                  double z, double meas_var, uint32_t sid, const su8& wp, const su4& wq)
{
    // wp: me2, radius, corr, min_contacts; wq: use_shape, m, eval_mask, end_mask (StepParams,
    // loaded by the caller once per particle row)
    CMResult r;
    // pushed contact points.  BATCH: slot = index of the contact that closed the group, so
    // every write has a static index; the slots are summed in index order = push order.
    double cz[MAXP], cv[MAXP];
    bool ok[MAXP];
#pragma unroll
    for (int k = 0; k < MAXP; ++k) ok[k] = false;
    uint32_t ncp = 0;
    bool valid = false, group_valid = true;
    double contact_ratio = 0, pose_var_avg = 0, posevar = 0;
    double pzd = 0, pzv = 0;
    const double qv = meas_var;
    const double radius = kd(wp, 1), corr = kd(wp, 2);
    const uint32_t m = wq[1], eval_mask = wq[2], end_mask = wq[3];

    auto push = [&](uint32_t i, double zd, double zv) {
        if constexpr (BATCH) {
            cz[i] = zd; cv[i] = zv; ok[i] = true;
        } else {
#pragma unroll
            for (int k = 0; k < MAXP; ++k)
                if ((uint32_t)k == ncp) { cz[k] = zd; cv[k] = zv; }
        }
        ++ncp;
    };
    // the sequential part of one contact (group logic, Q7 poisoning): found/mean/stdev are
    // the map lookup of its world point (used only when the contact is evaluated)
    auto contact = [&](uint32_t i, bool found, double mean, double stdev, double wz) {
        const bool c_eval = (eval_mask >> i) & 1u, c_end = (end_mask >> i) & 1u;
        if (group_valid && c_eval) {
            if (found) {
                const double zdiff = wz - mean;
                const double pose_var = stdev * stdev;
                const double zvar = stdev * stdev + meas_var;
                if (!valid && c_end && ratio_surely_significant(zdiff, zvar, corr)) {
                    // single-point group: (zdiff, zvar) pushed directly
                    posevar += pose_var;
                    push(i, zdiff, zvar);
                    group_valid = true;
                    valid = false;
                    pose_var_avg = 0;
                    contact_ratio = 0;
                    return;
                }
                const double ratio = dm_normal_pdf_cdf_ratio(zdiff, dm_sqrt(zvar) * corr);
                if (!valid) {
                    pzd = zdiff * ratio;
                    pzv = zvar * ratio;
                    contact_ratio = ratio;
                    pose_var_avg = pose_var * ratio;
                } else {
                    pzd += zdiff * ratio;
                    pzv += zvar * ratio;
                    contact_ratio += ratio;
                    pose_var_avg += pose_var * ratio;
                }
                valid = true;
            } else {
                group_valid = false;
            }
        }
        if (valid && c_end) {
            if (group_valid && contact_ratio > 1e-9) {
                const double inv = 1.0 / contact_ratio;
                pzd *= inv;
                pzv *= inv;
                posevar += pose_var_avg * inv;
                push(i, pzd, pzv);
            }
            group_valid = true;
            valid = false;
            pose_var_avg = 0;
            contact_ratio = 0;
        }
    };
    // pose * p with pose = Translation(x, y, z) * AngleAxis(theta, UnitZ); the zero products
    // of the affine multiply are per-step constants, and "- 0.0" is exact
    // the contact and the map's lookup header (for the lookup that follows) in one group
    auto world = [&](uint32_t i, double& wx, double& wy, double& wz, su16& h) {
        su8 c;
        su2 cpz;
        const uint32_t off = KOFF(p.c) + i * (uint32_t)sizeof(ContactC);
        kl8_2_16(c, off, cpz, off + (uint32_t)offsetof(ContactC, pz), h, KOFF(map));   // px, py, zp, zz | pz | header
        const double px = kd(c, 0), py = kd(c, 1), zp = kd(c, 2), zz = kd(c, 3), pz = kd(cpz, 0);
        wx = ((co * px + (-s) * py) + zp) + x;
        wy = ((s * px + co * py) + zp) + y;
        wz = ((zz + r22 * pz) + z) - radius;
    };
    auto lookup = [&](const su16& h, double wx, double wy, double wz, double& mean, double& stdev) -> bool {
        return get_patch<DELTA>(win, wx, wy, wz, qv, mean, stdev, sid, nullptr, nullptr, nullptr, &h);
    };

    if constexpr (BATCH && UNG && kK1LookupBatch < MAXP) {
        // the reduced group logic (below) with kK1LookupBatch lookups in flight at a time
        bool alive = true;
#pragma unroll
        for (int g = 0; g < MAXP; g += kK1LookupBatch) {
            bool fnd[kK1LookupBatch];
            double mn[kK1LookupBatch], sd[kK1LookupBatch], wzs[kK1LookupBatch];
#pragma unroll
            for (int q = 0; q < kK1LookupBatch; ++q) {
                const int i = g + q;
                fnd[q] = false; mn[q] = 0.0; sd[q] = 0.0; wzs[q] = 0.0;
                if ((uint32_t)i < m) {
                    double wx, wy;
                    su16 h;
                    world((uint32_t)i, wx, wy, wzs[q], h);
                    if ((eval_mask >> i) & 1u) fnd[q] = lookup(h, wx, wy, wzs[q], mn[q], sd[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < kK1LookupBatch; ++q) {
                const int i = g + q;
                if ((uint32_t)i >= m) break;
                if (!((eval_mask >> i) & 1u)) continue;
                if (alive && fnd[q]) {
                    const double zdiff = wzs[q] - mn[q];
                    const double pose_var = sd[q] * sd[q];
                    const double zvar = sd[q] * sd[q] + meas_var;
                    double pzd_i = zdiff, pzv_i = zvar, pv_i = pose_var;
                    bool take = true;
                    if (!ratio_surely_significant(zdiff, zvar, corr)) {
                        const double ratio = dm_normal_pdf_cdf_ratio(zdiff, dm_sqrt(zvar) * corr);
                        take = ratio > 1e-9;
                        const double inv = 1.0 / ratio;
                        pzd_i = (zdiff * ratio) * inv;
                        pzv_i = (zvar * ratio) * inv;
                        pv_i = (pose_var * ratio) * inv;
                    }
                    if (take) {
                        posevar += pv_i;
                        push((uint32_t)i, pzd_i, pzv_i);
                    }
                }
                alive = alive && fnd[q];
            }
        }
    } else if constexpr (BATCH) {
        // all m <= MAXP contacts' lookups first: independent, so their memory latencies
        // overlap (a lookup the group logic then skips is harmless: pure function)
        bool fnd[MAXP];
        double mn[MAXP], sd[MAXP], wzs[MAXP];
        if constexpr (DELTA) {
            if (!(sid >> 31)) {
                // the feet the shared grid leaves to the particle's map: their lookups together
                uint32_t dm[MAXP], dn[MAXP];
                double dlz[MAXP];
#pragma unroll
                for (int i = 0; i < MAXP; ++i) {
                    fnd[i] = false; mn[i] = 0.0; sd[i] = 0.0; wzs[i] = 0.0; dm[i] = 0xffffffffu; dn[i] = 0u; dlz[i] = 0.0;
                    if ((uint32_t)i < m) {
                        double wx, wy;
                        su16 h;
                        world((uint32_t)i, wx, wy, wzs[i], h);
                        if ((eval_mask >> i) & 1u)
                            fnd[i] = get_patch<true, true>(win, wx, wy, wzs[i], qv, mn[i], sd[i], sid, &dm[i], &dn[i], &dlz[i], &h);
                    }
                }
                store_patches<MAXP>(sid, dm, dn, dlz, qv, fnd, mn, sd);
            } else {
#pragma unroll
                for (int i = 0; i < MAXP; ++i) {
                    fnd[i] = false; mn[i] = 0.0; sd[i] = 0.0; wzs[i] = 0.0;
                    if ((uint32_t)i < m) {
                        double wx, wy;
                        su16 h;
                        world((uint32_t)i, wx, wy, wzs[i], h);
                        if ((eval_mask >> i) & 1u) fnd[i] = lookup(h, wx, wy, wzs[i], mn[i], sd[i]);
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < MAXP; ++i) {
                fnd[i] = false; mn[i] = 0.0; sd[i] = 0.0; wzs[i] = 0.0;
                if ((uint32_t)i < m) {
                    double wx, wy;
                    su16 h;
                    world((uint32_t)i, wx, wy, wzs[i], h);
                    if ((eval_mask >> i) & 1u) fnd[i] = lookup(h, wx, wy, wzs[i], mn[i], sd[i]);
                }
            }
        }
        if constexpr (UNG) {
            // contact() with c_end set for every contact: `valid` is false at the start of
            // each one, a surely-significant point is pushed as it is, any other one through
            // its ratio (pzd = (zdiff r) (1/r), ...), and a miss clears group_valid for good
            // (Q7: it is only reset under `valid`, which a miss never sets)
            bool alive = true;
#pragma unroll
            for (int i = 0; i < MAXP; ++i) {
                if ((uint32_t)i >= m) break;
                if (!((eval_mask >> i) & 1u)) continue;
                if (alive && fnd[i]) {
                    const double zdiff = wzs[i] - mn[i];
                    const double pose_var = sd[i] * sd[i];
                    const double zvar = sd[i] * sd[i] + meas_var;
                    double pzd_i = zdiff, pzv_i = zvar, pv_i = pose_var;
                    bool take = true;
                    if (!ratio_surely_significant(zdiff, zvar, corr)) {
                        const double ratio = dm_normal_pdf_cdf_ratio(zdiff, dm_sqrt(zvar) * corr);
                        take = ratio > 1e-9;
                        const double inv = 1.0 / ratio;
                        pzd_i = (zdiff * ratio) * inv;
                        pzv_i = (zvar * ratio) * inv;
                        pv_i = (pose_var * ratio) * inv;
                    }
                    if (take) {
                        posevar += pv_i;
                        push((uint32_t)i, pzd_i, pzv_i);
                    }
                }
                alive = alive && fnd[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < MAXP; ++i) {
                if ((uint32_t)i >= m) break;
                contact((uint32_t)i, fnd[i], mn[i], sd[i], wzs[i]);
            }
        }
    } else {
        for (uint32_t i = 0; i < m; ++i) {
            double wx, wy, wz, mean = 0.0, stdev = 0.0;
            su16 h;
            world(i, wx, wy, wz, h);
            bool found = false;
            if (group_valid && ((eval_mask >> i) & 1u)) found = lookup(h, wx, wy, wz, mean, stdev);
            contact(i, found, mean, stdev, wz);
        }
    }
    r.ncp = ncp;
    r.posevar = posevar;
    r.accepted = (uint64_t)ncp >= kq(wp, 3);
    r.weight = r.zdelta = r.zvar = r.s2 = 0.0;
    if (r.accepted) {
        // every zvar lies in [meas_var, meas_var + 2^256] (a float stdev squared), and d2 in
        // [2^-301, 4 / meas_var]: for meas_var in [2^-400, 2^300] the reciprocals need none of
        // the division's scaling (dm_div_inrange: the same bits)
        double d1 = 0, d2 = 0, inv_d2;
        auto sums = [&](auto recip) {
#pragma unroll
            for (int k = 0; k < MAXP; ++k) {
                if (BATCH ? ok[k] : (uint32_t)k < ncp) {
                    cv[k] = recip(cv[k]);       // cv now holds 1/zvar
                    d1 += cz[k] * cv[k];
                    d2 += cv[k];
                }
            }
            inv_d2 = recip(d2);
        };
        if (meas_var >= 0x1p-400 && meas_var <= 0x1p300) sums([](double v) { return dm_div_inrange(1.0, v); });
        else sums([](double v) { return 1.0 / v; });
        const double delta = d1 * inv_d2;
        double s2 = 0.0;
#pragma unroll
        for (int k = 0; k < MAXP; ++k) {
            if (BATCH ? ok[k] : (uint32_t)k < ncp) {
                const double d = cz[k] - delta;
                s2 += (d * d) * cv[k];
            }
        }
        r.s2 = s2;
        const uint32_t use_shape = wq[0];
        const double pz = use_shape ? dm_exp(-0.5 * s2) : 1.0;
        r.weight = pz;
        r.zdelta = -delta;
        r.zvar = inv_d2;
    }
    return r;
}

// ---------------------------------------------------------------------------------------
// k_project_weight: PoseEstimator::project and/or updateWeights phase A, one particle per
// lane, one canonical chunk (64 lanes x J rows) per wave.
// ---------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------
// source of a pending-gather output: expand the segment marks (inclusive max-scan) and
// decode.  Returns the local particle index, or sets *rec for a migrated particle.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t decode_source(uint32_t v, uint32_t multi, const gmem<const Rec>* __restrict__ recs,
                                                  const gmem<const Rec>** rec)
{
    *rec = nullptr;
    if (multi) {
        if (v >= kMarkOwn && v < kMarkHigh) return v - kMarkOwn;
        *rec = recs + (v >= kMarkHigh ? v - kMarkHigh : v);
        return 0;
    }
    return v;
}

// The state written by K1 (and w by K3) is streamed: each value is read once, by the next
// kernel, from another XCD.  Non-temporal stores (nt) leave fewer lines for the kernel-end L2
// writeback (interleaved A/B on MI355X: 256k +3 %, 4M +0.7 %, 16M +1.6 % per step; plain
// stores and agent-coherent sc1 stores measured beside them).  Same values, same bits.
#define K1_ST(p, v) __builtin_nontemporal_store((v), (p))

// K1's waves paced by rows done.  A launch of one generation starts every wave
// of a SIMD together on the same J rows, and at equal priority the SIMD serves its oldest wave
// first: the waves finish one after the other and the SIMD runs its last rows with few waves
// to hide latency.  Each wave sets its priority from its own progress at the top of a row, so
// a wave that is behind outranks one that is ahead.  0: nothing is emitted; 1: four bands,
// level 3 - min(3, 4 j / J); 2: two bands, level 1 for j < J / 2; 3: the control, the bands of
// 1 reversed (measured once, never shipped).  j and J are scalars and s_setprio takes an
// immediate: a scalar switch, run only where the band changes.  J == 1 emits nothing.
#ifndef ESLAM_K1_PACE
#define ESLAM_K1_PACE 1
#endif
__device__ __forceinline__ uint32_t k1_pace_level(uint32_t j, uint32_t J)
{
    if (ESLAM_K1_PACE == 2) return j < (J >> 1) ? 1u : 0u;
    // min(3, 4 j / J) without the division: 4 j / J >= k  <=>  4 j >= k J
    const uint32_t band = (4u * j >= J ? 1u : 0u) + (4u * j >= 2u * J ? 1u : 0u) + (4u * j >= 3u * J ? 1u : 0u);
    return ESLAM_K1_PACE == 3 ? band : 3u - band;
}
__device__ __forceinline__ void k1_set_priority(uint32_t level)
{
    switch (level) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}

#ifndef ESLAM_K1D_WPE
#define ESLAM_K1D_WPE 3                  // K1 DELTA: three waves a SIMD hold the batched own-map lookups unspilled
#endif
#ifndef ESLAM_K1_WPE
#define ESLAM_K1_WPE 1                    // the compiler's own choice; 5 asks a diagnostic build to keep five waves a SIMD
#endif
template <bool PROJECT, bool WEIGHT, int MAXP, bool BATCH, bool DELTA = false, bool UNG = false>
__global__ void __launch_bounds__(kBlock) ESLAM_K1_ATTR __attribute__((amdgpu_waves_per_eu(DELTA ? ESLAM_K1D_WPE : ESLAM_K1_WPE))) k_project_weight(K1Args a)
{
    // Inside the particle loop every argument is read by a scalar load where it is used
    // (KOFF offsets into the K1Args kernel argument); "a." appears only outside the loop.
    ESLAM_STAMP(g_stamps_k1, 0);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    ESLAM_STAMP_WAVE(0);
    const uint64_t n = a.p.n;
    const uint32_t J = a.p.J;
    const uint64_t csz = 64ull * J;
    const uint64_t nchunks = (n + csz - 1) / csz;
    Ctl* ctl = a.ctl;
    if (ctl->err & kFaultTimeout) return;    // poisoned filter (a wait gave up): nothing is touched
    // a pending resample gather is fused here: read the ancestors from state[base],
    // write the updated particles to state[base ^ 1] (the latest buffer)
    const uint32_t gath = ctl->gather;
    const uint32_t cur = ctl->base ^ ctl->flip;
    if (WEIGHT && blockIdx.x == 0 && threadIdx.x == 0) ctl->k3_base = cur;
    const uint32_t st_off = __builtin_amdgcn_readfirstlane(cur ? KOFF(s[1]) : KOFF(s[0]));
    const uint32_t si_off = __builtin_amdgcn_readfirstlane(gath ? (ctl->base ? KOFF(s[1]) : KOFF(s[0])) : st_off);
    const int wexp = ctl->wexp;
    double spread = 0.0;
    bool do_spread = false;
    double tf = 0.0, rf = 0.0;
    if (PROJECT) {
        spread = dm_weighting_function(ctl->max_weight, 0.0, a.p.spread_threshold, 0.0);
        do_spread = spread > 0 && !a.p.hash_use;
        tf = a.p.spread_trans * spread;
        rf = a.p.spread_rot * spread;
    }

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Window win;
    win.on = 0;
    if (WEIGHT) win = stage_window(a.map, a.p, ctl, 6.0 * tf, smem + kStatsLds);
    // the Box-Muller tables in LDS, behind the staged window's cells where those leave the
    // room (kBmLds at the end of the launch's LDS; a launch without the weighting has no
    // window).  Their reads then count in lgkmcnt and never queue behind the state gather's
    // loads; a block whose window is larger reads the tables from global memory.
    unsigned char* bm_tab = smem + kStatsLds + (WEIGHT ? kWindowLds - kBmLds : 0);
    uint32_t bm_lds = 0;                     // block-uniform (a scalar)
    if (ESLAM_K1_BM_LDS && PROJECT) {
        static_assert(sizeof(dm_bm_log_tab) == 4096 && sizeof(dm_bm_sc_tab32) == 2048 && kBlock == 256, "one piece per thread");
        int room = 1;
        if (win.on) {
            const WinBounds wb = win_bounds();   // written by stage_window before its barrier
            room = (wb.n1 - wb.n0) * wb.cols * (int)sizeof(WinCell) <= kWindowLds - kBmLds;
        }
        bm_lds = (uint32_t)__builtin_amdgcn_readfirstlane(room);
        if (bm_lds) {
            reinterpret_cast<uint4*>(bm_tab)[threadIdx.x] = reinterpret_cast<const uint4*>(&dm_bm_log_tab[0][0])[threadIdx.x];
            reinterpret_cast<uint2*>(bm_tab + 4096)[threadIdx.x] = reinterpret_cast<const uint2*>(&dm_bm_sc_tab32[0][0])[threadIdx.x];
        }
        __syncthreads();
    }
    ESLAM_STAMP_K1(1);

    // order-free per-lane state, kept across chunks
    double maxm = 0.0;
    // data particles | total points << 16 per lane (nD <= J, nTP <= ESLAM_MAX_CONTACTS J);
    // werr: some particle of the wave hit a zero measurement variance (wave-uniform)
    uint32_t nDTP = 0, werr = 0, flag = 0;
    uint32_t touched = 0;                // bit b: the wave walked bucket b (wave-uniform)
    // -min x, max x, -min y, max y of the cloud, rounded to float (the window only needs a
    // box that holds the cloud; it is widened by the float rounding in bbox_keys)
    float bb[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    uint64_t limb = 0;                  // lane t < 52: column t & 3 of exact accumulator t >> 2
    const int sa = DM_FX_SCALE - wexp, sb = DM_FX_SCALE - 2 * wexp;

    // one canonical chunk (64 x J particles) per wave; its totals go to exact fixed point.
    // A sharded step may split the launch (ChunkSel): the chunks of the rank's own outputs
    // first, the chunks that need exchanged records after the exchange (exact sums: the
    // statistics do not depend on the order in which chunks are processed)
    uint64_t chunk = (uint64_t)blockIdx.x * kWaves + wave;
    bool active = chunk < nchunks;
    if (a.sel.mode == 1u) {
        active = chunk >= a.sel.cdev[0] && chunk < a.sel.cdev[1];
    } else if (a.sel.mode == 2u) {
        chunk = chunk < a.sel.c_lo ? chunk : a.sel.c_hi + (chunk - a.sel.c_lo);
        active = chunk < nchunks;
    }
    if (active) {
    const uint64_t lbase = chunk * csz;
    // the per-bucket sums A_b, B_b of the sum contract: the pair of the bucket the wave is in
    // (cur_b; usually the chunk's only one) in registers, the others parked per lane in the
    // chunk's slot of K1Args::bspill and reloaded when the wave returns to them.  Each lane's
    // sum of bucket b sees the same additions in the same order as with a register per bucket.
    constexpr uint32_t kNoBucket = 0xffu;
    double curA = 0.0, curB = 0.0;
    uint32_t cur_b = kNoBucket;
    // DELTA (per-particle maps): a wave's particles find different numbers of contact points
    // (cells only their stores hold), so its rows span several buckets and parking pairs in
    // bspill costs a store and a load per switch (K1 DELTA 0.45 -> 0.51 ms at 8M, r04h).  Its
    // kernel runs at four waves per SIMD anyway: every bucket's pair stays in registers.
    constexpr bool kRegAcc = DELTA;
    double accA[kRegAcc ? DM_NBUCKETS : 1], accB[kRegAcc ? DM_NBUCKETS : 1];
#pragma unroll
    for (int k = 0; k < (kRegAcc ? DM_NBUCKETS : 1); ++k) accA[k] = accB[k] = 0.0;
    double accSW = 0.0;

    ESLAM_STAMP_WAVE(1);
    for (uint32_t j = 0; j < J; ++j) {
        const uint64_t row0 = lbase + 64ull * j;
        if (row0 >= n) break;
        if (ESLAM_K1_PACE != 0) {
            // nothing of this is live across the row: the band is recomputed from j and J.  J
            // passes through an empty asm, or the compiler hoists 2 J, 3 J and J > 1 out of the
            // loop into four long-lived SGPRs (one spilled: 97 VGPRs, four waves)
            uint32_t Jp = J;
            asm volatile("" : "+s"(Jp));
            if (Jp > 1u) {
                const uint32_t level = k1_pace_level(j, Jp);
                if (j == 0 || level != k1_pace_level(j - 1u, Jp)) k1_set_priority(level);
            }
        }
        const uint64_t i = row0 + lane;
        uint32_t src = (uint32_t)i;
        const gmem<const Rec>* rc = nullptr;
        uint32_t rec_anc = 0;
        bool clr = false;                        // this output's segment mark is set
        // The row's memory operations are ordered so that each wait covers only what its
        // consumer needs (vmcnt retires loads in issue order): the marks and the carry are
        // requested first and the draws, which need only the particle's index, are computed
        // while they fly; the Box-Muller table rows come from LDS (bm_lds) or are requested
        // before the gathered state, so the Box-Muller arithmetic waits for the tables alone
        // and runs under the state's latency; the state is waited for where theta is first
        // used.  The same operations on the same operands as in source order: the same bits.
        dm_philox_ctr d0 = {}, d1 = {};
        dm_bm_rows_t t0 = {}, t1 = {};
        su8 key = {};                            // seed, proj_event, gbase
        auto draws = [&]() {
            if (!PROJECT) return;
            const uint64_t gi = kq(key, 2) + i;
            // draw layout: call 0 -> two Box-Muller pairs (z0, z1), (z2, sn0);
            // call 1 -> slip test + slip factor, spread pair (sn1, sn2).  A lane past n draws
            // too (a pure function of its index) and uses nothing of it.
            d0 = dm_draw(kq(key, 0), DM_STREAM_PROJECT, kq(key, 1), gi, 0);
            d1 = dm_draw(kq(key, 0), DM_STREAM_PROJECT, kq(key, 1), gi, 1);
            // the words are used under i < n only, where the compiler would sink the whole
            // computation, behind the wait for the marks: this keeps it here
            asm volatile("" ::"v"(d0.v[0]), "v"(d0.v[1]), "v"(d0.v[2]), "v"(d0.v[3]), "v"(d1.v[0]), "v"(d1.v[1]),
                         "v"(d1.v[2]), "v"(d1.v[3]));
        };
        if (gath) {
            su8 g;                                    // marks, row_first, anc, recs
            su2 gf;                                   // record, multi
            if constexpr (PROJECT) kl8_2_8(g, KOFF(gv), gf, KOFF(gv.record), key, KOFF(p.seed));
            else kl8_2(g, KOFF(gv), gf, KOFF(gv.record));
            // a lane past n (the last row only) reads the last particle's mark and drops it: the
            // load stands in no branch, so nothing waits for it before the draws
            const uint32_t carry = kp<const uint32_t>(g, 1)[row0 / kRow] + 1u;
            uint32_t m = kp<uint32_t>(g, 0)[i < n ? i : n - 1];
            draws();
            // expand the segment marks of this row: inclusive max-scan + the row carry.  The
            // mark is cleared with the row's other stores at its end (vmcnt counts stores too: a
            // store here would add its round trip to the wait before the state loads)
            m = i < n ? m : 0u;
            clr = m != 0;
            m = wave_incl_max_u32(m);
            m = m > carry ? m : carry;
            src = decode_source(m - 1u, gf[1], kp<const Rec>(g, 3), &rc);
            rec_anc = gf[0];
        } else {
            if constexpr (PROJECT) key = kl8(KOFF(p.seed));
            draws();
        }
        if (PROJECT) {
            if (bm_lds) {
                auto rows = [&](uint32_t wa, uint32_t wb) {
                    const double* l = reinterpret_cast<const double*>(bm_tab) + 4 * dm_log_bm_row(dm_u32(wa));
                    const float* e = reinterpret_cast<const float*>(bm_tab + 4096) + 2 * (wb >> 24);
                    dm_bm_rows_t t;
                    t.l0 = l[0]; t.l1 = l[1]; t.l2 = l[2];
                    t.s = e[0]; t.c = e[1];
                    return t;
                };
                t0 = rows(d0.v[0], d0.v[1]);
                t1 = rows(d0.v[2], d0.v[3]);
            } else {
                t0 = dm_bm_rows(d0.v[0], d0.v[1]);
                t1 = dm_bm_rows(d0.v[2], d0.v[3]);
            }
            __builtin_amdgcn_sched_barrier(0);       // the table loads stay in front of the state's
        }
        // lanes past n (only in the last row of the last chunk) compute nothing but take part
        // in the row's bucket walk, so the walk's state stays wave-uniform (scalar)
        uint32_t bucket = kNoBucket;
        double am = 0.0, am2 = 0.0;
        bool rowerr = false;
        if (i < n) {
        double x, y, th, z, zs, w, mp_in = 0.0;
        uint32_t fl_in = 0;
        if (rc) {
            x = rc->x; y = rc->y; th = rc->th; z = rc->z; zs = rc->zs; w = rc->w;
            mp_in = rc->mprob; fl_in = (uint8_t)rc->src;
        } else {
            const StatePtrs si = kstate(si_off);
            x = si.x[src]; y = si.y[src]; th = si.th[src]; z = si.z[src];
            zs = si.zs[src]; w = si.w[src];
            if (!WEIGHT && gath) { mp_in = si.mprob[src]; fl_in = si.flags[src]; }
        }
        if (gath && rec_anc) {
            const su2 ga = kl2(KOFF(gv.anc));
            const uint64_t gbase = kq(kl2(KOFF(p.gbase)), 0);
            kp<uint32_t>(ga, 0)[i] = rc ? (uint32_t)(rc->src >> 8) : (uint32_t)(gbase + src);
        }
        const double w_in = w;
        double mprob = 0.0;
        uint32_t flags = 0;
        if (PROJECT) {
            // the sampler's and the z motion's arguments in one group, waited for while the
            // table rows and the state are in flight
            su16 P;                                  // mu0 mu1 mu2 L00 L10 L11 L20 L21
            su8 Q;                                   // L22 slip_factor yaw max_yaw_dev
            su4 Z;                                   // z_delta z_var
            kl16_8_4(P, KOFF(p.mu), Q, KOFF(p.L22), Z, KOFF(p.z_delta));
            double z0, z1, z2, sn0;
            dm_box_muller32_e(d0.v[0], d0.v[1], t0, &z0, &z1);
            dm_box_muller32_e(d0.v[2], d0.v[3], t1, &z2, &sn0);
            // odometry.getPoseDeltaSample2D() = mu + L z
            const double dx = kd(P, 0) + kd(P, 3) * z0;
            double dy = kd(P, 1) + (kd(P, 4) * z0 + kd(P, 5) * z1);
            const double dth = kd(P, 2) + ((kd(P, 6) * z0 + kd(P, 7) * z1) + kd(Q, 0) * z2);
            if (dm_u32(d1.v[0]) < kd(Q, 1)) dy *= dm_u32(d1.v[1]);
            // the first use of the gathered state.  The pose delta is complete in front of it (the
            // compiler would sink the Box-Muller arithmetic behind the wait for the state, next
            // to its uses), and nothing of the state moves up into that arithmetic, which would
            // bring the wait with it
            asm volatile("" ::"v"(dx), "v"(dy), "v"(dth));
            __builtin_amdgcn_sched_barrier(0);
            double s, co;
            dm_sincos(th, &s, &co);
            x += co * dx - s * dy;
            y += s * dx + co * dy;
            th += dth;
            if (kd(Q, 3) > 0.0) {
                if (dm_fabs(th - kd(Q, 2)) > kd(Q, 3)) w *= 0.7;
            }
            z += kd(Z, 0);
            zs = dm_sqrt_fast(zs * zs + kd(Z, 1));
            if (do_spread) {
                double sn1, sn2;
                dm_box_muller32(d1.v[2], d1.v[3], &sn1, &sn2);
                x += sn0 * tf + 0.0;
                y += sn1 * tf + 0.0;
                th += sn2 * rf + 0.0;
            }
        }
        if (WEIGHT) {
            double s, co;
            dm_sincos(th, &s, &co);
            const double r22 = (1.0 - co) + co;
            // the weighting's arguments, one group per row
            su8 wp;                                  // me2, radius, corr, min_contacts
            su4 wq;                                  // use_shape, m, eval_mask, end_mask
            kl8_4(wp, KOFF(p.me2), wq, KOFF(p.use_shape));
            const double meas_var = zs * zs + kd(wp, 0);
            uint32_t sid = 0;
            if constexpr (DELTA) {
                // per-particle maps: the host materialises every gather first, so particle i
                // is at i; its store name sits next to the state (DevState::sid)
                sid = store_sid(kp<const uint32_t>(kl2(st_off + (uint32_t)offsetof(DevState, sid)), 0)[i]);
            }
            CMResult r = evaluate_pose<MAXP, BATCH, DELTA, UNG>(win, co, s, r22, x, y, z, meas_var, sid, wp, wq);
            if (meas_var == 0) {            // evaluatePose throws (src/ContactModel.cpp:122): no contact points
                rowerr = true;
                r.accepted = false;
                r.ncp = 0;
            }
            uint32_t floating;
            double sw = 0.0;
            if (r.accepted) {
                // ContactModel::updateZPositionEstimate  src/ContactModel.cpp:319-340
                double zvar = zs * zs;
                // posevar / found: a power-of-two count divides exactly as a multiplication by
                // its reciprocal (the same correctly rounded quotient)
                const double inv_n = dm_recip_small(r.ncp);     // 1.0 / found, correctly rounded
                double pose_var;
                if (r.ncp != 0u && (r.ncp & (r.ncp - 1u)) == 0u) pose_var = r.posevar * inv_n;
                else pose_var = r.posevar / (double)r.ncp;
                const double av = zvar - pose_var;
                double delta_var = (av < 1e-9) ? 1e-9 : av;
                if (!(r.zdelta * r.zdelta > delta_var)) {
                    const double gain = zvar / (zvar + r.zvar);
                    z += gain * r.zdelta;
                    const double var_gain = delta_var / (delta_var + r.zvar);
                    delta_var = (1.0 - var_gain) * delta_var;
                    zvar = pose_var + delta_var;
                }
                zs = dm_sqrt_fast(zvar);
                if (r.ncp == 0u) {
                    // accepted without a contact point (minContacts = 0): delta = 0 * (1 / 0) and
                    // poseVar = 0 / 0 make zPos and zSigma NaN; the contract stores the canonical
                    // quiet NaN (a generated NaN's sign and payload are the processor's)
                    z = dm_from_bits(0x7ff8000000000000ull);
                    zs = dm_from_bits(0x7ff8000000000000ull);
                }
                w *= r.weight;
                mprob = r.weight;
                floating = 0;
                maxm = (maxm < r.weight) ? r.weight : maxm;
                nDTP += 1u + (r.ncp << 16);
                // pow(weight, 1.0/found) with weight = exp(-s2/2): exp(-s2/2 * (1/found))
                const uint32_t use_shape = wq[0];
                if (!use_shape || r.ncp == 0) sw = dm_pow(r.weight, inv_n);
                else sw = r.weight == 0.0 ? 0.0 : dm_exp((-0.5 * r.s2) * inv_n);
            } else {
                floating = 1;
                mprob = 1.0;
            }
            bucket = r.ncp < DM_NBUCKETS - 1 ? r.ncp : DM_NBUCKETS - 1;
            am = w * mprob;
            am2 = am * am;
            accSW = accSW + sw;
            flags = (r.ncp & 0x7fu) | (floating << 7);
        } else {
            mprob = mp_in;
            flags = fl_in;
        }
        // all stores of the row at the end: the output pointers and, for the clear, the marks
        // pointer in one group
        su16 so;
        su2 mp = {};
        if (gath) kl16_2(so, st_off, mp, KOFF(gv.marks));
        else so = kl16(st_off);
        const StatePtrs st = state_ptrs(so);
        if (PROJECT || gath) {
            K1_ST(st.x + i, x);
            K1_ST(st.y + i, y);
            K1_ST(st.th + i, th);
        }
        if (WEIGHT || gath) {
            K1_ST(st.mprob + i, mprob);
            K1_ST(st.flags + i, (uint8_t)flags);
        }
        if (PROJECT || WEIGHT) {
            K1_ST(st.z + i, z);
            K1_ST(st.zs + i, zs);
            if (gath || w != w_in || w != w) K1_ST(st.w + i, w);
        }
        if (clr) kp<uint32_t>(mp, 0)[i] = 0;
        {
            // v_max_f32 returns the other operand for a NaN: NaN coordinates are skipped
            const float xf = (float)x, yf = (float)y;
            bb[0] = __builtin_fmaxf(bb[0], -xf);
            bb[1] = __builtin_fmaxf(bb[1], xf);
            bb[2] = __builtin_fmaxf(bb[2], -yf);
            bb[3] = __builtin_fmaxf(bb[3], yf);
        }
        }
        if (WEIGHT) {
            // per bucket b the lane adds am if it holds b, else +0.0 (the oracle's canonical
            // per-bucket sums add +0.0 for the other buckets' particles: the same bits).  The
            // wave walks its distinct buckets (usually one): each pass adds to one bucket's two
            // sums, chosen by a scalar branch, instead of selecting over every bucket per lane.
            // ncp <= MAXP: the buckets above MAXP stay empty.  The whole wave walks (lanes
            // without a particle add +0.0), so cur_b and touched are scalars.
            werr |= __ballot(rowerr) != 0ull ? 1u : 0u;
            uint64_t todo = __ballot(bucket != kNoBucket);
            while (todo) {
                const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bucket, (int)__builtin_ctzll(todo));
                const bool mine = bucket == b0;
                if constexpr (kRegAcc) {
                    touched |= 1u << b0;
#pragma unroll
                    for (uint32_t k = 0; k < (uint32_t)DM_NBUCKETS; ++k) {
                        if (k == b0) {                   // scalar branch (b0 is wave-uniform)
                            accA[k] = accA[k] + (mine ? am : 0.0);
                            accB[k] = accB[k] + (mine ? am2 : 0.0);
                        }
                    }
                    todo &= ~__ballot(mine);
                    continue;
                }
                if (b0 != cur_b) {
                    // the wave moves to another bucket: park the current pair, take b0's (a
                    // bucket the wave never walked starts at +0.0)
                    gmem<double>* sp = kp<double>(kl2(KOFF(bspill)), 0) + chunk * (DM_NBUCKETS * 128) + lane;
                    if (cur_b != kNoBucket) {
                        sp[cur_b * 128] = curA;
                        sp[cur_b * 128 + 64] = curB;
                    }
                    curA = curB = 0.0;
                    if ((touched >> b0) & 1u) {
                        curA = sp[b0 * 128];
                        curB = sp[b0 * 128 + 64];
                    }
                    cur_b = b0;
                }
                touched |= 1u << b0;
                curA = curA + (mine ? am : 0.0);
                curB = curB + (mine ? am2 : 0.0);
                todo &= ~__ballot(mine);
            }
        }
    }
    // back to the launch's priority: a short last chunk leaves the loop in a raised band, and
    // the block's flush below meets its other waves at a barrier
    if (ESLAM_K1_PACE != 0 && J > 1u) __builtin_amdgcn_s_setprio(0);
    ESLAM_STAMP_WAVE(2);

    if (WEIGHT) {
        // chunk totals (sub-lane sums + the xor butterfly of the sum contract) -> exact fixed
        // point -> lane columns.  The butterfly runs transposed over the 2 * NB + 1 totals
        // (padded to 16): at distances 32, 16, 8 and 4 each lane pair splits the totals it
        // holds in halves and adds the half it keeps, so total q ends in lanes 4q..4q+3 after
        // the same pairwise additions as its own butterfly (the same bits); distances 2 and 1
        // finish it there, and each lane converts its total once and keeps limb lane & 3.
        constexpr int kQ = 2 * DM_NBUCKETS + 1;
        static_assert(kQ <= 16, "16 totals over the 64 lanes");
        const uint32_t q = lane >> 2;
        double t;
        // `touched` is only updated by the lanes active in a walk: lanes past n in the last row
        // keep an older set.  Lane 0 takes part in every walk (a row runs only if row0 < n), so
        // its set is complete, and read as a scalar the branch below is wave-uniform.
        const uint32_t touched0 = touched;
        if (__builtin_popcount(touched0) <= 1) {
            // the usual wave: every row's particles in one bucket b0, so the totals of the
            // other buckets are +0.0 (nothing was added to them) and the register pair holds
            // the sums of b0.  The
            // butterfly runs over A_b0, B_b0 and SW only (transposed at distances 32 and 16:
            // total k ends in lanes 16k..16k+15), the same pairwise additions, and lane 4q + c
            // picks total q.
            const uint32_t b0 = touched0 ? (uint32_t)__builtin_ctz(touched0) : 0u;
            if constexpr (kRegAcc) {
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)DM_NBUCKETS; ++k)
                    if (k == b0) { curA = accA[k]; curB = accB[k]; }
            }
            double w4[4] = {curA, curB, accSW, 0.0};
            transpose_add<32, 2>(w4, lane);
            transpose_add<16, 1>(w4, lane);
            double u = w4[0];
            u = u + xor_lane<8>(u);
            u = u + xor_lane<4>(u);
            u = u + xor_lane<2>(u);
            u = u + xor_lane<1>(u);
            auto lane_value = [](double x, int l) {      // v_readlane of both halves
                const uint64_t b = dm_bits(x);
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
                return dm_from_bits(((uint64_t)hi << 32) | lo);
            };
            const double tA = lane_value(u, 0), tB = lane_value(u, 16), tS = lane_value(u, 32);
            t = q == b0 ? tA : (q == DM_NBUCKETS + b0 ? tB : (q == kQ - 1 ? tS : 0.0));
        } else {
            // several buckets: the sums of bucket k are the register pair (k == cur_b), the
            // parked pair (a bucket the wave left), or +0.0 (a bucket it never walked)
            const gmem<const double>* sp = kp<const double>(kl2(KOFF(bspill)), 0) + chunk * (DM_NBUCKETS * 128) + lane;
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                v[k] = k == kQ - 1 ? accSW : 0.0;
                if (k < 2 * DM_NBUCKETS) {
                    const uint32_t b = (uint32_t)(k < DM_NBUCKETS ? k : k - DM_NBUCKETS);
                    if constexpr (kRegAcc) v[k] = k < DM_NBUCKETS ? accA[b] : accB[b];
                    else if (b == cur_b) v[k] = k < DM_NBUCKETS ? curA : curB;
                    else if ((touched >> b) & 1u) v[k] = sp[b * 128 + (k < DM_NBUCKETS ? 0 : 64)];
                }
            }
            transpose_add<32, 8>(v, lane);
            transpose_add<16, 4>(v, lane);
            transpose_add<8, 2>(v, lane);
            transpose_add<4, 1>(v, lane);
            t = v[0];
            t = t + xor_lane<2>(t);
            t = t + xor_lane<1>(t);
        }
        const int scale = q < DM_NBUCKETS ? sa : (q < 2 * DM_NBUCKETS ? sb : DM_FX_SCALE);
        const bool nan_ = t != t, inf_ = !nan_ && !dm_isfinite(t);
        uint32_t l[4] = {0, 0, 0, 0};
        if (!nan_ && !inf_) dm_fx128_limbs(t, scale, l);          // padding totals are 0: limbs 0
        const uint32_t c = lane & 3u;
        limb += c == 0 ? l[0] : (c == 1 ? l[1] : (c == 2 ? l[2] : l[3]));
        const uint64_t mn = __ballot(nan_), mi = __ballot(inf_);
#pragma unroll
        for (int k = 0; k < kQ; ++k) {
            if ((mn >> (4 * k)) & 1ull) flag |= 1u << k;
            if ((mi >> (4 * k)) & 1ull) flag |= 1u << (k + 16);
        }
    }
    }

    ESLAM_STAMP_K1(2);
    Shard* shb = a.shards + (blockIdx.x % kNShard);
    // bounding box of the cloud for the next step's LDS window (maxima, any order): the four
    // maxima in one transposed butterfly (at distances 32 and 16 each lane pair keeps half of
    // them), so value q ends in lanes 16q..16q+15 and lane 16q publishes it
    {
        transpose_op<32, 2>(bb, lane, [](float a, float b) { return __builtin_fmaxf(a, b); });
        transpose_op<16, 1>(bb, lane, [](float a, float b) { return __builtin_fmaxf(a, b); });
        float m = bb[0];
        m = __builtin_fmaxf(m, xor_lane<8>(m));
        m = __builtin_fmaxf(m, xor_lane<4>(m));
        m = __builtin_fmaxf(m, xor_lane<2>(m));
        m = __builtin_fmaxf(m, xor_lane<1>(m));
        const float xmax = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(m), 16));
        if ((lane & 15u) == 0u && xmax > -INFINITY) {
            const uint32_t q = lane >> 4;
            // |x - (float)x| <= 2^-24 |x| + 2^-150: widen outward, then the order key
            const double v = (double)m;
            const double wv = v + (dm_fabs(v) * 0x1p-22 + 0x1p-140);
            const uint64_t k = order_key((q & 1u) ? wv : -wv);
            atomicMax((unsigned long long*)&shb->bbox[q], (unsigned long long)((q & 1u) ? k : ~k));
        }
    }

    if (!WEIGHT) return;

    // ---- exact statistics: wave columns -> block (LDS) -> sharded atomics ----
    struct StatsLds {
        uint64_t limb[kWaves][(2 * DM_NBUCKETS + 1) * 4];
        uint32_t flag[kWaves];
        uint32_t cnt[kWaves][2];
        double mx[kWaves];
    };
    static_assert(sizeof(StatsLds) <= kStatsLds, "stats scratch");
    StatsLds& sl = *reinterpret_cast<StatsLds*>(smem);
    const double wmax = wave_max_butterfly(maxm);
    // the two counts in one sum: nD <= 64 J and nTP <= ESLAM_MAX_CONTACTS nD per wave (16 bits each)
    static_assert(64u * ESLAM_SUM_CHUNK_ROWS_MAX * ESLAM_MAX_CONTACTS < 65536u, "packed wave counts");
    static_assert(ESLAM_SUM_CHUNK_ROWS_MAX >= ESLAM_CHUNK_CAP, "the default chunk rows are accepted ones");
    const uint32_t wDTP = wave_sum_u32(nDTP);
    const uint32_t wD = wDTP & 0xffffu, wTP = wDTP >> 16;
    if (lane < (2 * DM_NBUCKETS + 1) * 4) sl.limb[wave][lane] = limb;
    if (lane == 0) {
        sl.flag[wave] = flag | (werr << 31);
        sl.cnt[wave][0] = wD;
        sl.cnt[wave][1] = wTP;
        sl.mx[wave] = wmax;
    }
    __syncthreads();
    Shard* sh = shb;
    const int t = threadIdx.x;
    if (t < (2 * DM_NBUCKETS + 1) * 4) {
        const int q = t >> 2, j = t & 3;
        uint64_t v = 0;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) v += sl.limb[wv][t];
        if (v) {
            uint64_t* dst = q < DM_NBUCKETS ? &sh->A[q][j] : (q < 2 * DM_NBUCKETS ? &sh->B[q - DM_NBUCKETS][j] : &sh->SW[j]);
            atomicAdd((unsigned long long*)dst, (unsigned long long)v);
        }
    } else if (t == 64) {
        uint64_t d = 0, tp = 0;
        uint32_t f = 0;
        double mx = 0.0;
        for (int wv = 0; wv < kWaves; ++wv) {
            d += sl.cnt[wv][0];
            tp += sl.cnt[wv][1];
            f |= sl.flag[wv];
            mx = (mx < sl.mx[wv]) ? sl.mx[wv] : mx;
        }
        if (d) atomicAdd((unsigned long long*)&sh->D, (unsigned long long)d);
        if (tp) atomicAdd((unsigned long long*)&sh->TP, (unsigned long long)tp);
        if (mx > 0.0) atomicMax((unsigned long long*)&sh->maxm, (unsigned long long)dm_bits(mx));
        if (f & 0x7fffffffu) atomicOr((unsigned long long*)&sh->flags, (unsigned long long)(f & 0x7fffffffu));
        if (f >> 31) atomicOr((unsigned long long*)&sh->err, 1ull);
    }
    ESLAM_STAMP_K1(3);
}

// ---------------------------------------------------------------------------------------
// k_contact_records (Configuration::logDebug / ESLAM_FLAG_RECORD_CONTACTS): the debug fields
// updateWeights stores in every PoseParticle (src/PoseEstimator.cpp:285-287, 322-325):
// meas_pos, meas_theta and cpoints.  Runs on the projected state between a project-only and
// a weight-only k_project_weight, so the weighting sees exactly the state these records
// describe.  ContactModel::evaluatePose (src/ContactModel.cpp:117-224) evaluated in contact
// order with the same arithmetic as evaluate_pose (the same pushes, bit for bit), recording
// each pushed ContactPoint: the surface point of the group's first valid contact (world x,
// y and the patch mean, :163-171), zdiff, zvar and prob = 1 (Q8).  One particle per thread,
// map lookups through the global CSR (the same values as the LDS window).
// ---------------------------------------------------------------------------------------
template <bool DELTA>
__global__ void __launch_bounds__(kBlock) k_contact_records(K1Args a, DebugRec d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (threadIdx.x < 8) k1_win[threadIdx.x] = 0;          // no LDS window: get_patch reads k1_win
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.p.n) return;
    const Ctl* ctl = a.ctl;
    const DevState& st = (ctl->base ^ ctl->flip) ? a.s[1] : a.s[0];
    const double x = st.x[i], y = st.y[i], th = st.th[i], z = st.z[i], zs = st.zs[i];
    Window win;
    win.on = 0;
    win.cells = reinterpret_cast<const WinCell*>(smem);
    double s, co;
    dm_sincos(th, &s, &co);
    const double r22 = (1.0 - co) + co;
    const double meas_var = zs * zs + a.p.me2;
    d.meas[4 * i + 0] = x;
    d.meas[4 * i + 1] = y;
    d.meas[4 * i + 2] = z;
    d.meas[4 * i + 3] = th;
    uint32_t ncp = 0;
    if (meas_var != 0) {
        bool valid = false, group_valid = true;
        double contact_ratio = 0, pzd = 0, pzv = 0, gx = 0, gy = 0, gm = 0;
        const double corr = a.p.corr;
        double* cp = d.cp + (uint64_t)6 * d.maxc * i;
        auto push = [&](double px, double py, double pm, double zd, double zv) {
            if (ncp < d.maxc) {
                double* r = cp + 6 * ncp;
                r[0] = px; r[1] = py; r[2] = pm; r[3] = zd; r[4] = zv; r[5] = 1.0;
            }
            ++ncp;
        };
        for (uint32_t k = 0; k < a.p.m; ++k) {
            const ContactC& c = a.p.c[k];
            const bool c_eval = (a.p.eval_mask >> k) & 1u, c_end = (a.p.end_mask >> k) & 1u;
            const double wx = ((co * c.px + (-s) * c.py) + c.zp) + x;
            const double wy = ((s * c.px + co * c.py) + c.zp) + y;
            const double wz = ((c.zz + r22 * c.pz) + z) - a.p.radius;
            if (group_valid && c_eval) {
                double mean = 0.0, stdev = 0.0;
                if (get_patch<DELTA>(win, wx, wy, wz, meas_var, mean, stdev, DELTA ? store_sid(st.sid[i]) : 0u)) {
                    const double zdiff = wz - mean;
                    const double zvar = stdev * stdev + meas_var;
                    if (!valid && c_end && ratio_surely_significant(zdiff, zvar, corr)) {
                        push(wx, wy, mean, zdiff, zvar);       // single-point group
                        continue;
                    }
                    const double ratio = dm_normal_pdf_cdf_ratio(zdiff, dm_sqrt(zvar) * corr);
                    if (!valid) {
                        pzd = zdiff * ratio; pzv = zvar * ratio; contact_ratio = ratio;
                        gx = wx; gy = wy; gm = mean;
                    } else {
                        pzd += zdiff * ratio; pzv += zvar * ratio; contact_ratio += ratio;
                    }
                    valid = true;
                } else {
                    group_valid = false;
                }
            }
            if (valid && c_end) {
                if (group_valid && contact_ratio > 1e-9) {
                    const double inv = 1.0 / contact_ratio;
                    push(gx, gy, gm, pzd * inv, pzv * inv);
                }
                group_valid = true;
                valid = false;
                contact_ratio = 0;
            }
        }
    }
    d.ncp[i] = (uint8_t)(ncp < 255u ? ncp : 255u);
}

// eslam_gpu_download_records: particles first + k * stride as PoseParticle records with their
// debug fields.  Particle i's records are those of the particle it descends from at the last
// update's resample (anc, global indices) -- the reference copies cpoints with the particle.
// On a sharded filter the host resolves the descent first (slot[k]: the record's position on
// this rank, or kRecRemote | its item in `remote`, fetched from the rank that held it).
constexpr uint64_t kRecRemote = 1ull << 63;
__device__ __forceinline__ uint32_t rec_items(uint32_t maxc) { return 5u + 6u * maxc; }    // doubles per item

__global__ void __launch_bounds__(kBlock) k_pack_records(DevState s0, DevState s1, const Ctl* __restrict__ ctl, uint64_t first,
                                                         uint64_t stride, uint64_t count, uint64_t gbase,
                                                         const uint32_t* __restrict__ anc, DebugRec d,
                                                         eslam_particle_record* __restrict__ out,
                                                         eslam_cpoint* __restrict__ cps, uint32_t max_cp,
                                                         const uint64_t* __restrict__ slot, const double* __restrict__ remote)
{
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    const uint64_t i = first + k * stride;
    const DevState& st = (ctl->base ^ ctl->flip) ? s1 : s0;
    eslam_particle_record r;
    r.position[0] = st.x[i];
    r.position[1] = st.y[i];
    r.orientation = st.th[i];
    r.zpos = st.z[i];
    r.zsigma = st.zs[i];
    r.mprob = st.mprob[i];
    r.weight = st.w[i];
    const uint8_t fl = st.flags[i];
    r.floating = fl >> 7;
    r.index = i + gbase;
    uint32_t n = 0;
    if (d.ncp) {
        const uint64_t s = slot ? slot[k] : (*d.resampled ? (uint64_t)anc[i] - gbase : i);
        const double *meas, *cp;
        if (s & kRecRemote) {                 // an item fetched from another rank
            const double* item = remote + (uint64_t)rec_items(d.maxc) * (s & ~kRecRemote);
            meas = item;
            n = (uint32_t)item[4];
            cp = item + 5;
        } else {
            meas = d.meas + 4 * s;
            n = d.ncp[s];
            cp = d.cp + (uint64_t)6 * d.maxc * s;
        }
        for (int q = 0; q < 3; ++q) r.meas_pos[q] = meas[q];
        r.meas_theta = meas[3];
        const uint32_t kept = n < d.maxc ? n : d.maxc;
        for (uint32_t q = 0; q < kept && q < max_cp; ++q) {
            const double* c = cp + 6 * q;
            eslam_cpoint& o = cps[(uint64_t)max_cp * k + q];
            o.point[0] = c[0]; o.point[1] = c[1]; o.point[2] = c[2];
            o.zdiff = c[3]; o.zvar = c[4]; o.prob = c[5];
        }
    } else {
        r.meas_pos[0] = r.meas_pos[1] = r.meas_pos[2] = 0.0;
        r.meas_theta = 0.0;
        n = fl & 0x7fu;
    }
    r.n_cpoints = n;
    out[k] = r;
}

// the records other ranks asked for (sharded download_records): item j = the debug fields
// of this rank's particle at global index req[j] during the last update (meas 4, ncp, cps)
__global__ void __launch_bounds__(kBlock) k_gather_records(const uint32_t* __restrict__ req, uint64_t nreq, uint64_t gbase,
                                                           DebugRec d, double* __restrict__ items)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nreq) return;
    const uint64_t s = (uint64_t)req[j] - gbase;
    double* o = items + (uint64_t)rec_items(d.maxc) * j;
    for (int q = 0; q < 4; ++q) o[q] = d.meas[4 * s + q];
    o[4] = (double)d.ncp[s];
    const double* c = d.cp + (uint64_t)6 * d.maxc * s;
    for (uint32_t q = 0; q < 6 * d.maxc; ++q) o[5 + q] = c[q];
}

// exclusive prefix sum of m counts in place, one block: chunks of 8192 counts are loaded and
// stored striped (coalesced, every load of a chunk in flight together) through LDS, where each
// thread scans 8 consecutive counts; the wave scans and a carry join the threads and chunks.
// (A thread per contiguous segment of m / 1024 counts read and wrote them one dependent load
// at a time: 73 us per call at 8M particles' 32k block sums.)
constexpr uint32_t kScanPer = 8, kScanChunk = 1024 * kScanPer;
__global__ void __launch_bounds__(1024) k_scan_excl(uint32_t* __restrict__ a, uint64_t m)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_v[kScanChunk];
    __shared__ uint32_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < m; base += kScanChunk) {
        const uint32_t cnt = m - base < kScanChunk ? (uint32_t)(m - base) : kScanChunk;
        uint32_t v[kScanPer];
#pragma unroll
        for (uint32_t q = 0; q < kScanPer; ++q) {
            const uint32_t k = q * 1024u + tid;
            v[q] = k < cnt ? a[base + k] : 0u;
        }
#pragma unroll
        for (uint32_t q = 0; q < kScanPer; ++q) s_v[q * 1024u + tid] = v[q];
        __syncthreads();
        const uint4 lo = reinterpret_cast<const uint4*>(s_v)[2 * tid], hi = reinterpret_cast<const uint4*>(s_v)[2 * tid + 1];
        const uint32_t u[kScanPer] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t tot = 0;
#pragma unroll
        for (uint32_t q = 0; q < kScanPer; ++q) tot += u[q];
        uint32_t incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t x = (uint32_t)__shfl_up((int)incl, o, 64);
            incl += lane >= (uint32_t)o ? x : 0u;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < 16; ++w) {
            before += w < wave ? s_w[w] : 0u;
            all += s_w[w];
        }
        uint32_t run = carry + before + (incl - tot);
        uint32_t r[kScanPer];
#pragma unroll
        for (uint32_t q = 0; q < kScanPer; ++q) { r[q] = run; run += u[q]; }
        reinterpret_cast<uint4*>(s_v)[2 * tid] = make_uint4(r[0], r[1], r[2], r[3]);
        reinterpret_cast<uint4*>(s_v)[2 * tid + 1] = make_uint4(r[4], r[5], r[6], r[7]);
        carry += all;
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < kScanPer; ++q) {
            const uint32_t k = q * 1024u + tid;
            if (k < cnt) a[base + k] = s_v[k];
        }
        __syncthreads();                 // s_v and s_w are reused by the next chunk
    }
}

// ---------------------------------------------------------------------------------------
// k_weight_stats: exact sum of the weights and of their squares (standalone
// getWeightsSum / normalizeWeights / resample, src/ParticleFilter.hpp:34-70)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_weight_stats(DevState s0, DevState s1, uint64_t n, uint32_t J,
                                                         Ctl* __restrict__ ctl, Shard* __restrict__ shards)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t lbase = ((uint64_t)blockIdx.x * kWaves + wave) * 64ull * J;
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    const int wexp = ctl->wexp;
    double a = 0.0, b = 0.0;
    for (uint32_t j = 0; j < J; ++j) {
        const uint64_t i = lbase + 64ull * j + lane;
        if (i >= n) continue;
        const double w = st.w[i];
        a = a + w;
        b = b + dm_stat_sq(w, wexp);        // (w 2^-wexp)^2: in range at any weight scale
    }
    __shared__ uint32_t s_limb[kWaves][2][4];
    __shared__ uint32_t s_flag[kWaves];
    uint32_t flag = 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        double v = q == 0 ? a : b;
        uint32_t l[4] = {0, 0, 0, 0};
        if (__ballot(v != 0.0) != 0ull) {
            v = wave_sum_butterfly(v);
            if (v != v) flag |= 1u << (q * DM_NBUCKETS);
            else if (!dm_isfinite(v)) flag |= 1u << (q * DM_NBUCKETS + 16);
            else dm_fx128_limbs(v, q == 0 ? DM_FX_SCALE - wexp : DM_FX_SCALE, l);
        }
        if (lane == 0) for (int j = 0; j < 4; ++j) s_limb[wave][q][j] = l[j];
    }
    if (lane == 0) s_flag[wave] = flag;
    __syncthreads();
    Shard* sh = shards + (blockIdx.x % kNShard);
    const int t = threadIdx.x;
    if (t < 8) {
        const int q = t >> 2, j = t & 3;
        uint64_t v = 0;
        for (int wv = 0; wv < kWaves; ++wv) v += s_limb[wv][q][j];
        if (v) atomicAdd((unsigned long long*)(q == 0 ? &sh->A[0][j] : &sh->B[0][j]), (unsigned long long)v);
    } else if (t == 64) {
        uint32_t f = 0;
        for (int wv = 0; wv < kWaves; ++wv) f |= s_flag[wv];
        if (f) atomicOr((unsigned long long*)&sh->flags, (unsigned long long)f);
    }
}

// ---------------------------------------------------------------------------------------
// k_finalize: one block.  Sums the shards exactly, then the scalar part of the update.
// ---------------------------------------------------------------------------------------
constexpr int kShardFields = 2 * DM_NBUCKETS * 4 + 4 + 5 + 4;   // A, B, SW, D, TP, maxm, flags, err, bbox

__device__ __forceinline__ double acc_value(const uint64_t* L, uint64_t flags, int qbit, int scale)
{
    if (flags & (1ull << qbit)) return __builtin_nan("");
    if (flags & (1ull << (qbit + 16))) return __builtin_inf();
    return dm_limbs_to_double(L, scale);
}

// combine field t of nrec statistics records exactly (sum / max / or by field) and zero them
// (exact integers: any grouping gives the same value)
__device__ __forceinline__ uint64_t reduce_field(Shard* recs, int nrec, int t)
{
    constexpr int kCap = kNShard;
    uint64_t acc = 0;
    const int base = 2 * DM_NBUCKETS * 4 + 4;                                  // D
    for (int k0 = 0; k0 < nrec; k0 += kCap) {
        // a group's loads first (they are independent), then combine: one memory latency
        uint64_t v[kCap];
#pragma unroll
        for (int k = 0; k < kCap; ++k) v[k] = k0 + k < nrec ? reinterpret_cast<const uint64_t*>(recs + k0 + k)[t] : 0ull;
#pragma unroll
        for (int k = 0; k < kCap; ++k)
            if (k0 + k < nrec) reinterpret_cast<uint64_t*>(recs + k0 + k)[t] = 0;
#pragma unroll
        for (int k = 0; k < kCap; ++k) {
            if (k0 + k >= nrec) break;
            if (t == base + 2 || t >= base + 5) acc = acc > v[k] ? acc : v[k];      // maxm, bbox
            else if (t == base + 3 || t == base + 4) acc |= v[k];                   // flags, err
            else acc += v[k];
        }
    }
    return acc;
}

// LDS of the finalize: the combined shard fields, the exact sums A_b, B_b, SW as doubles and
// the phase-B factors
struct FinLds {
    uint64_t s[kShardFields];
    double acc[2 * DM_NBUCKETS + 1];
    double f[DM_NBUCKETS];
};

// the finalize of one block (every thread calls it).  recs: kNShard local shards (one GPU)
// or the gathered per-rank records (multi-GPU)
__device__ __forceinline__ void finalize_block(Shard* __restrict__ recs, int nrec, Ctl* __restrict__ ctl, const FinParams& fp, FinLds& L)
{
    uint64_t* s = L.s;
    double* s_acc = L.acc;
    double* s_f = L.f;
    const int t = threadIdx.x;
    // the control fields the finalize reads, loaded with the shards (one memory round trip)
    const int wexp_ = ctl->wexp;
    uint32_t base0 = 0, flip0 = 0, minstd0 = 0;
    double last_max = 0.0;
    uint64_t updates0 = 0;
    if (t == 0) {
        base0 = ctl->base; flip0 = ctl->flip; minstd0 = ctl->minstd;
        last_max = ctl->max_weight; updates0 = ctl->update_count;
    }
    if (t < kShardFields) {
        s[t] = reduce_field(recs, nrec, t);
        // multi-GPU: the local shards were all-gathered (stream order: already read)
        if (fp.local_shards)
            for (int k = 0; k < kNShard; ++k) reinterpret_cast<uint64_t*>(fp.local_shards + k)[t] = 0;
    }
    __syncthreads();
    {
        // the 13 fixed-point -> double conversions, one per lane (same values as serially).  The
        // weight sums A_b and the sums of squares B_b are read scaled by 2^-wexp and 2^-2 wexp
        // (accumulated at DM_FX_SCALE - wexp and DM_FX_SCALE - 2 wexp, or the squares already
        // scaled: k_weight_stats), so the effective count below is in range at any weight scale
        const uint64_t flags_ = s[2 * DM_NBUCKETS * 4 + 7];
        if (t < 2 * DM_NBUCKETS + 1) s_acc[t] = acc_value(s + 4 * t, flags_, t, DM_FX_SCALE);
        __syncthreads();
        // phase-B factors (0.9 fw)^(4 - n), one bucket per lane
        if (fp.mode == FIN_UPDATE && t < DM_NBUCKETS) {
            const uint64_t D_ = s[2 * DM_NBUCKETS * 4 + 4];
            const double fw_ = D_ > 0 ? s_acc[2 * DM_NBUCKETS] / (double)D_ : 1.0;
            s_f[t] = dm_pow(fp.discount * fw_, (double)(uint64_t)(4ull - (uint64_t)t));
        }
        __syncthreads();
    }
    if (t != 0) return;

    const uint64_t D = s[2 * DM_NBUCKETS * 4 + 4];
    const uint64_t TP = s[2 * DM_NBUCKETS * 4 + 5];
    const double maxm = dm_from_bits(s[2 * DM_NBUCKETS * 4 + 6]);
    const uint64_t err = s[2 * DM_NBUCKETS * 4 + 8];
    if (s[2 * DM_NBUCKETS * 4 + 10]) {                 // a weighting kernel saw particles
        for (int q = 0; q < 4; ++q) ctl->bbox[q] = s[2 * DM_NBUCKETS * 4 + 9 + q];
    }
    // commit the previous resample's buffer flip
    ctl->base = base0 ^ flip0;
    ctl->flip = 0;
    ctl->gather = 0;
    if (err) atomicOr((unsigned long long*)&ctl->err, (unsigned long long)err);   // K3 blocks may OR in too
    ctl->tile_counter = 0;
    ctl->overruns = 0;
    ctl->aborted = 0;
    const double N = (double)fp.n_global;
    if (fp.mode == FIN_UPDATE && err) {
        // evaluatePose threw (src/ContactModel.cpp:122-123): updateWeights stops after its
        // particle loop has run, before the floating weight, phase B, the max-weight update,
        // normalizeWeights and resample (src/PoseEstimator.cpp:276-352, 244-255)
        ctl->aborted = 1;
        ctl->resample = 0;
        if (fp.mirror) { fp.mirror[0] = 0; fp.mirror[1] = ctl->minstd_start; fp.mirror[2] = (uint64_t)(int64_t)ctl->scan_shift; }
        return;
    }

    double S = 0.0, Q = 0.0;
    if (fp.mode == FIN_UPDATE) {
        const double SW = s_acc[2 * DM_NBUCKETS];
        const double fw = D > 0 ? SW / (double)D : 1.0;
        for (int b = 0; b < DM_NBUCKETS; ++b) {
            const double fb = s_f[b];
            ctl->f[b] = fb;
            S = S + fb * s_acc[b];
            Q = Q + (fb * fb) * s_acc[DM_NBUCKETS + b];
        }
        ctl->fw = fw;
        const double last = last_max;
        double mw = maxm;
        if (TP == 0) mw = last * fp.discount;
        ctl->max_weight = mw;
        ctl->data_particles = D;
        ctl->total_points = TP;
        ctl->update_count = updates0 + 1;
    } else {
        S = s_acc[0];
        Q = s_acc[DM_NBUCKETS];
        for (int b = 0; b < DM_NBUCKETS; ++b) ctl->f[b] = 1.0;
    }
    const double Ss = S;                                // S 2^-wexp; Q stays scaled (2^-2 wexp)
    S = dm_ldexp(Ss, wexp_);
    ctl->S = S;
    ctl->Q = Q;
    ctl->inv_n = 1.0 / N;

    if (fp.mode == FIN_UPDATE || fp.mode == FIN_NORMALIZE) {
        double eff;
        ctl->uniform = 0;
        if (S <= 0.0) {
            ctl->uniform = 1;
            eff = 1.0 / (1.0 / N);
        } else {
            eff = 1.0 / (Q / (Ss * Ss));
        }
        ctl->eff = eff;
        ctl->wexp = 1;
        ctl->scan_shift = 60;
        ctl->resample = (fp.mode == FIN_UPDATE && eff < (double)fp.min_effective) ? 1u : 0u;
    } else if (fp.mode == FIN_RESAMPLE) {
        ctl->resample = 1;
        ctl->scan_shift = 61 - (dm_weight_exp(S) + 1);
    } else {
        ctl->resample = 0;
    }
    if (fp.mirror) {
        fp.mirror[0] = ctl->resample;
        fp.mirror[1] = ctl->resample ? minstd0 : ctl->minstd_start;      // minstd_start below
        fp.mirror[2] = (uint64_t)(int64_t)ctl->scan_shift;
    }
    if (ctl->resample) {
        ctl->minstd_start = minstd0;
        ctl->minstd = dm_mulmod31(fp.minstd_jump_n, minstd0);       // A^N, precomputed
        ctl->flip = 1;
        ctl->gather = 1;
    }
}

__global__ void __launch_bounds__(kBlock) k_finalize(Shard* __restrict__ recs, int nrec, Ctl* __restrict__ ctl, FinParams fp)
{
    __shared__ FinLds L;
    finalize_block(recs, nrec, ctl, fp, L);
}

// ---------------------------------------------------------------------------------------
// count of stratified draws T_k = fx(((k + U_k) / N), shift) that are <= c
// (U_k = boost uniform_real of the (k+1)-th minstd draw after x_start)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t fx_shift(double v, int shift) { return dm_fx_shift(v, shift); }

// dm_fx_shift(q, shift) for 0 <= q <= 1 without branches: then sh = e - 1075 + shift <= 9
// (shift <= 61), inside the general function's "m << sh" range, and q = +0 or subnormal
// (e = 0) gives 0 as there
__device__ __forceinline__ uint64_t fx_unit(double q, int shift)
{
    const uint64_t b = dm_bits(q);
    const uint32_t e = (uint32_t)(b >> 52);
    const uint64_t m = (b & 0x000fffffffffffffull) | 0x0010000000000000ull;
    const int sh = (int)e - 1075 + shift;
    const uint64_t r = sh >= 0 ? (m << (sh & 63)) : (m >> ((-sh) & 63));
    return ((e == 0u) | (sh <= -64)) ? 0ull : r;
}

// T_k = fx((k + U_k) / N): both divisions as dm_div_recip (bit-identical to "/", checked by
// tests/c/check_div.c); inv_N = 1.0 / N.  k < N < 2^32, so (k + U_k) / N <= 1.
__device__ __forceinline__ uint64_t draw_fx(uint64_t k, uint32_t x, double dN, double inv_N, int shift)
{
    return fx_unit(dm_div_recip((double)(uint32_t)k + dm_minstd_uniform_fast(x), dN, inv_N), shift);
}

__device__ __forceinline__ uint64_t count_draws_le(uint64_t c, uint64_t N, uint32_t xs, int shift,
                                                   const uint32_t* __restrict__ jt)
{
    const unsigned __int128 prod = (unsigned __int128)c * N;
    const uint64_t kstar = (uint64_t)(prod >> shift);
    const uint64_t k0 = kstar >= 1 ? kstar - 1 : 0;
    if (k0 >= N) return N;
    uint64_t cnt = k0;
    uint32_t x = dm_mulmod31(jump_pow(jt, k0 + 1), xs);
    const double dN = (double)N, inv_N = 1.0 / dN;
    for (uint64_t k = k0; k <= kstar + 1 && k < N; ++k) {
        const uint64_t T = draw_fx(k, x, dN, inv_N, shift);
        if (T <= c) cnt = k + 1;
        else break;
        x = dm_minstd_next(x);
    }
    return cnt;
}

// phase B (updateWeights' second pass, src/PoseEstimator.cpp:332-344) + normalisation
// (src/ParticleFilter.hpp:46-70) of one tile's items r * kBlock + tid, in place; v[r] is the
// final weight (0 past the filter's end).  Every load of the tile is issued first (indices
// clamped into the filter: no branches between them), so their latencies overlap instead of
// costing one memory round trip per item.
__device__ __forceinline__ uint32_t sgpr_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ double sgpr_f64(double v)
{
    const uint64_t b = dm_bits(v);
    return dm_from_bits(((uint64_t)sgpr_u32((uint32_t)(b >> 32)) << 32) | sgpr_u32((uint32_t)b));
}

template <int ITEMS>
__device__ __forceinline__ void phase_b_load(const DevState& st, const ScanParams& sp, uint64_t t0, uint32_t tid,
                                             double (&v)[ITEMS], double (&mp)[ITEMS], uint32_t (&fl)[ITEMS])
{
    const uint64_t last = sp.n - 1;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const uint64_t i = t0 + (uint64_t)(r * kBlock + (int)tid);
        v[r] = st.w[(i < sp.n ? i : last)];
    }
    if (sp.phase_b) {
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const uint64_t i = t0 + (uint64_t)(r * kBlock + (int)tid);
            const uint64_t ic = i < sp.n ? i : last;
            fl[r] = st.flags[ic];
            mp[r] = st.mprob[ic];
        }
    }
}

// ctl: k_finalize's outputs (S, uniform, inv_n, f)
template <int ITEMS>
__device__ __forceinline__ void phase_b_apply(const DevState& st, const ScanParams& sp, const Ctl* ctl, uint64_t t0,
                                              uint32_t tid, double (&v)[ITEMS], const double (&mp)[ITEMS],
                                              const uint32_t (&fl)[ITEMS])
{
    // block-uniform values (the fused K3 reads them from LDS): kept in SGPRs
    const double S = sgpr_f64(ctl->S);
    const bool uniform = sgpr_u32(ctl->uniform) != 0;
    const double inv_n = sgpr_f64(ctl->inv_n);
    double f[DM_NBUCKETS];
#pragma unroll
    for (int b = 0; b < DM_NBUCKETS; ++b) f[b] = sgpr_f64(ctl->f[b]);
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const uint64_t i = t0 + (uint64_t)(r * kBlock + (int)tid);
        double x = v[r];
        if (sp.phase_b) {
            const uint32_t ncp = fl[r] & 0x7fu;
            const uint32_t bucket = ncp < DM_NBUCKETS - 1 ? ncp : DM_NBUCKETS - 1;
            double fb = f[0];
#pragma unroll
            for (int b = 1; b < DM_NBUCKETS; ++b) fb = (bucket == (uint32_t)b) ? f[b] : fb;
            const double factor = mp[r] * fb;
            x *= factor;
        }
        if (sp.normalize) x = uniform ? inv_n : x / S;
        if (i < sp.n) {
            if (sp.phase_b || sp.normalize) K1_ST(st.w + i, x);
        } else {
            x = 0.0;
        }
        v[r] = x;
    }
}

template <int ITEMS>
__device__ __forceinline__ void phase_b_tile(const DevState& st, const ScanParams& sp, const Ctl* ctl, uint64_t t0,
                                             uint32_t tid, double (&v)[ITEMS])
{
    double mp[ITEMS];
    uint32_t fl[ITEMS];
    phase_b_load<ITEMS>(st, sp, t0, tid, v, mp, fl);
    phase_b_apply<ITEMS>(st, sp, ctl, t0, tid, v, mp, fl);
}

// ---------------------------------------------------------------------------------------
// The fused finalize (one-GPU update step): block 0 of K3 runs k_finalize's block
// (finalize_block) and then publishes the launch's epoch in one word with an agent-scope
// release store; every block waits for that word (one lane polls, with a sleep) and copies
// the control block into LDS with agent-scope loads (its lines may be stale in this XCD's
// L2).  Block 0 is dispatched first and waits on nothing before it publishes, so the wait
// terminates; a bounded spin turns a violated assumption into ctl->err bit 2.  The epoch is
// a per-context launch counter: a word left by an earlier launch never equals it.
// ---------------------------------------------------------------------------------------
constexpr int kCtlWords = (int)(sizeof(Ctl) / 8);
static_assert(sizeof(Ctl) % 8 == 0 && kCtlWords <= 64, "the control block is copied by one wave");

// a cross-block wait gave up: poison the filter (kFaultTimeout in ctl->err, which every later
// launch checks, and in the host-mapped word the host checks before it trusts anything)
__device__ __forceinline__ void raise_timeout(Ctl* ctl, uint32_t* fault)
{
    atomicOr((unsigned long long*)&ctl->err, (unsigned long long)kFaultTimeout);
    if (fault) __hip_atomic_fetch_or(fault, kFaultTimeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// true (block-uniform) when the wait gave up: s_img is then not valid
__device__ __forceinline__ bool fin_wait_copy(Ctl* ctl, const uint64_t* fin_word, uint64_t epoch, uint64_t* s_img,
                                              const ScanParams& sp, uint32_t* s_flag)
{
    const uint32_t tid = threadIdx.x;
    if (tid < 64) {
        bool timeout = sp.spin_limit == 0;       // testing: give up at once
        if (tid == 0) {
            uint32_t spins = 0;
            // relaxed agent-scope polls and copies: on gfx950 an agent-scope atomic load reads
            // through this XCD's L2 to memory, where block 0's release store (a write-back of its
            // L2) has put the ctl lines.  Acquire loads (or an acquire fence) here invalidate
            // the L2 in every block: K3 53 -> 91 us at 4M, 18 -> 48 us at 256k (r03b).
            while (!timeout && atomic_load_agent(fin_word) != epoch) {
                if (spins++ >= sp.spin_limit) { timeout = true; break; }
                __builtin_amdgcn_s_sleep(8);
            }
            *s_flag = timeout ? 1u : 0u;
            if (timeout) raise_timeout(ctl, sp.fault);
        }
        // lane 0's verdict for the whole wave (the other lanes skip the copy's retry loop)
        timeout = __builtin_amdgcn_readfirstlane(timeout ? 1 : 0) != 0;
        // the copy must carry this launch's epoch (ctl->fin_epoch, written by block 0 before its
        // release): a stale copy of the line holding it would show an older one.  The relaxed
        // loads rely on gfx950's agent-scope loads missing this XCD's L2 for lines another XCD
        // wrote back.  Only the epoch's own 128-byte line is validated: were that assumption to
        // fail for another line of the block (resample, scan_shift, aborted sit in other lines),
        // this check would not see it -- it guards the common failure, not every one
        constexpr uint32_t kEpochWord = (uint32_t)(offsetof(Ctl, fin_epoch) / 8);
        if (!timeout) {
            uint64_t word = 0;
            for (int attempt = 0;; ++attempt) {
                if (tid < (uint32_t)kCtlWords) word = atomic_load_agent(reinterpret_cast<const uint64_t*>(ctl) + tid);
                if (!__any(tid == kEpochWord && word != epoch)) break;
                if (attempt == 64) {
                    if (tid == 0) { *s_flag = 1u; raise_timeout(ctl, sp.fault); }
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
            }
            if (tid < (uint32_t)kCtlWords) s_img[tid] = word;
        }
    }
    __syncthreads();
    return *s_flag != 0u;
}

// ---------------------------------------------------------------------------------------
// k_normalize_scan (K3a): phase B + normalisation and the tile totals; k_segments (K3b):
// the prefix of the fixed-point weights and the segment boundaries.  No cross-tile waiting
// inside a kernel: K3b re-sums the preceding tile totals (exact integers, any order).
// ---------------------------------------------------------------------------------------


// In-tile exclusive prefix of this thread's first item (thread -> wave -> block).
// run = this thread's total; s_wtot: kWaves words of LDS.
__device__ __forceinline__ uint64_t block_excl(uint64_t run, uint64_t* s_wtot)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t tincl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(tincl, o, 64);
        if ((int)lane >= o) tincl += t;
    }
    if (lane == 63) s_wtot[wave] = tincl;
    __syncthreads();
    uint64_t wexcl = 0;
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv)
        if ((uint32_t)wv < wave) wexcl += s_wtot[wv];
    return wexcl + (tincl - run);
}

// mark the segment [lo, hi) (outputs relative to this rank's slice) with value v
__device__ __forceinline__ void mark_segment(uint32_t* __restrict__ marks, uint32_t* __restrict__ tile_first,
                                             uint64_t lo, uint64_t hi, uint32_t v)
{
    marks[lo] = v;
    for (uint64_t t = (lo + kRow - 1) / kRow; t * kRow < hi; ++t) tile_first[t] = v - 1u;
}

// LDS staging of one scan tile: values in particle order, skewed by one slot every 32
// doubles so both the striped writes and the blocked (8 per thread) reads are conflict-free
constexpr int kSkew = 32;

__device__ __forceinline__ int skew(int k) { return k + k / kSkew; }

// this thread's 8 consecutive values (blocked) -> fixed-point inclusive running sums
template <int ITEMS>
__device__ __forceinline__ uint64_t blocked_fx(const double* s_v, int shift, uint64_t (&c)[ITEMS])
{
    uint64_t run = 0;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        run += fx_shift(s_v[skew((int)threadIdx.x * ITEMS + r)], shift);
        c[r] = run;
    }
    return run;
}

constexpr int kWaveChunks = 2;           // more draws than kWaveChunks * wave_draws: per-target windows

// stratified draws one wave holds in LDS at a time: its particles' share plus a row of slack
// (at least 576)
template <int ITEMS> constexpr int wave_draws() { return 64 * ITEMS + 64 > 576 ? 64 * ITEMS + 64 : 576; }

// the LDS slot of a wave's draw x, one pad slot per 8: a lane's window reads sit near draw
// 8 l + const (one target per particle, ITEMS = 8 particles per lane), and unpadded that stride
// of 8 doubles put lanes l and l + 4 on one bank (8-way within each 32-lane ds_read_b64 group);
// padded, the lanes' 8-byte reads cover the 64 banks once
__device__ __forceinline__ uint32_t draw_slot(uint32_t x) { return x + (x >> 3); }

// K3's LDS: the staged weights, then the wave's draws (the weights are dead before the
// draws are written)
template <int ITEMS> union K3Lds {
    double v[kBlock * ITEMS + kBlock * ITEMS / kSkew];
    uint64_t T[kWaves][wave_draws<ITEMS>() + wave_draws<ITEMS>() / 8];
    // the draws' minstd states (wave_counts' integer path): a wave's row is the first half of
    // its row of T, so a wave that falls back to T never touches another wave's states
    uint32_t X[kWaves][2 * (wave_draws<ITEMS>() + wave_draws<ITEMS>() / 8)];
};

// Write the marks of the tile's segment starts (relative to the slice) and the row carries
// of tile_first.  The marks buffer is all zero here (the gather clears every mark it
// reads), so only the segment starts are stored: direct stores measured ~1 µs faster per
// step than staging the tile's output range in LDS and writing it densely.
// seg_lo/seg_hi: this thread's segments (relative; empty when equal), val: their values.
template <int ITEMS>
__device__ __forceinline__ void flush_marks(uint32_t* __restrict__ marks, uint32_t* __restrict__ tile_first,
                                            const uint64_t (&seg_lo)[ITEMS], const uint64_t (&seg_hi)[ITEMS],
                                            const uint32_t (&val)[ITEMS])
{
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        const uint64_t lo = seg_lo[q], hi = seg_hi[q];
        if (hi <= lo) continue;
        marks[lo] = val[q];
        for (uint64_t t = (lo + kRow - 1) / kRow; t * kRow < hi; ++t) tile_first[t] = val[q] - 1u;
    }
}

// one segment's start mark and row carries (flush_marks for a single item)
__device__ __forceinline__ void flush_mark(uint32_t* __restrict__ marks, uint32_t* __restrict__ tile_first, uint64_t lo,
                                           uint64_t hi, uint32_t val)
{
    if (hi <= lo) return;
    marks[lo] = val;
    for (uint64_t t = (lo + kRow - 1) / kRow; t * kRow < hi; ++t) tile_first[t] = val - 1u;
}

constexpr uint64_t kPubMask = (1ull << 61) - 1;

// a tile's word into every replica (ScanParams::pub_stride), one lane each.  The sharded K3a
// writes every replica too (one thread): the words of a launch tag never outlive a launch in
// any copy, whichever kernel last wrote them
__device__ __forceinline__ void publish_tile(uint64_t* pub, uint32_t stride, uint32_t tile, uint64_t w)
{
    if (threadIdx.x < kPubReplicas) atomic_store_agent(pub + (uint64_t)threadIdx.x * stride + tile, w);
}
__device__ __forceinline__ void publish_tile_1(uint64_t* pub, uint32_t stride, uint32_t tile, uint64_t w)
{
#pragma unroll
    for (uint32_t r = 0; r < kPubReplicas; ++r) atomic_store_agent(pub + (uint64_t)r * stride + tile, w);
}

// sum of the published totals of tiles [0, count) (any order: exact integers).  Wave 0 reads
// them, 8 loads in flight per lane, and polls the unpublished ones with a sleep between
// polls (light on the memory system the tiles it waits for are still streaming through);
// the other waves wait at the barrier.
// A wait that gives up (sp.spin_limit polls) poisons the filter and returns ~0.
__device__ __forceinline__ uint64_t tiles_before_pub(const uint64_t* __restrict__ pub, uint32_t count, const ScanParams& sp,
                                                     uint64_t* s_red, Ctl* __restrict__ ctl)
{
    const uint32_t tag = sp.tag;
    const uint32_t tid = threadIdx.x;
    if (tid < 64) {
        uint64_t acc = 0;
        bool timeout = sp.spin_limit == 0 && count > 0;   // testing: give up at once
        for (uint32_t b0 = 0; !timeout && b0 < count; b0 += 8u * 64u) {
            uint64_t v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t k = b0 + (uint32_t)q * 64u + tid;
                v[q] = k < count ? atomic_load_agent(pub + k) : ((uint64_t)tag << 61);
            }
            uint32_t spins = 0;
            for (;;) {
                bool ready = true;
#pragma unroll
                for (int q = 0; q < 8; ++q) ready &= (uint32_t)(v[q] >> 61) == tag;
                if (__ballot(!ready) == 0ull) break;
                if (spins++ >= sp.spin_limit) { timeout = true; break; }
                __builtin_amdgcn_s_sleep(8);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const uint32_t k = b0 + (uint32_t)q * 64u + tid;
                    if ((uint32_t)(v[q] >> 61) != tag) v[q] = atomic_load_agent(pub + k);
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) acc += v[q] & kPubMask;
        }
        acc = wave_sum_u64(acc);
        if (tid == 0) s_red[0] = timeout ? ~0ull : acc;
        if (timeout && tid == 0) raise_timeout(ctl, sp.fault);
    }
    __syncthreads();
    return s_red[0];
}

// sum of the first `count` tile totals of a finished K3a (one block, coalesced, any order:
// exact integers; the words carry K3a's launch tag above bit 61)
__device__ __forceinline__ uint64_t tiles_before(const uint64_t* __restrict__ tile_sum, uint32_t count, uint64_t* s_wtot)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t acc = 0;
    for (uint32_t k = tid; k < count; k += kBlock) acc += tile_sum[k] & kPubMask;
    acc = wave_sum_u64(acc);
    if (lane == 0) s_wtot[wave] = acc;
    __syncthreads();
    uint64_t t = 0;
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv) t += s_wtot[wv];
    __syncthreads();                     // s_wtot is reused by the caller
    return t;
}

// K3a (multi-GPU): phase B + normalisation (striped, coalesced) and, when resampling, the
// tile's exact fixed-point weight total, published as tag << 61 | total like the one-GPU
// K3's words (every launch writes every word).  The last tile waits for the others' words
// and writes this slice's total (the value all-gathered before K3b), so no separate kernel
// sums the tiles; K3b re-sums the words before its own tile (any order: exact integers).
template <int ITEMS, bool FUSED>
__global__ void __launch_bounds__(kBlock) k_normalize_scan(DevState s0, DevState s1, ScanParams sp, Ctl* __restrict__ ctl,
                                                           uint64_t* __restrict__ tile_sum, uint64_t* __restrict__ total,
                                                           FusedFin ff)
{
    __shared__ uint64_t s_wtot[kWaves], s_red[kWaves];
    __shared__ uint64_t s_img[FUSED ? kCtlWords : 1];
    __shared__ uint32_t s_flag;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t tile = blockIdx.x;
    const uint64_t tagw = (uint64_t)sp.tag << 61;
    const bool last_tile = total && tile + 1 == sp.ntiles;
    if (ctl->err & kFaultTimeout) {      // poisoned: nothing is written (the waits of the other blocks end)
        if (tid == 0) {
            publish_tile_1(tile_sum, sp.pub_stride, tile, tagw);
            if (FUSED && tile == 0) __hip_atomic_store(ff.fin_word, ff.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            if (last_tile) *total = ~0ull;
        }
        return;
    }
    if constexpr (FUSED) {
        // the update step's finalize over every rank's statistics (block 0; the sharded
        // counterpart of k_normalize_segments' fused finalize)
        if (tile == 0) {
            __shared__ FinLds s_fin;
            finalize_block(ff.shards, ff.nrec, ctl, ff.fp, s_fin);
            __syncthreads();
            if (tid == 0) {
                ctl->fin_epoch = ff.epoch;       // ordered before the publication by the release
                __hip_atomic_store(ff.fin_word, ff.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    const Ctl* cv = FUSED ? reinterpret_cast<const Ctl*>(s_img) : ctl;
    const DevState st = (FUSED ? ctl->k3_base : ctl->base) ? s1 : s0;
    const uint64_t t0 = (uint64_t)tile * (kBlock * ITEMS);
    double v[ITEMS];
    if constexpr (FUSED) {
        double mp[ITEMS];
        uint32_t fl[ITEMS];
        phase_b_load<ITEMS>(st, sp, t0, tid, v, mp, fl);
        if (fin_wait_copy(ctl, ff.fin_word, ff.epoch, s_img, sp, &s_flag)) {
            if (tid == 0) {
                publish_tile_1(tile_sum, sp.pub_stride, tile, tagw);
                if (last_tile) *total = ~0ull;               // every rank sees the fault
            }
            return;
        }
        if (cv->aborted) {               // the update threw (k_finalize): weights stay as phase A left them
            if (tid == 0) publish_tile_1(tile_sum, sp.pub_stride, tile, tagw);
            return;
        }
        phase_b_apply<ITEMS>(st, sp, cv, t0, tid, v, mp, fl);
    } else {
        if (ctl->aborted) {              // the update threw (k_finalize): weights stay as phase A left them
            if (tid == 0) publish_tile_1(tile_sum, sp.pub_stride, tile, tagw);
            return;
        }
        phase_b_tile<ITEMS>(st, sp, ctl, t0, tid, v);
    }
    const bool resample = sgpr_u32(cv->resample) != 0;
    const int shift = (int)sgpr_u32((uint32_t)cv->scan_shift);
    uint64_t fx_sum = 0;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) fx_sum += fx_shift(v[r], shift);   // 0 past the end
    if (!resample) {
        if (tid == 0) publish_tile_1(tile_sum, sp.pub_stride, tile, tagw);
        return;
    }

    fx_sum = wave_sum_u64(fx_sum);
    if (lane == 0) s_wtot[wave] = fx_sum;
    __syncthreads();
    uint64_t t = 0;
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv) t += s_wtot[wv];
    if (tid == 0) publish_tile_1(tile_sum, sp.pub_stride, tile, tagw | (t & kPubMask));
    if (last_tile) {
        const uint64_t before = tiles_before_pub(tile_sum, tile, sp, s_red, ctl);
        if (tid == 0) *total = before == ~0ull ? ~0ull : before + t;     // ~0: every rank sees the fault
    }
}

// Draw counting (#{k : T_k <= C}) for the particles of one wave: the counts of its targets
// only read the draws [dlo, dhi) around floor(C N) of its first and last target.  Its lanes
// evaluate those draws in parallel, wave_draws at a time (lane l: k = q0 + l + 64 j, one jump
// then a 64-stride minstd step), store them in LDS, and every target reads the (at most
// three) draws of its window there.  No per-lane serial walk, no search, no divergence.
// Waves with more than kWaveChunks chunks of draws (heavy weights) evaluate each target's
// window directly (count_draws_le).
//
// count_draws_le with the draws read from LDS instead of evaluated.  The count of a target c
// is k0 = k* - 1 plus the leading draws among k0, k0 + 1, k0 + 2 (at most k* + 1, below N)
// that are <= c, k* = floor(c N) (draws below k0 are <= c, draws above k* + 1 are > c).
__device__ __forceinline__ uint64_t kstar_of(uint64_t c, uint64_t N, int shift)
{
    // c * N with N < 2^32 as two 32 x 32 -> 64 products: (hi << 32) + lo, and for shift >= 32
    // (the update path: 60) the shift needs only hi + (lo >> 32) (< 2^62, no carry out)
    if (shift >= 32) {
        const uint64_t lo = (uint64_t)(uint32_t)c * (uint32_t)N, hi = (c >> 32) * (uint64_t)(uint32_t)N;
        return (hi + (lo >> 32)) >> ((shift - 32) & 63);
    }
    return (uint64_t)(((unsigned __int128)c * N) >> shift);
}

// The window of target c as one word: bits 0..15 k0 - dlo (< kWaveChunks * wave_draws),
// 16..17 the number of window draws (k0 + d <= k* + 1, < N), bit 18 "k0 >= N" (count N),
// bits 19..21 set by draws_le_chunk: window draw d is <= c.
__device__ __forceinline__ uint32_t window_of(uint64_t c, uint64_t N, int shift, uint64_t dlo)
{
    const uint64_t kstar = kstar_of(c, N, shift);
    const uint64_t k0 = kstar >= 1 ? kstar - 1 : 0;
    if (k0 >= N) return 1u << 18;
    // draws k0 + d with k0 + d <= k* + 1 and k0 + d < N
    const uint64_t room = N - k0;
    uint32_t nd = kstar >= 1 ? 3u : 2u;
    nd = room < (uint64_t)nd ? (uint32_t)room : nd;
    return (uint32_t)(k0 - dlo) | (nd << 16);
}

// rq0, rq1: the LDS chunk [q0, q1) relative to dlo (u32: the wave's draws span < 2^16)
__device__ __forceinline__ uint32_t draws_le_chunk(uint32_t w, uint64_t c, const uint64_t* sT, uint32_t rq0, uint32_t rq1)
{
    const uint32_t r0 = w & 0xffffu;
    const uint32_t nd = (w >> 16) & 3u;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const uint32_t r = r0 + (uint32_t)d;
        const bool in = ((uint32_t)d < nd) & (r >= rq0) & (r < rq1);
        const uint64_t t = sT[draw_slot(in ? r - rq0 : 0u)];    // slot 0 is in LDS; used only when in
        w |= (in && t <= c) ? 1u << (19 + d) : 0u;
    }
    return w;
}

__device__ __forceinline__ uint64_t count_from_window(uint32_t w, uint64_t dlo, uint64_t N)
{
    if ((w >> 18) & 1u) return N;
    const uint64_t k0 = dlo + (w & 0xffffu);
    const uint32_t le = (w >> 19) & 7u;
    // leading draws <= c (draws are nondecreasing in k; le has no bits beyond nd)
    const uint32_t lead = (le & 1u) ? ((le & 2u) ? ((le & 4u) ? 3u : 2u) : 1u) : 0u;
    return k0 + lead;
}

// The counts #{k : T_k <= base + c[r]} of one wave's targets (hi_r) and, for the lane's
// first item, the count of its predecessor (lo: lane 0 #{T_k <= base}, the others the
// previous lane's last count).  The wave's cumulative range [wlo, whi] needs only the draws
// in [dlo, dhi) (the windows k* - 1 .. k* + 1 of wlo and whi, clamped to [0, N)): its lanes
// evaluate them in parallel into LDS (sT, wave_draws at a time) and every target reads the
// (at most three) draws of its window there.  Heavy weights (more than kWaveChunks chunks of
// draws): each target's window evaluated directly.
template <int ITEMS>
__device__ __forceinline__ void wave_counts_fp(uint64_t base, uint64_t run, const uint64_t (&c)[ITEMS], uint64_t N, int shift,
                                               uint32_t xs, const uint32_t* __restrict__ jt, uint64_t* sT,
                                               uint64_t (&hi_r)[ITEMS], uint64_t& lo)
{
    const uint32_t lane = threadIdx.x & 63u;
    const double dN = (double)N, inv_N = 1.0 / dN;
    // wave-uniform by construction: moved to SGPRs, so the window bounds, the loop and the
    // jump-ahead table reads of the first draw are scalar (readfirstlane returns int: each
    // half is widened as unsigned)
    auto rfl64 = [](uint64_t v) {
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
        const uint32_t lo_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
        return ((uint64_t)hi << 32) | (uint64_t)lo_;
    };
    const uint64_t wlo = rfl64(__shfl(base, 0, 64)), whi = rfl64(__shfl(base + run, 63, 64));
    const uint64_t ks_lo = kstar_of(wlo, N, shift), ks_hi = kstar_of(whi, N, shift);
    const uint64_t dlo = ks_lo >= 1 ? ks_lo - 1 : 0;
    const uint64_t dhi = ks_hi + 2 < N ? ks_hi + 2 : N;
    if (dlo >= dhi || dhi - dlo <= (uint64_t)kWaveChunks * wave_draws<ITEMS>()) {
        // le[r] bit d: draw k0_r + d of target r (r = ITEMS: wlo) is <= its target
        uint32_t win[ITEMS + 1];
#pragma unroll
        for (int r = 0; r <= ITEMS; ++r) win[r] = window_of(r < ITEMS ? base + c[r] : wlo, N, shift, dlo);
        const uint32_t a64 = jt[64], a_lane = jt[lane];            // A^64, A^lane
        for (uint64_t q0 = dlo; q0 < dhi; q0 += wave_draws<ITEMS>()) {
            const uint64_t q1 = dhi - q0 < (uint64_t)wave_draws<ITEMS>() ? dhi : q0 + wave_draws<ITEMS>();
            if (q0 + lane < q1) {
                uint32_t x = dm_mulmod31(dm_mulmod31(jump_pow(jt, q0 + 1), xs), a_lane);
#pragma unroll 4
                for (uint64_t k = q0 + lane; k < q1; k += 64) {
                    sT[draw_slot((uint32_t)(k - q0))] = draw_fx(k, x, dN, inv_N, shift);
                    x = dm_mulmod31(x, a64);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int r = 0; r <= ITEMS; ++r)
                win[r] = draws_le_chunk(win[r], r < ITEMS ? base + c[r] : wlo, sT, (uint32_t)(q0 - dlo),
                                        (uint32_t)(q1 - dlo));
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) hi_r[r] = count_from_window(win[r], dlo, N);
        const uint64_t K0 = count_from_window(win[ITEMS], dlo, N);
        const uint64_t prev = __shfl_up(hi_r[ITEMS - 1], 1, 64);
        lo = lane == 0 ? K0 : prev;
    } else {
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) hi_r[r] = count_draws_le(base + c[r], N, xs, shift, jt);
        const uint64_t K0 = count_draws_le(wlo, N, xs, shift, jt);
        const uint64_t prev = __shfl_up(hi_r[ITEMS - 1], 1, 64);
        lo = lane == 0 ? K0 : prev;
    }
}

// wave_counts_fp's results without evaluating a draw, when every target of the wave is decided
// by dm_draw_decide (eslam_detmath.h: the count of a decided target is k* + [T_k* <= c], what
// the three-draw window gives).  The wave stages only the minstd states x_k of its draws, one
// 32-bit word each, and a target reads the state of its k*.  Taken when the wave's draws fit
// one chunk and the shift is one the decision supports; a wave with an ambiguous target in any
// lane (a target within the rounding margin of a draw or of a stratum edge: equal weights
// k / N, the filter's last target) runs wave_counts_fp from its start instead.
template <int ITEMS>
__device__ __forceinline__ void wave_counts(uint64_t base, uint64_t run, const uint64_t (&c)[ITEMS], uint64_t N, int shift,
                                            uint32_t xs, const uint32_t* __restrict__ jt, uint64_t* sT, uint32_t* sX,
                                            uint64_t (&hi_r)[ITEMS], uint64_t& lo)
{
    // (N < 2^32 - 1 as everywhere in the draw counting: the context refuses larger filters)
    ESLAM_DRAW_WAVE(0);
    if (dm_draw_shift_ok(shift)) {                           // wave-uniform: the shift is scalar
        const uint32_t lane = threadIdx.x & 63u;
        auto rfl64 = [](uint64_t v) {
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
            const uint32_t lo_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
            return ((uint64_t)hi << 32) | (uint64_t)lo_;
        };
        const uint64_t wlo = rfl64(__shfl(base, 0, 64)), whi = rfl64(__shfl(base + run, 63, 64));
        const uint64_t ks_lo = kstar_of(wlo, N, shift), ks_hi = kstar_of(whi, N, shift);
        const uint64_t dlo = ks_lo >= 1 ? ks_lo - 1 : 0;
        const uint64_t dhi = ks_hi + 2 < N ? ks_hi + 2 : N;
        if (dlo < dhi && dhi - dlo <= (uint64_t)wave_draws<ITEMS>()) {
            if (dlo + lane < dhi) {
                const uint32_t a64 = jt[64];
                uint32_t x = dm_mulmod31(dm_mulmod31(jump_pow(jt, dlo + 1), xs), jt[lane]);
#pragma unroll 4
                for (uint64_t k = dlo + lane; k < dhi; k += 64) {
                    sX[draw_slot((uint32_t)(k - dlo))] = x;
                    x = dm_mulmod31(x, a64);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // every target lies in [wlo, whi], so its k* lies in [ks_lo, ks_hi], inside
            // [dlo, dhi) unless k* >= N (ambiguous: slot 0 read, not used)
            // (a decided target has k* < N < 2^32: 32-bit slots and counts)
            bool amb = false;
            uint32_t cnt[ITEMS + 1];
            const uint32_t span = (uint32_t)(dhi - dlo);
#pragma unroll
            for (int r = 0; r <= ITEMS; ++r) {
                uint64_t ks, rem;
                dm_draw_split(r < ITEMS ? base + c[r] : wlo, N, shift, &ks, &rem);
                const uint32_t rel = (uint32_t)ks - (uint32_t)dlo;
                const bool staged = rel < span;
                const uint32_t x = sX[draw_slot(staged ? rel : 0u)];
                const int d = dm_draw_decide(ks, rem, N, x, shift);
                amb |= !staged | (d < 0);
                cnt[r] = (uint32_t)ks + (d > 0 ? 1u : 0u);
            }
            if (__builtin_amdgcn_ballot_w64(amb) == 0) {
#pragma unroll
                for (int r = 0; r < ITEMS; ++r) hi_r[r] = cnt[r];
                const uint64_t prev = __shfl_up(hi_r[ITEMS - 1], 1, 64);
                lo = lane == 0 ? cnt[ITEMS] : prev;
                return;
            }
            // the states are read before wave_counts_fp stores draws over them
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    ESLAM_DRAW_WAVE(1);
    wave_counts_fp<ITEMS>(base, run, c, N, shift, xs, jt, sT, hi_r, lo);
}

// ---------------------------------------------------------------------------------------
// K3 (one GPU): phase B + normalisation, the tile's exact fixed-point total, the prefix of
// the preceding tiles and the segment marks, in one pass.  Each tile publishes its total as
// one 64-bit word, tag << 61 | total (fixed point < 2^61: the weights are normalised with
// shift 60, or scaled below 2^61 by k_finalize's shift for a standalone resample); the host
// cycles the tag per launch and every launch writes every tile's word, so a word still
// holding the previous launch's value never carries the current tag.  A tile sums its
// predecessors' words (exact integers, any order), waiting for those not yet published.
// The wait needs only that a tile's predecessors get scheduled: workgroups are dispatched in
// order (per XCD), and a predecessor publishes before it waits on anything itself.  A
// bounded spin turns a violated assumption into ctl->err bit 2 instead of a hang.
// ---------------------------------------------------------------------------------------

// 8 items: the 6 waves per SIMD the unfused kernel reaches by itself (<= 80 VGPRs; the fused
// one would take 86 and run at 5)
template <int ITEMS, bool FUSED>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ITEMS == 8 ? 6 : 1))) k_normalize_segments(DevState s0, DevState s1, ScanParams sp, Ctl* __restrict__ ctl,
                                                               uint64_t* __restrict__ tile_pub, uint32_t* __restrict__ marks,
                                                               uint32_t* __restrict__ tile_first,
                                                               const uint32_t* __restrict__ jt, FusedFin ff)
{
    __shared__ uint64_t s_wtot[kWaves], s_red[kWaves];
    __shared__ K3Lds<ITEMS> s_u;
    __shared__ uint64_t s_img[FUSED ? kCtlWords : 1];
    __shared__ uint32_t s_flag;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t tile = blockIdx.x;
    ESLAM_STAMP(g_stamps_k3, 0);
    const uint64_t tagw = (uint64_t)sp.tag << 61;
    if (ctl->err & kFaultTimeout) {      // poisoned: nothing is written (the waits of the other blocks end)
        if (tid == 0) {
            if (FUSED && tile == 0) __hip_atomic_store(ff.fin_word, ff.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
        publish_tile(tile_pub, sp.pub_stride, tile, tagw);
        return;
    }
    if constexpr (FUSED) {
        if (tile == 0) {
            __shared__ FinLds s_fin;
            finalize_block(ff.shards, ff.nrec, ctl, ff.fp, s_fin);
            __syncthreads();
            if (tid == 0) {
                ctl->fin_epoch = ff.epoch;       // ordered before the publication by the release
                __hip_atomic_store(ff.fin_word, ff.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    // the finalize's outputs: ctl itself (k_finalize ran before this launch), or its copy in
    // LDS once block 0 has published (fused)
    const Ctl* cv = FUSED ? reinterpret_cast<const Ctl*>(s_img) : ctl;
    // the buffer the weighting kernel wrote (= base after the finalize's commit)
    const DevState st = (FUSED ? ctl->k3_base : ctl->base) ? s1 : s0;
    const uint64_t t0 = (uint64_t)tile * (kBlock * ITEMS);
    bool resample = false;
    if constexpr (!FUSED) {
        if (cv->aborted) {               // the update threw (k_finalize): weights stay as phase A left them
            publish_tile(tile_pub, sp.pub_stride, tile, tagw);
            return;
        }
        resample = cv->resample != 0;
    }
    {
        // phase B + normalisation, striped (coalesced); the values are staged in LDS for the
        // blocked scan below.  Fused: the loads do not depend on the finalize, so they are
        // issued before its wait.
        double v[ITEMS];
        if constexpr (FUSED) {
            double mp[ITEMS];
            uint32_t fl[ITEMS];
            phase_b_load<ITEMS>(st, sp, t0, tid, v, mp, fl);
            ESLAM_STAMP(g_stamps_k3, 1);
            if (fin_wait_copy(ctl, ff.fin_word, ff.epoch, s_img, sp, &s_flag)) {
                publish_tile(tile_pub, sp.pub_stride, tile, tagw);
                return;
            }
            if (cv->aborted) {           // the update threw (k_finalize): weights stay as phase A left them
                publish_tile(tile_pub, sp.pub_stride, tile, tagw);
                return;
            }
            ESLAM_STAMP(g_stamps_k3, 2);
            phase_b_apply<ITEMS>(st, sp, cv, t0, tid, v, mp, fl);
            resample = sgpr_u32(cv->resample) != 0;
        } else {
            phase_b_tile<ITEMS>(st, sp, cv, t0, tid, v);
        }
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) s_u.v[skew(r * kBlock + (int)tid)] = v[r];
    }
    if (!resample) {
        publish_tile(tile_pub, sp.pub_stride, tile, tagw);
        return;
    }
    __syncthreads();
    ESLAM_STAMP(g_stamps_k3, 3);
    const int shift = (int)sgpr_u32((uint32_t)cv->scan_shift);
    uint64_t c[ITEMS];
    const uint64_t run = blocked_fx(s_u.v, shift, c);
    // in-tile exclusive prefix and the tile total (wave scans -> LDS)
    uint64_t tincl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(tincl, o, 64);
        if ((int)lane >= o) tincl += t;
    }
    if (lane == 63) s_wtot[wave] = tincl;
    __syncthreads();                     // (s_u.v is dead after it)
    uint64_t wexcl = 0, agg = 0;
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv) {
        const uint64_t t = s_wtot[wv];
        if ((uint32_t)wv < wave) wexcl += t;
        agg += t;
    }
    ESLAM_STAMP(g_stamps_k3, 4);
    publish_tile(tile_pub, sp.pub_stride, tile, tagw | (agg & kPubMask));
    const uint64_t tb = tiles_before_pub(tile_pub + (uint64_t)(tile % kPubReplicas) * sp.pub_stride, tile, sp, s_red, ctl);
    if (tb == ~0ull) return;             // gave up waiting: poisoned, no marks
    ESLAM_STAMP(g_stamps_k3, 5);
    const uint64_t base = tb + wexcl + (tincl - run);

    const uint64_t N = sp.n_global;
    const uint32_t xs = sgpr_u32(cv->minstd_start);
    const uint64_t i0 = t0 + (uint64_t)tid * ITEMS;
    uint64_t hi_r[ITEMS];
    uint64_t lo;
    wave_counts<ITEMS>(base, run, c, N, shift, xs, jt, s_u.T[wave], s_u.X[wave], hi_r, lo);
    ESLAM_STAMP(g_stamps_k3, 6);
    if (i0 == 0) lo = 0;
    // each item's segment [lo, hi) marked as it is found (no arrays of segments held)
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const uint64_t i = i0 + r;
        if (i < sp.n) {
            uint64_t hi = hi_r[r];
            if (i == N - 1) {
                if (hi < N) atomicAdd((unsigned long long*)&ctl->overruns, (unsigned long long)(N - hi));
                hi = N;
            }
            flush_mark(marks, tile_first, lo, hi, (uint32_t)(i + 1));
            lo = hi;
        }
    }
    ESLAM_STAMP(g_stamps_k3, 7);
}

// ---------------------------------------------------------------------------------------
// multi-GPU segments: the same scan, offset by the lower ranks' totals.  Outputs that land
// in this rank's slice [W0, W1) are marked directly (own particles never move); particles
// whose outputs reach another rank's slice record their range for k_pack.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void plan_bounds(const PlanParams& pp, const Ctl* ctl, const uint64_t* totals,
                                            const uint32_t* jt, uint64_t& off, uint64_t& O0, uint64_t& O1)
{
    off = 0;
    for (int r = 0; r < pp.rank; ++r) off += totals[r];
    const uint64_t N = pp.n_global;
    const uint32_t xs = ctl->minstd_start;
    const int shift = ctl->scan_shift;
    O0 = pp.rank == 0 ? 0 : count_draws_le(off, N, xs, shift, jt);
    O1 = pp.rank == pp.nranks - 1 ? N : count_draws_le(off + totals[pp.rank], N, xs, shift, jt);
}

__global__ void __launch_bounds__(kBlock) k_segments_multi(DevState s0, DevState s1, ScanParams sp, PlanParams pp,
                                                           Ctl* __restrict__ ctl, const uint64_t* __restrict__ tile_sum,
                                                           uint32_t* __restrict__ marks, uint32_t* __restrict__ tile_first,
                                                           const uint64_t* __restrict__ totals, const uint32_t* __restrict__ jt,
                                                           uint2* __restrict__ range, uint64_t* __restrict__ first_last,
                                                           uint64_t* host_out, uint64_t* host_epoch, uint64_t epoch)
{
    __shared__ uint64_t s_wtot[kWaves];
    __shared__ K3Lds<kScanItems> s_u;
    double* s_v = s_u.v;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the gathered totals and the finalize mirror (they follow the totals) to the host-mapped
        // buffer, then this launch's epoch: the host plans the exchange from them while the
        // kernel runs (no copy on the stream)
        for (int r = 0; r < pp.nranks; ++r) host_out[r] = totals[r];
        for (int q = 0; q < 3; ++q) host_out[kMaxRanks + q] = totals[kMaxRanks + q];
        __hip_atomic_store(host_epoch, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        // the chunks the next weighting launch may process before the exchange: all of them
        // without a resample (no gather pending), else those of the own outputs
        uint64_t c_lo = 0, c_hi = (pp.n_local + 64ull * pp.J - 1) / (64ull * pp.J);
        if (ctl->resample) {
            uint64_t off, O0, O1;
            plan_bounds(pp, ctl, totals, jt, off, O0, O1);
            own_chunks(O0, O1, pp.gbase[pp.rank], pp.n_local, pp.J, &c_lo, &c_hi);
        }
        pp.chunk_sel[0] = c_lo;
        pp.chunk_sel[1] = c_hi;
    }
    if (!ctl->resample) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const DevState st = ctl->base ? s1 : s0;
    const uint64_t t0 = (uint64_t)tile * kScanTile;
#pragma unroll
    for (int r = 0; r < kScanItems; ++r) {
        const int k = r * kBlock + (int)tid;
        const uint64_t i = t0 + (uint64_t)k;
        s_v[skew(k)] = i < sp.n ? st.w[i] : 0.0;
    }
    __syncthreads();
    const int shift = ctl->scan_shift;
    uint64_t c[kScanItems];
    const uint64_t run = blocked_fx<kScanItems>(s_v, shift, c);
    const uint64_t tbase = tiles_before(tile_sum, tile, s_wtot) + block_excl(run, s_wtot);
    uint64_t off, O0, O1;
    plan_bounds(pp, ctl, totals, jt, off, O0, O1);
    const uint64_t base = off + tbase;
    const uint64_t N = pp.n_global;
    const uint64_t W0 = pp.gbase[pp.rank], W1 = pp.gbase[pp.rank + 1];
    const uint64_t i0 = t0 + (uint64_t)tid * kScanItems;
    uint64_t hi_r[kScanItems];
    uint64_t lo;
    wave_counts<kScanItems>(base, run, c, N, shift, ctl->minstd_start, jt, s_u.T[tid >> 6], s_u.X[tid >> 6], hi_r, lo);
    if (i0 == 0) lo = O0;
    uint64_t seg_lo[kScanItems], seg_hi[kScanItems];
    uint32_t val[kScanItems];
#pragma unroll
    for (int r = 0; r < kScanItems; ++r) {
        const uint64_t i = i0 + r;
        seg_lo[r] = seg_hi[r] = 0;
        val[r] = kMarkOwn + 1u + (uint32_t)i;
        if (i >= sp.n) continue;
        uint64_t hi = hi_r[r];
        if (i + 1 == sp.n) {
            if (pp.rank == pp.nranks - 1 && hi < N)
                atomicAdd((unsigned long long*)&ctl->overruns, (unsigned long long)(N - hi));
            hi = O1;
        }
        const uint64_t a = lo > W0 ? lo : W0, b = hi < W1 ? hi : W1;
        if (a < b) { seg_lo[r] = a - W0; seg_hi[r] = b - W0; }
        // every particle a foreign destination's [first, last] run can include (empty
        // ranges too) has lo < W0 or hi > W1: record its range for k_pack
        if (lo < W0 || hi > W1) {
            range[i] = make_uint2((uint32_t)lo, (uint32_t)hi);
            if (hi > lo) {
                for (int d = 0; d < pp.nranks; ++d) {
                    if (d == pp.rank) continue;
                    const uint64_t Wd0 = pp.gbase[d], Wd1 = pp.gbase[d + 1];
                    const uint64_t Sd = O0 > Wd0 ? O0 : Wd0, Ed = O1 < Wd1 ? O1 : Wd1;
                    if (Sd >= Ed) continue;
                    if (lo <= Sd && Sd < hi) first_last[2 * d] = i;
                    if (lo <= Ed - 1 && Ed - 1 < hi) first_last[2 * d + 1] = i;
                }
            }
        }
        lo = hi;
    }
    flush_marks(marks, tile_first, seg_lo, seg_hi, val);
}

// one record per output of this rank that lands in another slice: send slot j of
// destination d is output k = sd[d] + (j - send_off[d]); its source is the particle of
// [first, last] (d's run, from k_segments_multi) whose range [lo, hi) contains k
__global__ void __launch_bounds__(kBlock) k_pack(DevState s0, DevState s1, const Ctl* __restrict__ ctl, PlanParams pp,
                                                 const uint2* __restrict__ range, const uint64_t* __restrict__ first_last,
                                                 Rec* __restrict__ send)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= pp.send_off[pp.nranks]) return;
    int d = 0;
    while (j >= pp.send_off[d + 1]) ++d;
    const uint64_t k = pp.sd[d] + (j - pp.send_off[d]);
    uint64_t a = first_last[2 * d], b = first_last[2 * d + 1];   // range[a].x <= k < range[b].y
    while (a < b) {                                               // last i in [a, b] with lo_i <= k
        const uint64_t mid = a + (b - a + 1) / 2;
        if ((uint64_t)range[mid].x <= k) a = mid;
        else b = mid - 1;
    }
    const uint64_t i = a;
    const DevState st = ctl->base ? s1 : s0;
    Rec r;
    r.x = st.x[i]; r.y = st.y[i]; r.th = st.th[i]; r.z = st.z[i]; r.zs = st.zs[i]; r.w = st.w[i]; r.mprob = st.mprob[i];
    r.lohi = k | ((k + 1) << 32);
    r.src = (uint64_t)st.flags[i] | ((pp.gbase[pp.rank] + i) << 8);
    send[j] = r;
}

// records -> marks (lower ranks: 1 + j, higher ranks: kMarkHigh + 1 + j)
__global__ void __launch_bounds__(kBlock) k_expand(const Rec* __restrict__ recv, uint64_t nrecv, uint64_t W0,
                                                   uint32_t* __restrict__ marks, uint32_t* __restrict__ tile_first)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nrecv) return;
    const Rec& r = recv[j];
    const uint64_t glo = r.lohi & 0xffffffffull, ghi = r.lohi >> 32;
    if (ghi > glo) {
        const uint32_t v = ((r.src >> 8) < W0 ? 1u : kMarkHigh + 1u) + (uint32_t)j;
        mark_segment(marks, tile_first, glo - W0, ghi - W0, v);
    }
}

// ---------------------------------------------------------------------------------------
// k_resample_gather: materialise a pending resample gather (xi_k.swap(xi_kp),
// src/ParticleFilter.hpp:107) before the state is read by anything but the next
// k_project_weight, which gathers on the fly.  Weights are carried, not reset (Q4).
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_resample_gather(DevState s0, DevState s1, uint64_t n, uint64_t gbase,
                                                            Ctl* __restrict__ ctl, GatherView gv, uint32_t aux)
{
    if (!ctl->gather) return;
    __shared__ uint32_t s_wmax[kWaves];
    __shared__ uint32_t s_idx[kGatherTile];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t t = blockIdx.x;
    const DevState in = ctl->base ? s1 : s0;
    const DevState out = ctl->base ? s0 : s1;
    const uint64_t k0 = (uint64_t)t * kGatherTile + (uint64_t)tid * kScanItems;
    uint32_t mk[kScanItems];
    uint32_t run = 0;
#pragma unroll
    for (int r = 0; r < kScanItems; ++r) {
        const uint64_t k = k0 + r;
        uint32_t v = 0;
        if (k < n) { v = gv.marks[k]; if (v) gv.marks[k] = 0; }
        run = run > v ? run : v;
        mk[r] = run;
    }
    const uint32_t tincl = wave_incl_max_u32(run);
    if (lane == 63) s_wmax[wave] = tincl;
    __syncthreads();
    uint32_t carry = gv.row_first[(uint64_t)t * (kGatherTile / kRow)] + 1u;
    for (uint32_t wv = 0; wv < wave; ++wv) carry = carry > s_wmax[wv] ? carry : s_wmax[wv];
    uint32_t texcl = __shfl_up(tincl, 1, 64);
    if (lane == 0) texcl = 0;
    carry = carry > texcl ? carry : texcl;
#pragma unroll
    for (int r = 0; r < kScanItems; ++r) {
        const uint32_t v = mk[r] > carry ? mk[r] : carry;
        s_idx[tid * kScanItems + r] = v - 1u;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kScanItems; ++r) {
        const uint32_t slot = (uint32_t)r * kBlock + tid;
        const uint64_t k = (uint64_t)t * kGatherTile + slot;
        if (k >= n) continue;
        const gmem<const Rec>* rc;
        const uint32_t i = decode_source(s_idx[slot], gv.multi, (const gmem<const Rec>*)gv.recs, &rc);
        if (rc) {
            out.x[k] = rc->x; out.y[k] = rc->y; out.th[k] = rc->th; out.z[k] = rc->z; out.zs[k] = rc->zs; out.w[k] = rc->w;
            if (aux) { out.mprob[k] = rc->mprob; out.flags[k] = (uint8_t)rc->src; }
            if (gv.record) gv.anc[k] = (uint32_t)(rc->src >> 8);
            if (in.sid) out.sid[k] = kSidRecord | (uint32_t)(rc - (const gmem<const Rec>*)gv.recs);   // store: the record's
            continue;
        }
        out.x[k] = in.x[i];
        out.y[k] = in.y[i];
        out.th[k] = in.th[i];
        out.z[k] = in.z[i];
        out.zs[k] = in.zs[i];
        out.w[k] = in.w[i];
        if (aux) {
            out.mprob[k] = in.mprob[i];
            out.flags[k] = in.flags[i];
        }
        if (in.sid) out.sid[k] = in.sid[i];            // per-particle maps: the store's name
        if (gv.record) gv.anc[k] = (uint32_t)(gbase + i);
    }
}

// commit a consumed gather / flip outside an update (after a project-only step or a
// materialising gather): the latest state becomes state[base]
__global__ void k_commit(Ctl* __restrict__ ctl)
{
    if (threadIdx.x == 0) {
        ctl->base ^= ctl->flip;
        ctl->flip = 0;
        ctl->gather = 0;
    }
}

// ---------------------------------------------------------------------------------------
// PoseEstimator::init(N, mu, sigma, zpos, zsigma): samplePose2D per particle
// (src/PoseEstimator.cpp:64-73, 88-102) from the INIT Philox stream.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_init_gaussian(DevState s0, uint64_t n, uint64_t gbase, uint64_t seed, uint64_t ev,
                                                          double mx, double my, double mt, double sx, double sy, double stt,
                                                          double zpos, double zsigma)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t gi = gbase + i;
    const dm_philox_ctr d0 = dm_draw(seed, DM_STREAM_INIT, ev, gi, 0);
    double n0, n1, n2, n3;
    dm_box_muller32(d0.v[0], d0.v[1], &n0, &n1);
    dm_box_muller32(d0.v[2], d0.v[3], &n2, &n3);
    s0.x[i] = n0 * sx + mx;
    s0.y[i] = n1 * sy + my;
    s0.th[i] = n2 * stt + mt;
    s0.z[i] = zpos;
    s0.zs[i] = zsigma;
    s0.w[i] = 0.0;
    s0.mprob[i] = 0.0;
    s0.flags[i] = 0x80u;   // floating = true, no contact points
}

// ---------------------------------------------------------------------------------------
// ParticleFilter::getBestParticleIndex (src/ParticleFilter.hpp:160-173): first index of the
// maximum weight; NaN never compares greater, and -0 == +0 (the reference's `weight > best`):
// the zero's sign is dropped before the ordered key.  out[0] = max ordered key, out[1] = index.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_best_max(DevState s0, DevState s1, uint64_t n, const Ctl* __restrict__ ctl,
                                                     uint64_t* out)
{
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    uint64_t best = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        double w = st.w[i];
        if (w == 0.0) w = 0.0;
        if (w == w) { const uint64_t k = order_key(w); best = best > k ? best : k; }
    }
    for (int o = 32; o >= 1; o >>= 1) { const uint64_t t = __shfl_xor(best, o, 64); best = best > t ? best : t; }
    if ((threadIdx.x & 63u) == 0 && best) atomicMax((unsigned long long*)&out[0], (unsigned long long)best);
}

__global__ void __launch_bounds__(kBlock) k_best_index(DevState s0, DevState s1, uint64_t n, const Ctl* __restrict__ ctl,
                                                       uint64_t* out)
{
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    const uint64_t key = out[0];
    uint64_t idx = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        double w = st.w[i];
        if (w == 0.0) w = 0.0;
        if (w == w && order_key(w) == key) { idx = i < idx ? i : idx; break; }
    }
    for (int o = 32; o >= 1; o >>= 1) { const uint64_t t = __shfl_xor(idx, o, 64); idx = idx < t ? idx : t; }
    if ((threadIdx.x & 63u) == 0 && idx != ~0ull) atomicMin((unsigned long long*)&out[1], (unsigned long long)idx);
}

// ---------------------------------------------------------------------------------------
// PoseEstimator::getCentroid sums (src/PoseEstimator.cpp:354-383): x w, y w, theta w, z w, w
// in the canonical chunk order, then a fixed pairwise tree over the chunk totals.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_centroid_chunks(DevState s0, DevState s1, uint64_t n, uint32_t J,
                                                            const Ctl* __restrict__ ctl, double* __restrict__ chunk_out)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t chunk = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t lbase = chunk * 64ull * J;
    if (lbase >= n) return;
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t j = 0; j < J; ++j) {
        const uint64_t i = lbase + 64ull * j + lane;
        if (i >= n) continue;
        const double w = st.w[i];
        a[0] = a[0] + st.x[i] * w;
        a[1] = a[1] + st.y[i] * w;
        a[2] = a[2] + st.th[i] * w;
        a[3] = a[3] + st.z[i] * w;
        a[4] = a[4] + w;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const double v = wave_sum_butterfly(a[q]);
        if (lane == 0) chunk_out[chunk * 5 + q] = v;
    }
}

// one level of the fixed pairwise tree: dst[i] = src[2i] + src[2i+1]; odd tail moves up
__global__ void __launch_bounds__(kBlock) k_tree_level(const double* __restrict__ src, double* __restrict__ dst, uint64_t m)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t h = m / 2;
    if (i > h || (i == h && !(m & 1))) return;
    for (int q = 0; q < 5; ++q)
        dst[i * 5 + q] = i < h ? src[(2 * i) * 5 + q] + src[(2 * i + 1) * 5 + q] : src[(m - 1) * 5 + q];
}

}  // namespace eslam_dev

// ---------------------------------------------------------------------------------------
// launchers (called by eslam_ctx.hip)
// ---------------------------------------------------------------------------------------
using namespace eslam_dev;

// One canonical chunk per wave (dm_chunk_rows sizes the chunks so that there are ~16k of
// them from 1M particles on).  A persistent grid striding over chunks was measured slower:
// its loop state spills SGPRs, and the LDS window it saves is staged from L2 anyway.
static uint32_t k1_grid(uint64_t chunks) { return (uint32_t)((chunks + kWaves - 1) / kWaves); }

extern "C" hipError_t eslam_launch_project_weight(int project, int weight, int maxp, DevState s0, DevState s1,
                                                  const MapView* map, const StepParams* p, Ctl* ctl, Shard* shards,
                                                  const GatherView* gv, const LocalMaps* store, hipStream_t stream,
                                                  const ChunkSel* sel, double* bspill)
{
    const uint64_t csz = 64ull * p->J;
    uint64_t chunks = (p->n + csz - 1) / csz;
    if (sel && sel->mode == 2u) chunks = sel->c_lo + (chunks > sel->c_hi ? chunks - sel->c_hi : 0);   // the edge chunks
    if (chunks == 0) return hipSuccess;
    const size_t lds = kStatsLds + (weight ? kWindowLds : (project && ESLAM_K1_BM_LDS ? kBmLds : 0));
    K1Args args;
    args.p = *p;
    args.map = *map;
    args.gv = *gv;
    args.s[0] = s0;
    args.s[1] = s1;
    args.ctl = ctl;
    args.shards = shards;
    memset(&args.store, 0, sizeof(args.store));
    if (store) args.store = *store;
    memset(&args.sel, 0, sizeof(args.sel));
    if (sel) args.sel = *sel;
    args.bspill = bspill;
    if (weight && !bspill) return hipErrorInvalidValue;
#define ESLAM_LAUNCH(P, W, M, B, ...)                                                                   \
    hipLaunchKernelGGL((k_project_weight<P, W, M, B, ##__VA_ARGS__>), dim3(k1_grid(chunks)), dim3(kBlock), lds, \
                       stream, args)
    // every contact closes its group (groupId -1 or groups of one): the reduced group logic
    const uint32_t all = p->m >= 32 ? 0xffffffffu : ((1u << p->m) - 1u);
    const bool ung = (p->end_mask & all) == all;
    if (weight && store) {
        // per-particle maps: the lookups fall back to the particle's store (every pending
        // gather has been materialised by the host)
        if (p->m <= 4 && maxp <= 4) {
            if (project) { if (ung) ESLAM_LAUNCH(true, true, 4, true, true, true); else ESLAM_LAUNCH(true, true, 4, true, true); }
            else { if (ung) ESLAM_LAUNCH(false, true, 4, true, true, true); else ESLAM_LAUNCH(false, true, 4, true, true); }
        } else {
            if (project) ESLAM_LAUNCH(true, true, ESLAM_MAX_CONTACTS, false, true);
            else ESLAM_LAUNCH(false, true, ESLAM_MAX_CONTACTS, false, true);
        }
        return hipGetLastError();
    }
    // batched contact lookups when every contact fits the MAXP-sized arrays
    if (project && !weight) ESLAM_LAUNCH(true, false, 4, false);
    else if (!project && weight) {
        if (maxp <= 4) {
            if (p->m <= 4) { if (ung) ESLAM_LAUNCH(false, true, 4, true, false, true); else ESLAM_LAUNCH(false, true, 4, true); }
            else ESLAM_LAUNCH(false, true, 4, false);
        }
        else if (maxp <= 8) { if (p->m <= 8) ESLAM_LAUNCH(false, true, 8, true); else ESLAM_LAUNCH(false, true, 8, false); }
        else ESLAM_LAUNCH(false, true, ESLAM_MAX_CONTACTS, false);
    } else {
        if (maxp <= 4) {
            if (p->m <= 4) { if (ung) ESLAM_LAUNCH(true, true, 4, true, false, true); else ESLAM_LAUNCH(true, true, 4, true); }
            else ESLAM_LAUNCH(true, true, 4, false);
        }
        else if (maxp <= 8) { if (p->m <= 8) ESLAM_LAUNCH(true, true, 8, true); else ESLAM_LAUNCH(true, true, 8, false); }
        else ESLAM_LAUNCH(true, true, ESLAM_MAX_CONTACTS, false);
    }
#undef ESLAM_LAUNCH
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_contact_records(DevState s0, DevState s1, const MapView* map, const StepParams* p, Ctl* ctl,
                                                   const DebugRec* d, const LocalMaps* store, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)((p->n + kBlock - 1) / kBlock);
    if (!blocks) return hipSuccess;
    K1Args args;
    memset(&args, 0, sizeof(args));
    args.p = *p;
    args.map = *map;
    args.s[0] = s0;
    args.s[1] = s1;
    args.ctl = ctl;
    if (store) args.store = *store;
    if (s0.sid) hipLaunchKernelGGL(k_contact_records<true>, dim3(blocks), dim3(kBlock), 16, stream, args, *d);
    else hipLaunchKernelGGL(k_contact_records<false>, dim3(blocks), dim3(kBlock), 16, stream, args, *d);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_pack_records(DevState s0, DevState s1, const Ctl* ctl, uint64_t first, uint64_t stride,
                                                uint64_t count, uint64_t gbase, const uint32_t* anc, const DebugRec* d, eslam_particle_record* out, eslam_cpoint* cps,
                                                uint32_t max_cp, const uint64_t* slot, const double* remote, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)((count + kBlock - 1) / kBlock);
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(k_pack_records, dim3(blocks), dim3(kBlock), 0, stream, s0, s1, ctl, first, stride, count, gbase, anc,
                       *d, out, cps, max_cp, slot, remote);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_gather_records(const uint32_t* req, uint64_t nreq, uint64_t gbase, const DebugRec* d,
                                                  double* items, hipStream_t stream)
{
    const uint64_t blocks = (nreq + kBlock - 1) / kBlock;
    if (blocks) hipLaunchKernelGGL(k_gather_records, dim3((uint32_t)blocks), dim3(kBlock), 0, stream, req, nreq, gbase, *d, items);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_scan_excl(uint32_t* a, uint64_t m, hipStream_t stream)
{
    if (m) hipLaunchKernelGGL(k_scan_excl, dim3(1), dim3(1024), 0, stream, a, m);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_weight_stats(DevState s0, DevState s1, uint64_t n, uint32_t J, Ctl* ctl, Shard* shards,
                                                hipStream_t stream)
{
    const uint64_t csz = 64ull * J;
    const uint64_t chunks = (n + csz - 1) / csz;
    const uint32_t blocks = (uint32_t)((chunks + kWaves - 1) / kWaves);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_weight_stats, dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, J, ctl, shards);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_finalize(Shard* recs, int nrec, Ctl* ctl, const FinParams* fp, hipStream_t stream)
{
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(kBlock), 0, stream, recs, nrec, ctl, *fp);
    return hipGetLastError();
}

// ff: the update step's finalize fused into block 0 (nullptr: k_finalize ran before)
extern "C" hipError_t eslam_launch_normalize_scan(DevState s0, DevState s1, const ScanParams* sp, Ctl* ctl, uint64_t* tile_sum,
                                                  uint64_t* total, const FusedFin* ff, hipStream_t stream)
{
    if (sp->ntiles == 0) return hipSuccess;
    if (sp->tag < 1 || sp->tag > 7) return hipErrorInvalidValue;
    FusedFin none;
    memset(&none, 0, sizeof(none));
    const FusedFin& f = ff ? *ff : none;
#define ESLAM_K3A(I)                                                                                                  \
    do {                                                                                                              \
        if (ff) hipLaunchKernelGGL((k_normalize_scan<I, true>), dim3(sp->ntiles), dim3(kBlock), 0, stream, s0, s1, *sp, \
                                   ctl, tile_sum, total, f);                                                          \
        else hipLaunchKernelGGL((k_normalize_scan<I, false>), dim3(sp->ntiles), dim3(kBlock), 0, stream, s0, s1, *sp,   \
                                ctl, tile_sum, total, f);                                                             \
    } while (0)
    switch (sp->items) {
    case 2: ESLAM_K3A(2); break;
    case 4: ESLAM_K3A(4); break;
    case kScanItems: ESLAM_K3A(kScanItems); break;
    default: return hipErrorInvalidValue;
    }
#undef ESLAM_K3A
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_normalize_segments(DevState s0, DevState s1, const ScanParams* sp, Ctl* ctl,
                                                      uint64_t* tile_pub, uint32_t* marks, uint32_t* tile_first,
                                                      const uint32_t* jt, const FusedFin* ff, hipStream_t stream)
{
    if (sp->ntiles == 0) return hipSuccess;
    if (sp->tag < 1 || sp->tag > 7) return hipErrorInvalidValue;
    if (ff && (!ff->shards || !ff->fin_word || ff->fp.mode != FIN_UPDATE || ff->fp.mirror)) return hipErrorInvalidValue;
    const FusedFin none{};
#define ESLAM_SEG(I) do { \
        if (ff) hipLaunchKernelGGL((k_normalize_segments<I, true>), dim3(sp->ntiles), dim3(kBlock), 0, stream, s0, s1, *sp, ctl, \
                                   tile_pub, marks, tile_first, jt, *ff); \
        else hipLaunchKernelGGL((k_normalize_segments<I, false>), dim3(sp->ntiles), dim3(kBlock), 0, stream, s0, s1, *sp, ctl, \
                                tile_pub, marks, tile_first, jt, none); \
    } while (0)
    switch (sp->items) {
    case 1: ESLAM_SEG(1); break;
    case 2: ESLAM_SEG(2); break;
    case 4: ESLAM_SEG(4); break;
    case 8: ESLAM_SEG(8); break;
    default: return hipErrorInvalidValue;
    }
#undef ESLAM_SEG
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_resample_gather(DevState s0, DevState s1, uint64_t n, uint64_t gbase, Ctl* ctl,
                                                   const GatherView* gv, uint32_t aux, hipStream_t stream)
{
    const uint32_t tiles = (uint32_t)((n + kGatherTile - 1) / kGatherTile);
    if (tiles) hipLaunchKernelGGL(k_resample_gather, dim3(tiles), dim3(kBlock), 0, stream, s0, s1, n, gbase, ctl, *gv, aux);
    hipLaunchKernelGGL(k_commit, dim3(1), dim3(64), 0, stream, ctl);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_commit(Ctl* ctl, hipStream_t stream)
{
    hipLaunchKernelGGL(k_commit, dim3(1), dim3(64), 0, stream, ctl);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_segments_multi(DevState s0, DevState s1, const ScanParams* sp, const PlanParams* pp, Ctl* ctl,
                                                  const uint64_t* tile_prefix, uint32_t* marks, uint32_t* tile_first,
                                                  const uint64_t* totals, const uint32_t* jt, uint2* range, uint64_t* first_last,
                                                  uint64_t* host_out, uint64_t* host_epoch, uint64_t epoch, hipStream_t stream)
{
    if (sp->items != kScanItems) return hipErrorInvalidValue;       // the sharded scan uses full tiles
    if (sp->ntiles) hipLaunchKernelGGL(k_segments_multi, dim3(sp->ntiles), dim3(kBlock), 0, stream, s0, s1, *sp, *pp, ctl,
                                       tile_prefix, marks, tile_first, totals, jt, range, first_last, host_out, host_epoch,
                                       epoch);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_pack(DevState s0, DevState s1, Ctl* ctl, const PlanParams* pp, const uint2* range,
                                        const uint64_t* first_last, uint64_t nsend, void* send, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)((nsend + kBlock - 1) / kBlock);
    if (blocks)
        hipLaunchKernelGGL(k_pack, dim3(blocks), dim3(kBlock), 0, stream, s0, s1, ctl, *pp, range, first_last, (Rec*)send);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_expand(const void* recv, uint64_t nrecv, uint64_t W0, uint32_t* marks, uint32_t* row_first,
                                          hipStream_t stream)
{
    if (nrecv) hipLaunchKernelGGL(k_expand, dim3((uint32_t)((nrecv + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                                  (const Rec*)recv, nrecv, W0, marks, row_first);
    return hipGetLastError();
}

extern "C" uint64_t eslam_record_bytes(void) { return sizeof(Rec); }

extern "C" hipError_t eslam_launch_init_gaussian(DevState s0, uint64_t n, uint64_t gbase, uint64_t seed, uint64_t ev,
                                                 const double mu[3], const double sigma[3], double zpos, double zsigma,
                                                 hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)((n + kBlock - 1) / kBlock);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_init_gaussian, dim3(blocks), dim3(kBlock), 0, stream, s0, n, gbase, seed, ev, mu[0], mu[1], mu[2],
                       sigma[0], sigma[1], sigma[2], zpos, zsigma);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_best_index(DevState s0, DevState s1, uint64_t n, Ctl* ctl, uint64_t* out2,
                                              hipStream_t stream)
{
    const uint64_t init[2] = {0ull, ~0ull};
    hipError_t e = hipMemcpyAsync(out2, init, 16, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    uint32_t blocks = (uint32_t)((n + kBlock - 1) / kBlock);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_best_max, dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, ctl, out2);
    hipLaunchKernelGGL(k_best_index, dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, ctl, out2);
    return hipGetLastError();
}

// the fixed pairwise tree over m chunk records of 5 doubles at a (b: scratch of the same
// size; both are overwritten); the total goes to out
static hipError_t centroid_tree(double* a, double* b, uint64_t m, double* out, hipStream_t stream)
{
    while (m > 1) {
        const uint64_t m2 = (m + 1) / 2;
        hipLaunchKernelGGL(k_tree_level, dim3((uint32_t)((m2 + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, a, b, m);
        double* t = a; a = b; b = t;
        m = m2;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, a, 5 * sizeof(double), hipMemcpyDeviceToDevice, stream);
    return e;
}

// per canonical chunk (64 x J particles) of this context: sum x w, y w, theta w, z w, w
extern "C" hipError_t eslam_launch_centroid_chunks(DevState s0, DevState s1, uint64_t n, uint32_t J, Ctl* ctl,
                                                   double* chunk_out, hipStream_t stream)
{
    const uint64_t csz = 64ull * J;
    const uint64_t chunks = (n + csz - 1) / csz;
    const uint32_t blocks = (uint32_t)((chunks + kWaves - 1) / kWaves);
    if (blocks) hipLaunchKernelGGL(k_centroid_chunks, dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, J, ctl, chunk_out);
    return hipGetLastError();
}

// sharded getCentroid: the tree over the all-gathered chunk records (m chunks at a, b scratch)
extern "C" hipError_t eslam_launch_centroid_tree(double* a, double* b, uint64_t m, double* out, hipStream_t stream)
{
    if (m == 0) return hipMemsetAsync(out, 0, 5 * sizeof(double), stream);
    return centroid_tree(a, b, m, out, stream);
}

// tmp: the caller's scratch of 2 x max(chunks, 1) x 5 doubles (the chunk records and the tree's
// second level).  It belongs to the context: stream-ordered pool memory here gave the second of
// two contexts of one process, each on its own stream, another centroid than the first for the
// same particles (the block one stream had freed was handed to the other).
extern "C" hipError_t eslam_launch_centroid(DevState s0, DevState s1, uint64_t n, uint32_t J, Ctl* ctl, double* tmp, double* out,
                                            hipStream_t stream)
{
    const uint64_t csz = 64ull * J;
    const uint64_t chunks = (n + csz - 1) / csz;
    const uint64_t cap = chunks ? chunks : 1;
    double* a = tmp;
    double* b = tmp + cap * 5;
    hipError_t e = hipMemsetAsync(a, 0, 5 * sizeof(double), stream);
    if (e == hipSuccess) e = eslam_launch_centroid_chunks(s0, s1, n, J, ctl, a, stream);
    if (e == hipSuccess) e = centroid_tree(a, b, chunks, out, stream);
    return e;
}

// blocks per CU of the main K1 instantiation (diagnostics)
extern "C" int eslam_debug_k1_occupancy(int* blocks_per_cu, int lds)
{
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_project_weight<true, true, 4, true>, kBlock,
                                                        lds < 0 ? kStatsLds + kWindowLds : lds) == hipSuccess ? 0 : -1;
}

#ifdef ESLAM_STAMPS
// diagnostic builds: zero the stamps (before the launch to be measured: a block that returns
// early then leaves zeros, not an older launch's stamps)
extern "C" int eslam_gpu_debug_stamps_clear(void)
{
    if (stamps_clear(g_stamps_k1) != 0 || stamps_clear(g_stamps_k1_grid) != 0 || stamps_clear(g_stamps_k1w) != 0 ||
        stamps_clear(g_stamps_k3) != 0 || stamps_clear(g_stamps_k3_grid) != 0 || stamps_mg_clear() != 0)
        return -1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

// copy the per-wave stamps of the last K1 launch (kWaveStampSlots words per wave, wave w of
// block b at b * kWaves + w); returns the launch's block count, or -1
extern "C" int64_t eslam_gpu_debug_stamps_k1_waves(uint64_t* out, uint64_t waves)
{
    if (waves > (uint64_t)kStampBlocks * kWaves) waves = (uint64_t)kStampBlocks * kWaves;
    return stamps_read(g_stamps_k1w, g_stamps_k1_grid, out, waves * kWaveStampSlots * 8);
}

// copy the stamps of the last K1 (which = 1), K3 (which = 3) or map merge (which = 5) launch; returns that launch's
// block count (its grid; blocks past kStampBlocks are not stamped), or -1
extern "C" int64_t eslam_gpu_debug_stamps(int which, uint64_t* out, uint64_t blocks)
{
    if (blocks > kStampBlocks) blocks = kStampBlocks;
    return which == 1 ? stamps_read(g_stamps_k1, g_stamps_k1_grid, out, blocks * kStampSlots * 8)
           : which == 3 ? stamps_read(g_stamps_k3, g_stamps_k3_grid, out, blocks * kStampSlots * 8)
                        : stamps_mg_read(out, blocks);
}
#endif

#ifdef ESLAM_DRAW_STATS
// out[0] the waves that counted stratified draws (K3, k_segments_multi) since the counters were
// last cleared, out[1] those of them that evaluated the draws (an ambiguous target, or no
// integer path); clear != 0 zeroes the counters afterwards
extern "C" int eslam_gpu_debug_draw_waves(uint32_t* out, int clear)
{
    const uint32_t zero[2] = {0, 0};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out, HIP_SYMBOL(g_draw_waves), 8) != hipSuccess) return -1;
    return !clear || hipMemcpyToSymbol(HIP_SYMBOL(g_draw_waves), zero, 8) == hipSuccess ? 0 : -1;
}
#endif
