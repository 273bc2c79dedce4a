// eslam_wave.h -- lane and wave primitives of the gfx950 kernels (device code only): xor-lane
// moves without the LDS crossbar, the butterflies and the max-scan built on them, and the
// agent-scope atomics.  Everything is wave64.  The butterflies' association order is part of
// the sum contract (include/eslam_detmath.h): a kernel whose fp64 result bits are fixed by
// another order keeps its own reduction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eslam_internal.h"

namespace eslam_dev {

// lane i receives lane i ^ O's value without the LDS crossbar (ds_bpermute: ~100+ cycles of
// latency per step).  O = 1, 2: DPP quad_perm; O = 4, 8: DPP row_shl / row_shr, each writing
// only the banks (4-lane groups of a row) whose partner lies in that direction; O = 16, 32:
// gfx950's v_permlane16_swap / v_permlane32_swap (odd rows <-> even rows, upper half <->
// lower half) with both operands the value, then a per-lane pick of the swapped copy.
template <int O> __device__ __forceinline__ uint32_t xor_lane_u32(uint32_t v)
{
    static_assert(O == 1 || O == 2 || O == 4 || O == 8 || O == 16 || O == 32, "xor distance");
    if constexpr (O == 32) {
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);   // r[0]: [lo, lo], r[1]: [hi, hi]
        return (threadIdx.x & 32u) ? r[0] : r[1];
    } else if constexpr (O == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);   // r[0]: even rows, r[1]: odd rows
        return (threadIdx.x & 16u) ? r[0] : r[1];
    } else if constexpr (O == 8) {
        const int t = __builtin_amdgcn_update_dpp(0, (int)v, 0x108, 0xf, 0x3, false);     // row_shl:8, banks 0-1
        return (uint32_t)__builtin_amdgcn_update_dpp(t, (int)v, 0x118, 0xf, 0xc, false);  // row_shr:8, banks 2-3
    } else if constexpr (O == 4) {
        const int t = __builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xf, 0x5, false);     // row_shl:4, banks 0, 2
        return (uint32_t)__builtin_amdgcn_update_dpp(t, (int)v, 0x114, 0xf, 0xa, false);  // row_shr:4, banks 1, 3
    } else if constexpr (O == 2) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    } else {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    }
}

template <int O> __device__ __forceinline__ uint64_t xor_lane_u64(uint64_t v)
{
    return (uint64_t)xor_lane_u32<O>((uint32_t)v) | ((uint64_t)xor_lane_u32<O>((uint32_t)(v >> 32)) << 32);
}
template <int O> __device__ __forceinline__ double xor_lane(double v) { return dm_from_bits(xor_lane_u64<O>(dm_bits(v))); }
template <int O> __device__ __forceinline__ float xor_lane(float v) { return __uint_as_float(xor_lane_u32<O>(__float_as_uint(v))); }
template <int O> __device__ __forceinline__ uint32_t xor_lane(uint32_t v) { return xor_lane_u32<O>(v); }
template <int O> __device__ __forceinline__ uint64_t xor_lane(uint64_t v) { return xor_lane_u64<O>(v); }

// xor butterfly over the 64 lanes, distances 32, 16, ..., 1 (the sum contract's chunk tree:
// every stage adds the same pair in both lanes, so all lanes end with the same bits)
template <class T, class Op> __device__ __forceinline__ T wave_butterfly(T v, Op op)
{
    v = op(v, xor_lane<32>(v));
    v = op(v, xor_lane<16>(v));
    v = op(v, xor_lane<8>(v));
    v = op(v, xor_lane<4>(v));
    v = op(v, xor_lane<2>(v));
    v = op(v, xor_lane<1>(v));
    return v;
}

// one stage of a transposed xor butterfly over 2H totals per lane (see K1's chunk flush):
// the lane with bit O set keeps the upper H totals, its partner the lower H, and each adds
// the partner's copy of the totals it keeps
// transpose_add with another order-free operation (float maxima)
template <int O, int H, int N, class Op> __device__ __forceinline__ void transpose_op(float (&v)[N], uint32_t lane, Op op)
{
    const bool up = (lane & (uint32_t)O) != 0u;
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const float send = up ? v[j] : v[H + j];
        const float keep = up ? v[H + j] : v[j];
        v[j] = op(keep, xor_lane<O>(send));
    }
}

template <int O, int H, int N> __device__ __forceinline__ void transpose_add(double (&v)[N], uint32_t lane)
{
    const bool up = (lane & (uint32_t)O) != 0u;
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const double send = up ? v[j] : v[H + j];
        const double keep = up ? v[H + j] : v[j];
        v[j] = keep + xor_lane<O>(send);
    }
}

__device__ __forceinline__ double wave_sum_butterfly(double v)
{
    return wave_butterfly(v, [](double a, double b) { return a + b; });
}

__device__ __forceinline__ double wave_max_butterfly(double v)
{
    return wave_butterfly(v, [](double a, double b) { return (a < b) ? b : a; });
}

// inclusive max-scan over the 64 lanes with DPP (VALU lane moves, no LDS round trips):
// row_shr 1,2,4,8 inside each row of 16, then row_bcast:15 and row_bcast:31 across rows.
// 0 is the identity (lanes without a source keep it).
__device__ __forceinline__ uint32_t wave_incl_max_u32(uint32_t m)
{
    uint32_t t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x111, 0xf, 0xf, false); m = m > t ? m : t;   // row_shr:1
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x112, 0xf, 0xf, false); m = m > t ? m : t;   // row_shr:2
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x114, 0xf, 0xf, false); m = m > t ? m : t;   // row_shr:4
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x118, 0xf, 0xf, false); m = m > t ? m : t;   // row_shr:8
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x142, 0xa, 0xf, false); m = m > t ? m : t;   // row_bcast:15
    t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x143, 0xc, 0xf, false); m = m > t ? m : t;   // row_bcast:31
    return m;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    return wave_butterfly(v, [](uint32_t a, uint32_t b) { return a + b; });
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
    return wave_butterfly(v, [](uint64_t a, uint64_t b) { return a + b; });
}

__device__ __forceinline__ uint64_t atomic_load_agent(const uint64_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void atomic_store_agent(uint64_t* p, uint64_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace eslam_dev
