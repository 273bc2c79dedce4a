// eslam_stamps.h -- diagnostic builds only (-DESLAM_STAMPS, -DESLAM_DRAW_STATS; tools/stamps.py,
// tools/stamps_maps.py).  The product build compiles none of it: the macros expand to nothing.
//
// -DESLAM_STAMPS: per-block s_memrealtime stamps (100 MHz, one clock for the whole device) at
// the phase boundaries of K1, K3 and the map merge, written by thread 0 to arrays of their own.
// Each array, with the word that holds the grid of the last stamped launch, lives in the file of
// the kernel that writes it (ESLAM_STAMP_ARRAY): g_stamps_k1, the per-wave g_stamps_k1w and
// g_stamps_k3 in eslam_kernels.hip, g_stamps_mg in eslam_particle_maps.hip.  The exported
// eslam_gpu_debug_stamps* functions (eslam_kernels.hip) reach the other file's array through
// stamps_mg_clear and stamps_mg_read below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eslam_internal.h"

namespace eslam_dev {

#ifdef ESLAM_STAMPS
constexpr uint32_t kStampBlocks = 32768, kStampSlots = 8;
#define ESLAM_STAMP_ARRAY(arr) \
    __device__ uint64_t arr[kStampBlocks][kStampSlots]; \
    __device__ uint32_t arr##_grid           /* gridDim.x of the last stamped launch */
__device__ __forceinline__ uint64_t stamp_now()
{
    uint64_t t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
// blockIdx.x through an empty asm: each stamp forms its address anew, so none is kept in VGPRs
// from one stamp to the next, across the phase between them (K1's bench instantiation: 99 VGPRs
// with the addresses kept, 98 without; -DESLAM_K1_WPE=5 holds it to the product's 96 and five
// waves a SIMD, with 24 bytes of scratch)
__device__ __forceinline__ uint32_t stamp_block()
{
    uint32_t b = blockIdx.x;
    asm volatile("" : "+s"(b));
    return b;
}
#define ESLAM_STAMP(arr, k) \
    do { \
        const uint32_t sb_ = stamp_block(); \
        if (threadIdx.x == 0 && sb_ < kStampBlocks) arr[sb_][(k)] = stamp_now(); \
        if ((k) == 0 && threadIdx.x == 0 && blockIdx.x == 0) arr##_grid = gridDim.x; \
    } while (0)
// K1 also stamps per wave (lane 0 of each wave, slots below), all three outside the row loop
// and stored at once, so no stamp is live across the rows and the diagnostic kernel keeps the
// product's registers.  The placement word is HW_ID (wave slot, SIMD, CU, SH, SE) | XCC_ID << 32.
constexpr uint32_t kWaveStampSlots = 4;  // start, first row starts, last row done, placement
// (K1's stamps test its own lane and wave, which it keeps anyway, not threadIdx.x)
#define ESLAM_STAMP_K1(k) \
    do { \
        const uint32_t sb_ = stamp_block(); \
        if (lane == 0 && wave == 0 && sb_ < kStampBlocks) g_stamps_k1[sb_][(k)] = stamp_now(); \
    } while (0)
#define ESLAM_STAMP_WAVE(k) \
    do { \
        const uint32_t sb_ = stamp_block(); \
        if (lane == 0 && sb_ < kStampBlocks) { \
            uint64_t* ws_ = g_stamps_k1w[sb_ * kWaves + wave]; \
            ws_[(k)] = stamp_now(); \
            if ((k) == 0) ws_[3] = (uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32); \
        } \
    } while (0)

// host side: zero a device symbol (a stamp array or a grid word); 0, or -1
template <class A> static int stamps_clear(const A& sym)
{
    void* p = nullptr;
    return hipGetSymbolAddress(&p, HIP_SYMBOL(sym)) == hipSuccess && hipMemset(p, 0, sizeof(A)) == hipSuccess ? 0 : -1;
}
// copy a stamp array's first `bytes` bytes to out; returns the grid of the launch that wrote them, or -1
template <class A> static int64_t stamps_read(const A& arr, const uint32_t& grid, uint64_t* out, size_t bytes)
{
    uint32_t blocks = 0;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(arr), bytes) == hipSuccess &&
                   hipMemcpyFromSymbol(&blocks, HIP_SYMBOL(grid), 4) == hipSuccess ? (int64_t)blocks : -1;
}
// the two on the map merge's array, defined next to it (not exported)
__attribute__((visibility("hidden"))) int stamps_mg_clear();
__attribute__((visibility("hidden"))) int64_t stamps_mg_read(uint64_t* out, uint64_t blocks);
#else
#define ESLAM_STAMP(arr, k) do { } while (0)
#define ESLAM_STAMP_K1(k) do { } while (0)
#define ESLAM_STAMP_WAVE(k) do { } while (0)
#endif

// -DESLAM_DRAW_STATS (eslam_kernels.hip's g_draw_waves): how many waves counted stratified draws
// (wave_counts) and how many of them had to evaluate the draws.  Kept apart from the stamps: the
// two atomics per wave on one address disturb the timeline.
#ifdef ESLAM_DRAW_STATS
#define ESLAM_DRAW_WAVE(k) do { if ((threadIdx.x & 63u) == 0) atomicAdd(&g_draw_waves[(k)], 1u); } while (0)
#else
#define ESLAM_DRAW_WAVE(k) do { } while (0)
#endif

}  // namespace eslam_dev
