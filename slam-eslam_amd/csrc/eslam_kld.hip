// eslam_kld.hip -- gfx950 kernels of KLD-sampling's bin count: the occupied bins
// of a fixed lattice over the particles' (x, y, yaw), counted exactly.
//
//   k_kld_bounds    pass 1: every particle counted or skipped (dm_kld_index); the minima and maxima
//                   of the counted particles' cell indices and the two counts, per wave by
//                   shuffles, per block through LDS, one record per block
//   k_kld_fold      one block: the blocks' records into one (minima, maxima, integer sums)
//   k_kld_mark      pass 2, over particles [first, n): the indices again, and the particle's bit in
//                   the box's bitmap
//   k_kld_or        sharded: the word-wise OR of the ranks' gathered bitmaps
//   k_kld_popcount  pass 3: the set bits of the bitmap, one record per block (folded by k_kld_fold)
//
// Minima, maxima, integer sums, ORs and a population count do not depend on the order anything
// arrives in, so the count is the same bits on one GPU, on a sharded filter and in
// tests/c/kld_ref.c.  The host side (eslam_gpu_kld_count, eslam_host_stats.hip) reads the box between
// pass 1 and pass 2 and computes the bound.  A particle's arithmetic is eslam_detmath.h's, shared
// with the CPU restatement; the file is compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "eslam_internal.h"
#include "eslam_launch.h"

namespace eslam_dev {

constexpr int64_t kKldNoMin = 2147483647ll, kKldNoMax = -2147483648ll;

// a record over the wave, then over the block; thread 0 returns the block's
__device__ __forceinline__ void kld_reduce_block(int64_t (&r)[kKldWords])
{
    __shared__ int64_t sh[kWaves][kKldWords];
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int q = 0; q < kKldWords; ++q) {
            const int64_t t = __shfl_xor(r[q], o, 64);
            if (q == kKldIx0 || q == kKldIy0) r[q] = r[q] < t ? r[q] : t;
            else if (q == kKldIx1 || q == kKldIy1) r[q] = r[q] > t ? r[q] : t;
            else r[q] += t;
        }
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int q = 0; q < kKldWords; ++q) sh[threadIdx.x >> 6][q] = r[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < kWaves; ++v) {
#pragma unroll
            for (int q = 0; q < kKldWords; ++q) {
                const int64_t t = sh[v][q];
                if (q == kKldIx0 || q == kKldIy0) r[q] = r[q] < t ? r[q] : t;
                else if (q == kKldIx1 || q == kKldIy1) r[q] = r[q] > t ? r[q] : t;
                else r[q] += t;
            }
        }
    }
}

__device__ __forceinline__ void kld_record_init(int64_t (&r)[kKldWords])
{
    r[kKldIx0] = r[kKldIy0] = kKldNoMin;
    r[kKldIx1] = r[kKldIy1] = kKldNoMax;
    r[kKldCounted] = r[kKldSkipped] = 0;
}

__global__ void __launch_bounds__(kBlock) k_kld_bounds(DevState s0, DevState s1, uint64_t n, const Ctl* __restrict__ ctl, double inv,
                                                       uint32_t theta_bins, int64_t* __restrict__ part)
{
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    int64_t r[kKldWords];
    kld_record_init(r);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        int32_t ix, iy;
        uint32_t it;
        if (!dm_kld_index(st.x[i], st.y[i], st.th[i], st.w[i], inv, theta_bins, &ix, &iy, &it)) { ++r[kKldSkipped]; continue; }
        ++r[kKldCounted];
        r[kKldIx0] = r[kKldIx0] < ix ? r[kKldIx0] : ix;
        r[kKldIx1] = r[kKldIx1] > ix ? r[kKldIx1] : ix;
        r[kKldIy0] = r[kKldIy0] < iy ? r[kKldIy0] : iy;
        r[kKldIy1] = r[kKldIy1] > iy ? r[kKldIy1] : iy;
    }
    kld_reduce_block(r);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kKldWords; ++q) part[(uint64_t)blockIdx.x * kKldWords + q] = r[q];
    }
}

// one block: nparts records into out
__global__ void __launch_bounds__(kBlock) k_kld_fold(const int64_t* __restrict__ part, uint32_t nparts, int64_t* __restrict__ out)
{
    int64_t r[kKldWords];
    kld_record_init(r);
    for (uint32_t p = threadIdx.x; p < nparts; p += kBlock) {
        const int64_t* s = part + (uint64_t)p * kKldWords;
        r[kKldIx0] = r[kKldIx0] < s[kKldIx0] ? r[kKldIx0] : s[kKldIx0];
        r[kKldIx1] = r[kKldIx1] > s[kKldIx1] ? r[kKldIx1] : s[kKldIx1];
        r[kKldIy0] = r[kKldIy0] < s[kKldIy0] ? r[kKldIy0] : s[kKldIy0];
        r[kKldIy1] = r[kKldIy1] > s[kKldIy1] ? r[kKldIy1] : s[kKldIy1];
        r[kKldCounted] += s[kKldCounted];
        r[kKldSkipped] += s[kKldSkipped];
    }
    kld_reduce_block(r);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kKldWords; ++q) out[q] = r[q];
    }
}

// The particles a first small launch marks before the launch over the rest.  On a converged
// cloud every wave of one launch starts on clear words and sends its atomics to the same few of
// them; after this head the rest finds its bits set (4M particles: 0.24 ms a call without it,
// 0.11 ms with it)
constexpr uint64_t kKldHead = 16384;

__global__ void __launch_bounds__(kBlock) k_kld_mark(DevState s0, DevState s1, uint64_t first, uint64_t n, const Ctl* __restrict__ ctl,
                                                     const KldGrid g, uint64_t* __restrict__ bits, uint64_t words)
{
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    // whole waves take every trip: the shuffles of mark_bits_wave (eslam_internal.h) need all 64 lanes
    for (uint64_t b = first + (uint64_t)blockIdx.x * kBlock; b < n; b += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = b + threadIdx.x;
        bool need = false;
        uint64_t wi = 0, m = 0;
        if (i < n) {
            int32_t ix, iy;
            uint32_t it;
            if (dm_kld_index(st.x[i], st.y[i], st.th[i], st.w[i], g.inv, g.theta_bins, &ix, &iy, &it)) {
                const uint64_t bit = ((uint64_t)((int64_t)iy - g.iy0) * g.nx + (uint64_t)((int64_t)ix - g.ix0)) * g.theta_bins + it;
                wi = bit >> 6;
                m = 1ull << (bit & 63u);
                // the box is pass 1's over the same particles; a word beyond it would be a fault
                need = wi < words;
            }
        }
        mark_bits_wave(bits, need, wi, m);
    }
}

__global__ void __launch_bounds__(kBlock) k_kld_or(const uint64_t* __restrict__ all, uint32_t G, uint64_t words, uint64_t* __restrict__ bits)
{
    for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < words; w += (uint64_t)gridDim.x * kBlock) {
        uint64_t v = 0;
        for (uint32_t r = 0; r < G; ++r) v |= all[(uint64_t)r * words + w];
        bits[w] = v;
    }
}

__global__ void __launch_bounds__(kBlock) k_kld_popcount(const uint64_t* __restrict__ bits, uint64_t words, int64_t* __restrict__ part)
{
    int64_t r[kKldWords];
    kld_record_init(r);
    for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < words; w += (uint64_t)gridDim.x * kBlock)
        r[kKldCounted] += __popcll(bits[w]);
    kld_reduce_block(r);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kKldWords; ++q) part[(uint64_t)blockIdx.x * kKldWords + q] = r[q];
    }
}

static uint32_t kld_blocks(uint64_t items)
{
    const uint64_t b = (items + kBlock - 1) / kBlock;
    return (uint32_t)(b > (uint64_t)kKldBlocks ? (uint64_t)kKldBlocks : b);
}

}  // namespace eslam_dev

// pass 1 over this context's particles: the folded record at out[kKldWords]; part: kKldBlocks records
extern "C" hipError_t eslam_launch_kld_bounds(DevState s0, DevState s1, uint64_t n, const Ctl* ctl, double inv, uint32_t theta_bins,
                                              int64_t* part, int64_t* out, hipStream_t stream)
{
    const uint32_t blocks = kld_blocks(n);
    if (blocks) hipLaunchKernelGGL(k_kld_bounds, dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, ctl, inv, theta_bins, part);
    hipLaunchKernelGGL(k_kld_fold, dim3(1), dim3(kBlock), 0, stream, part, blocks, out);
    return hipGetLastError();
}

// pass 2: the bitmap of `words` words is zeroed, then every counted particle's bit is set: the
// first kKldHead particles in a launch of their own, then the rest
extern "C" hipError_t eslam_launch_kld_mark(DevState s0, DevState s1, uint64_t n, const Ctl* ctl, const KldGrid* g, uint64_t* bits,
                                            uint64_t words, hipStream_t stream)
{
    const hipError_t e = hipMemsetAsync(bits, 0, words * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    const uint64_t head = n < kKldHead ? n : kKldHead;
    if (head)
        hipLaunchKernelGGL(k_kld_mark, dim3(kld_blocks(head)), dim3(kBlock), 0, stream, s0, s1, (uint64_t)0, head, ctl, *g, bits, words);
    if (n > head)
        hipLaunchKernelGGL(k_kld_mark, dim3(kld_blocks(n - head)), dim3(kBlock), 0, stream, s0, s1, head, n, ctl, *g, bits, words);
    return hipGetLastError();
}

// bits = the OR of the G bitmaps of `words` words at `all`
extern "C" hipError_t eslam_launch_kld_or(const uint64_t* all, uint32_t G, uint64_t words, uint64_t* bits, hipStream_t stream)
{
    const uint32_t blocks = kld_blocks(words);
    if (blocks) hipLaunchKernelGGL(k_kld_or, dim3(blocks), dim3(kBlock), 0, stream, all, G, words, bits);
    return hipGetLastError();
}

// pass 3: the bitmap's set bits at out[kKldCounted]
extern "C" hipError_t eslam_launch_kld_popcount(const uint64_t* bits, uint64_t words, int64_t* part, int64_t* out, hipStream_t stream)
{
    const uint32_t blocks = kld_blocks(words);
    if (blocks) hipLaunchKernelGGL(k_kld_popcount, dim3(blocks), dim3(kBlock), 0, stream, bits, words, part);
    hipLaunchKernelGGL(k_kld_fold, dim3(1), dim3(kBlock), 0, stream, part, blocks, out);
    return hipGetLastError();
}
