// eslam_gmm.hip -- gfx950 kernels of the pose distribution's Gaussian mixture:
// a 2-D mixture over the particles' (x, y), fitted by EM on the device.
//
//   k_gmm_bounds   pass B: max w, min/max x, min/max y and the counts of the fitted and the
//                  skipped particles (order-free: integer maxima of ordered keys, integer sums),
//                  per wave; k_gmm_bounds_final, one block, combines the waves' words
//   k_gmm_pass<K>  one pass over x, y, w: the hard initial assignment, or the E-step under the
//                  current parameters fused with the sums of the next M-step; one record of
//                  6 K + 2 doubles per canonical chunk, summed in getCentroid's order (a lane's
//                  rows in order, the wave butterfly)
//   k_gmm_tree     one level of the fixed pairwise tree over the chunk records
//
// The host side (eslam_gpu_fit_pose_gmm, eslam_host_stats.hip) sequences the passes, runs the M-step
// (dm_gmm_mstep) and the stop test, and reads one record back per pass.  The arithmetic of a
// particle is eslam_detmath.h's (dm_gmm_*), shared with the CPU restatement, and the file is
// compiled with -ffp-contract=off: the fit equals tests/c/gmm_ref.c bit for bit.
#include <hip/hip_runtime.h>

#include "eslam_internal.h"
#include "eslam_launch.h"

namespace eslam_dev {

// the particle's coordinates with -0.0 as +0.0, and whether it is fitted
__device__ __forceinline__ bool gmm_load(const DevState& st, uint64_t i, double& x, double& y, double& w)
{
    x = st.x[i];
    y = st.y[i];
    w = st.w[i];
    if (x == 0.0) x = 0.0;
    if (y == 0.0) y = 0.0;
    return dm_gmm_valid(x, y, w);
}

// reduces seven words over the wave: five maxima and two sums
__device__ __forceinline__ void gmm_bounds_wave(uint64_t (&m)[5], uint64_t& used, uint64_t& skipped)
{
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int q = 0; q < 5; ++q) { const uint64_t t = __shfl_xor(m[q], o, 64); m[q] = m[q] > t ? m[q] : t; }
        used += __shfl_xor(used, o, 64);
        skipped += __shfl_xor(skipped, o, 64);
    }
}

// every wave leaves its words at part[wave id]: atomics on the seven result words from every
// wave of a 4M-particle filter serialise in L2 (measured 575 us; 12 us would read the data)
__global__ void __launch_bounds__(kBlock) k_gmm_bounds(DevState s0, DevState s1, uint64_t n, const Ctl* __restrict__ ctl,
                                                       uint64_t* __restrict__ part)
{
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    uint64_t m[5] = {0, 0, 0, 0, 0}, used = 0, skipped = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        double x, y, w;
        if (!gmm_load(st, i, x, y, w)) { ++skipped; continue; }
        ++used;
        const uint64_t k[5] = {gmm_key(w), ~gmm_key(x), gmm_key(x), ~gmm_key(y), gmm_key(y)};
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] = m[q] > k[q] ? m[q] : k[q];
    }
    gmm_bounds_wave(m, used, skipped);
    if ((threadIdx.x & 63u) == 0) {
        uint64_t* p = part + ((uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * kGmmWords;
#pragma unroll
        for (int q = 0; q < 5; ++q) p[kGmmMaxW + q] = m[q];
        p[kGmmUsed] = used;
        p[kGmmSkipped] = skipped;
    }
}

// one block: the waves' words (zeros where a wave fitted nothing) into out, zeroed before
__global__ void __launch_bounds__(kBlock) k_gmm_bounds_final(const uint64_t* __restrict__ part, uint32_t nparts,
                                                             uint64_t* __restrict__ out)
{
    uint64_t m[5] = {0, 0, 0, 0, 0}, used = 0, skipped = 0;
    for (uint32_t r = threadIdx.x; r < nparts; r += kBlock) {
        const uint64_t* p = part + (uint64_t)r * kGmmWords;
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] = m[q] > p[kGmmMaxW + q] ? m[q] : p[kGmmMaxW + q];
        used += p[kGmmUsed];
        skipped += p[kGmmSkipped];
    }
    gmm_bounds_wave(m, used, skipped);
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int q = 0; q < 5; ++q) atomicMax((unsigned long long*)&out[kGmmMaxW + q], (unsigned long long)m[q]);
        atomicAdd((unsigned long long*)&out[kGmmUsed], (unsigned long long)used);
        atomicAdd((unsigned long long*)&out[kGmmSkipped], (unsigned long long)skipped);
    }
}

// One chunk per wave, one particle per lane per row.  HARD: responsibility 1 for the component of
// the particle's slab on the longer axis; else the E-step under P.c.  6 K + 2 accumulators per lane.
template <int K, bool HARD>
__global__ void __launch_bounds__(kBlock) k_gmm_pass(DevState s0, DevState s1, uint64_t n, uint32_t J, const Ctl* __restrict__ ctl,
                                                     const GmmPass P, double* __restrict__ chunk_out)
{
    constexpr int R = DM_GMM_REC(K);
    // the E-step's parameters are read from LDS: K x 11 doubles held in scalar registers beside
    // the accumulators' addresses spilled (K >= 5)
    __shared__ dm_gmm_comp sc[HARD ? 1 : K];
    if constexpr (!HARD) {
        constexpr uint32_t words = K * sizeof(dm_gmm_comp) / 8;
        const uint64_t* src = reinterpret_cast<const uint64_t*>(P.c);
        for (uint32_t t = threadIdx.x; t < words; t += kBlock) reinterpret_cast<uint64_t*>(sc)[t] = src[t];
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t chunk = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t lbase = chunk * 64ull * J;
    if (lbase >= n) return;
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    double a[R];
#pragma unroll
    for (int q = 0; q < R; ++q) a[q] = 0.0;
    for (uint32_t j = 0; j < J; ++j) {
        const uint64_t i = lbase + 64ull * j + lane;
        if (i >= n) continue;
        double x, y, w;
        if (!gmm_load(st, i, x, y, w)) continue;
        const double wh = dm_ldexp(w, -P.E);
        const double xp = x - P.cx, yp = y - P.cy;
        if constexpr (HARD) {
            const int kk = dm_gmm_hard(P.axis ? y : x, P.amin, P.h, K);
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (k == kk) dm_gmm_add(&a[6 * k], wh, xp, yp);
            a[6 * K] = a[6 * K] + wh;
        } else {
            double r[K];
            // the parameters are read again every row: hoisted out of the loop they would occupy
            // 22 VGPRs per component for the whole kernel
            __asm__ volatile("" ::: "memory");
            const double ll = dm_gmm_estep(sc, K, xp, yp, r);
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (sc[k].live) dm_gmm_add(&a[6 * k], wh * r[k], xp, yp);
            a[6 * K] = a[6 * K] + wh;
            a[6 * K + 1] = a[6 * K + 1] + wh * ll;
        }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
        double v = a[q];
        for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
        if (lane == 0) chunk_out[chunk * R + q] = v;
    }
}

// one level of the fixed pairwise tree over m records of R doubles: dst[i] = src[2i] + src[2i+1];
// an odd tail moves up (k_tree_level at any record width)
__global__ void __launch_bounds__(kBlock) k_gmm_tree(const double* __restrict__ src, double* __restrict__ dst, uint64_t m, uint32_t R)
{
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i = t / R, q = t % R;
    const uint64_t h = m / 2;
    if (i > h || (i == h && !(m & 1))) return;
    dst[i * R + q] = i < h ? src[(2 * i) * R + q] + src[(2 * i + 1) * R + q] : src[(m - 1) * R + q];
}

template <int K>
static void gmm_pass_launch(bool hard, uint32_t blocks, DevState s0, DevState s1, uint64_t n, uint32_t J, const Ctl* ctl,
                            const GmmPass& P, double* chunk_out, hipStream_t stream)
{
    if (hard) hipLaunchKernelGGL((k_gmm_pass<K, true>), dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, J, ctl, P, chunk_out);
    else hipLaunchKernelGGL((k_gmm_pass<K, false>), dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, J, ctl, P, chunk_out);
}

}  // namespace eslam_dev

// pass B of this context's particles into out[kGmmWords] (zeroed here); part: scratch of
// kGmmBoundsBlocks x kWaves x kGmmWords words
extern "C" hipError_t eslam_launch_gmm_bounds(DevState s0, DevState s1, uint64_t n, Ctl* ctl, uint64_t* part, uint64_t* out,
                                              hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(out, 0, kGmmWords * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    uint32_t blocks = (uint32_t)((n + kBlock - 1) / kBlock);
    if (blocks > (uint32_t)kGmmBoundsBlocks) blocks = kGmmBoundsBlocks;
    if (blocks) {
        hipLaunchKernelGGL(k_gmm_bounds, dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, ctl, part);
        hipLaunchKernelGGL(k_gmm_bounds_final, dim3(1), dim3(kBlock), 0, stream, part, blocks * kWaves, out);
    }
    return hipGetLastError();
}

// per canonical chunk (64 x J particles) of this context: the record of DM_GMM_REC(K) doubles
extern "C" hipError_t eslam_launch_gmm_pass(int K, int hard, DevState s0, DevState s1, uint64_t n, uint32_t J, Ctl* ctl,
                                            const GmmPass* P, double* chunk_out, hipStream_t stream)
{
    const uint64_t csz = 64ull * J;
    const uint64_t chunks = (n + csz - 1) / csz;
    const uint32_t blocks = (uint32_t)((chunks + kWaves - 1) / kWaves);
    if (!blocks) return hipSuccess;
    switch (K) {
    case 1: gmm_pass_launch<1>(hard != 0, blocks, s0, s1, n, J, ctl, *P, chunk_out, stream); break;
    case 2: gmm_pass_launch<2>(hard != 0, blocks, s0, s1, n, J, ctl, *P, chunk_out, stream); break;
    case 3: gmm_pass_launch<3>(hard != 0, blocks, s0, s1, n, J, ctl, *P, chunk_out, stream); break;
    case 4: gmm_pass_launch<4>(hard != 0, blocks, s0, s1, n, J, ctl, *P, chunk_out, stream); break;
    case 5: gmm_pass_launch<5>(hard != 0, blocks, s0, s1, n, J, ctl, *P, chunk_out, stream); break;
    case 6: gmm_pass_launch<6>(hard != 0, blocks, s0, s1, n, J, ctl, *P, chunk_out, stream); break;
    case 7: gmm_pass_launch<7>(hard != 0, blocks, s0, s1, n, J, ctl, *P, chunk_out, stream); break;
    case 8: gmm_pass_launch<8>(hard != 0, blocks, s0, s1, n, J, ctl, *P, chunk_out, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the fixed pairwise tree over m chunk records of R doubles at a (b: scratch of the same size;
// both are overwritten); the total goes to out (device or pinned host memory); m == 0: zeros
extern "C" hipError_t eslam_launch_gmm_tree(double* a, double* b, uint64_t m, uint32_t R, double* out, hipStream_t stream)
{
    if (m == 0) {
        const hipError_t e = hipMemsetAsync(a, 0, R * sizeof(double), stream);
        if (e != hipSuccess) return e;
    }
    while (m > 1) {
        const uint64_t m2 = (m + 1) / 2;
        hipLaunchKernelGGL(k_gmm_tree, dim3((uint32_t)((m2 * R + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, a, b, m, R);
        double* t = a; a = b; b = t;
        m = m2;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, a, R * sizeof(double), hipMemcpyDefault, stream);
    return e;
}
