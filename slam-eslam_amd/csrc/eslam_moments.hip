// eslam_moments.hip -- gfx950 kernels of the pose estimate's moments: the weighted
// mean of (x, y, z), the circular mean of the yaw and the 4 x 4 covariance over (x, y, z, yaw
// deviation) of the valid particles, or of those inside a gate ellipse over (x, y).
//
//   k_moments_bounds    pass B: max w over the valid particles and the counts of the counted, the
//                       gated-out and the skipped ones (order-free: an integer maximum of ordered
//                       keys, integer sums), per wave; k_moments_bounds_final, one block, combines
//                       the waves' words
//   k_moments_pass<P>   P = 1: W_all and the counted particles' S0, Q, Sx, Sy, Sz, Ss, Sc, Sv;
//                       P = 2: S0, the four first and the ten second moments of the deviations
//                       from the mean; one record of 9 or 15 doubles per canonical chunk, summed in
//                       getCentroid's order (a lane's rows in order, the wave butterfly)
//
// The fixed pairwise tree over the chunk records is eslam_gmm.hip's (eslam_launch_gmm_tree).  The
// host side (eslam_gpu_pose_moments, eslam_host_stats.hip) sequences the passes and forms the mean
// (dm_mom_mean) and the covariance (dm_mom_cov).  The arithmetic of a particle is
// eslam_detmath.h's (dm_mom_*), shared with the CPU restatement, and the file is compiled with
// -ffp-contract=off: the result equals tests/c/moments_ref.c bit for bit.
#include <hip/hip_runtime.h>

#include "eslam_internal.h"
#include "eslam_launch.h"

namespace eslam_dev {

// a particle's six values, and whether it is valid
__device__ __forceinline__ bool mom_load(const DevState& st, uint64_t i, double& x, double& y, double& z, double& th, double& zs,
                                         double& w)
{
    x = st.x[i];
    y = st.y[i];
    z = st.z[i];
    th = st.th[i];
    zs = st.zs[i];
    w = st.w[i];
    return dm_mom_valid(x, y, z, th, zs, w);
}

// reduces the four words over the wave: one maximum and three sums
__device__ __forceinline__ void mom_bounds_wave(uint64_t& m, uint64_t (&c)[3])
{
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t t = __shfl_xor(m, o, 64);
        m = m > t ? m : t;
#pragma unroll
        for (int q = 0; q < 3; ++q) c[q] += __shfl_xor(c[q], o, 64);
    }
}

// every wave leaves its words at part[wave id] (no atomics on one line: k_gmm_bounds)
__global__ void __launch_bounds__(kBlock) k_moments_bounds(DevState s0, DevState s1, uint64_t n, const Ctl* __restrict__ ctl,
                                                           const dm_mom_gate g, uint64_t* __restrict__ part)
{
    const DevState st = (ctl->base ^ ctl->flip) ? s1 : s0;
    uint64_t m = 0, c[3] = {0, 0, 0};                // counted, gated out, skipped
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        double x, y, z, th, zs, w;
        if (!mom_load(st, i, x, y, z, th, zs, w)) { ++c[2]; continue; }
        const uint64_t k = gmm_key(w);
        m = m > k ? m : k;
        if (dm_mom_inside(&g, x, y)) ++c[0];
        else ++c[1];
    }
    mom_bounds_wave(m, c);
    if ((threadIdx.x & 63u) == 0) {
        uint64_t* p = part + ((uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * kMomWords;
        p[kMomMaxW] = m;
#pragma unroll
        for (int q = 0; q < 3; ++q) p[kMomCounted + q] = c[q];
    }
}

// one block: the waves' words into out, zeroed before
__global__ void __launch_bounds__(kBlock) k_moments_bounds_final(const uint64_t* __restrict__ part, uint32_t nparts,
                                                                 uint64_t* __restrict__ out)
{
    uint64_t m = 0, c[3] = {0, 0, 0};
    for (uint32_t r = threadIdx.x; r < nparts; r += kBlock) {
        const uint64_t* p = part + (uint64_t)r * kMomWords;
        m = m > p[kMomMaxW] ? m : p[kMomMaxW];
#pragma unroll
        for (int q = 0; q < 3; ++q) c[q] += p[kMomCounted + q];
    }
    mom_bounds_wave(m, c);
    if ((threadIdx.x & 63u) == 0) {
        atomicMax((unsigned long long*)&out[kMomMaxW], (unsigned long long)m);
#pragma unroll
        for (int q = 0; q < 3; ++q) atomicAdd((unsigned long long*)&out[kMomCounted + q], (unsigned long long)c[q]);
    }
}

// One chunk per wave, one particle per lane per row; 9 (PASS 1) or 15 (PASS 2) accumulators per lane.
template <int PASS>
__global__ void __launch_bounds__(kBlock) k_moments_pass(DevState s0, DevState s1, uint64_t n, uint32_t J, const Ctl* __restrict__ ctl,
                                                         const MomPass P, double* __restrict__ chunk_out)
{
    constexpr int R = PASS == 1 ? DM_MOM_REC1 : DM_MOM_REC2;
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
        double x, y, z, th, zs, w;
        if (!mom_load(st, i, x, y, z, th, zs, w)) continue;
        const double wh = dm_ldexp(w, -P.E);
        const int inside = dm_mom_inside(&P.g, x, y);
        if constexpr (PASS == 1) {
            dm_mom_add1(a, inside, wh, x, y, z, th, zs);
        } else {
            if (inside) dm_mom_add2(a, wh, P.mean, x, y, z, th);
        }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
        double v = a[q];
        for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
        if (lane == 0) chunk_out[chunk * R + q] = v;
    }
}

}  // namespace eslam_dev

// pass B of this context's particles into out[kMomWords] (zeroed here); part: scratch of
// kMomBoundsBlocks x kWaves x kMomWords words
extern "C" hipError_t eslam_launch_moments_bounds(DevState s0, DevState s1, uint64_t n, Ctl* ctl, const MomPass* P, uint64_t* part,
                                                  uint64_t* out, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(out, 0, kMomWords * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    uint32_t blocks = (uint32_t)((n + kBlock - 1) / kBlock);
    if (blocks > (uint32_t)kMomBoundsBlocks) blocks = kMomBoundsBlocks;
    if (blocks) {
        hipLaunchKernelGGL(k_moments_bounds, dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, ctl, P->g, part);
        hipLaunchKernelGGL(k_moments_bounds_final, dim3(1), dim3(kBlock), 0, stream, part, blocks * kWaves, out);
    }
    return hipGetLastError();
}

// per canonical chunk (64 x J particles) of this context: the record of DM_MOM_REC1 (pass 1) or
// DM_MOM_REC2 (pass 2) doubles
extern "C" hipError_t eslam_launch_moments_pass(int pass, DevState s0, DevState s1, uint64_t n, uint32_t J, Ctl* ctl,
                                                const MomPass* P, double* chunk_out, hipStream_t stream)
{
    const uint64_t csz = 64ull * J;
    const uint64_t chunks = (n + csz - 1) / csz;
    const uint32_t blocks = (uint32_t)((chunks + kWaves - 1) / kWaves);
    if (!blocks) return hipSuccess;
    if (pass == 1) hipLaunchKernelGGL((k_moments_pass<1>), dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, J, ctl, *P, chunk_out);
    else if (pass == 2) hipLaunchKernelGGL((k_moments_pass<2>), dim3(blocks), dim3(kBlock), 0, stream, s0, s1, n, J, ctl, *P, chunk_out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
