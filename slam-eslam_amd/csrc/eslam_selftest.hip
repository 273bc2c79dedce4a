// eslam_selftest.hip -- the device self-tests: the deterministic math and the lane exchanges
// (k_selftest_math) and every Box-Muller radius (k_selftest_bm_radius), with their launchers.
#include <hip/hip_runtime.h>

#include "eslam_internal.h"
#include "eslam_launch.h"
#include "eslam_wave.h"

namespace eslam_dev {

// device self-test of the deterministic math (tests/test_gpu_math.py)
__global__ void k_selftest_math(int fn, const double* x, const double* y, double* out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (fn >= 20 && fn <= 25) {
        // lane exchanges of the butterflies: x[i ^ 2^(fn - 20)] (n a multiple of the block)
        const double v = i < n ? x[i] : 0.0;
        double r = 0.0;
        switch (fn) {
        case 20: r = xor_lane<1>(v); break;
        case 21: r = xor_lane<2>(v); break;
        case 22: r = xor_lane<4>(v); break;
        case 23: r = xor_lane<8>(v); break;
        case 24: r = xor_lane<16>(v); break;
        default: r = xor_lane<32>(v); break;
        }
        if (i < n) out[i] = r;
        return;
    }
    if (i >= n) return;
    double s, c, r = 0;
    switch (fn) {
    case 0: r = dm_exp(x[i]); break;
    case 1: r = dm_log(x[i]); break;
    case 2: dm_sincos(x[i], &s, &c); r = s; break;
    case 3: dm_sincos(x[i], &s, &c); r = c; break;
    case 4: r = dm_erfc(x[i]); break;
    case 5: r = dm_sqrt(x[i]); break;
    case 6: r = x[i] / y[i]; break;
    case 7: r = dm_normal_pdf_cdf_ratio(x[i], y[i]); break;
    case 8: r = dm_pow(x[i], y[i]); break;
    case 9: r = dm_from_bits(dm_fx61(x[i])); break;
    case 13: dm_sincos2pi(x[i], &s, &c); r = s; break;
    case 14: dm_sincos2pi(x[i], &s, &c); r = c; break;
    case 15: r = dm_log_bm(x[i]); break;
    case 16: dm_sincos2pi32((uint32_t)x[i], &s, &c); r = s; break;
    case 17: dm_sincos2pi32((uint32_t)x[i], &s, &c); r = c; break;
    case 18: dm_box_muller32((uint32_t)x[i], (uint32_t)y[i], &s, &c); r = s; break;
    case 19: dm_box_muller32((uint32_t)x[i], (uint32_t)y[i], &s, &c); r = c; break;
    case 26: { float fs, fc; dm_sincos2pi32f((uint32_t)x[i], &fs, &fc); r = fs; } break;
    case 27: { float fs, fc; dm_sincos2pi32f((uint32_t)x[i], &fs, &fc); r = fc; } break;
    default: r = __builtin_nan("");
    }
    out[i] = r;
}

// every Box-Muller radius: the range-restricted sqrt against the general one on -2 log u, for
// all 2^32 uniform words (counts the words whose radius differs in any bit)
__global__ void __launch_bounds__(kBlock) k_selftest_bm_radius(unsigned long long* bad)
{
    uint32_t cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t a = (uint64_t)blockIdx.x * kBlock + threadIdx.x; a < (1ull << 32); a += stride) {
        const float x = (float)(-2.0 * dm_log_bm(dm_u32((uint32_t)a)));
        cnt += __float_as_uint(dm_sqrtf_pos(x)) != __float_as_uint(__builtin_sqrtf(x)) ? 1u : 0u;
    }
    cnt = wave_sum_u32(cnt);
    if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(bad, (unsigned long long)cnt);
}

}  // namespace eslam_dev

using namespace eslam_dev;

extern "C" hipError_t eslam_launch_selftest_math(int fn, const double* x, const double* y, double* out, uint64_t n,
                                                 hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_selftest_math, dim3(blocks), dim3(kBlock), 0, stream, fn, x, y, out, n);
    return hipGetLastError();
}

extern "C" hipError_t eslam_launch_selftest_bm_radius(unsigned long long* bad, hipStream_t stream)
{
    hipLaunchKernelGGL(k_selftest_bm_radius, dim3(4096), dim3(kBlock), 0, stream, bad);
    return hipGetLastError();
}
