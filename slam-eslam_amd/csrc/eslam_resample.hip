// eslam_resample.hip -- resample to any particle count (eslam_gpu_resample_stratified /
// eslam_gpu_resample_multinomial with samples != n; DESIGN.md 2 "Resample to a count").
//
// ParticleFilter<T>::resample_stratified(samples) and resample_multinomial(samples)
// (src/ParticleFilter.hpp:85-108, 120-148) on the exact fixed-point cumulative sum
// C_i = sum_{j <= i} fx(w_j, shift): draw k has the threshold T_k (stratified:
// fx((k + U_k) / samples); multinomial: fx(U_k)), U_k the boost uniform of the (k+1)-th minstd
// draw after the state at the call, and its ancestor is the first i with T_k <= C_i.  Both
// kinds of draw are addressable (jump-ahead), so one lane takes one draw and searches:
//   k_rs_tile_sums   the fixed-point total of every tile of kRsTile particles
//   k_rs_scan_u64    their inclusive prefix, one block: coarse[t] = C at the end of tile t
//   k_rs_cumsum      C (8 bytes per particle)
//   k_rs_draw        per draw: T_k, a binary search in coarse[], one in the tile's 16 KB of C;
//                    the ancestor (stratified beyond the sum: the last particle, counted --
//                    the Q5 clamp; multinomial beyond the sum: dropped, counted), and the kept
//                    draws per tile of kRsTile draws
//   k_rs_compact     multinomial: the kept draws' ancestors in draw order (stable), from the
//                    exclusive prefix of the tiles' counts (k_scan_excl)
//   k_rs_gather      out[k] = in[anc[k]], into buffers of the new count; the weight carried
//                    (stratified, Q4) or 1 / n_before (multinomial)
// No kernel waits for another block, and every total is an integer: any tiling gives the same
// bits.  Zero-weight particles have C_i = C_(i-1): the searches are lower bounds, so a draw
// takes the first index of an equal run, as the reference's sequential walk does.
#include "eslam_launch.h"

namespace {

constexpr int kRsTile = kScanTile;               // particles per coarse entry, draws per draw tile
constexpr int kRsItems = kRsTile / kBlock;
constexpr uint32_t kRsDropped = 0xffffffffu;     // no particle index: n < 2^32 - 1

__device__ __forceinline__ uint64_t rs_shfl_up_u64(uint64_t v, int o)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t rs_wave_incl_u64(uint64_t v, uint32_t lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t x = rs_shfl_up_u64(v, o);
        v += lane >= (uint32_t)o ? x : 0ull;
    }
    return v;
}

// inclusive prefix of v over the block's threads (in thread order) and the block's total
__device__ __forceinline__ uint64_t rs_block_incl_u64(uint64_t v, uint64_t* s_w, uint64_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t incl = rs_wave_incl_u64(v, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint64_t all = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kWaves; ++w) {
        incl += w < wave ? s_w[w] : 0ull;
        all += s_w[w];
    }
    __syncthreads();                             // s_w may be written again
    *total = all;
    return incl;
}

// the call's scalars, from the exact weight sum a FIN_SUM finalize left in ctl->S: the shift of
// eslam_gpu_resample (k_finalize, FIN_RESAMPLE), and the minstd state moved on by `samples` draws
__global__ void k_rs_begin(Ctl* __restrict__ ctl, uint32_t jump_samples, uint64_t* __restrict__ counter)
{
    if (threadIdx.x != 0) return;
    ctl->scan_shift = 61 - (dm_weight_exp(ctl->S) + 1);
    const uint32_t x0 = ctl->minstd;
    ctl->minstd_start = x0;
    ctl->minstd = dm_mulmod31(jump_samples, x0);
    counter[0] = 0;
}

__global__ void __launch_bounds__(kBlock) k_rs_tile_sums(DevState s0, DevState s1, uint64_t n, const Ctl* __restrict__ ctl,
                                                         uint64_t* __restrict__ coarse)
{
    __shared__ uint64_t s_w[kWaves];
    const double* __restrict__ w = (ctl->base ? s1 : s0).w;
    const int shift = ctl->scan_shift;
    const uint64_t base = (uint64_t)blockIdx.x * kRsTile;
    uint64_t v = 0;
#pragma unroll
    for (int r = 0; r < kRsItems; ++r) {
        const uint64_t i = base + (uint64_t)r * kBlock + threadIdx.x;
        if (i < n) v += dm_fx_shift(w[i], shift);
    }
    uint64_t total;
    (void)rs_block_incl_u64(v, s_w, &total);
    if (threadIdx.x == 0) coarse[blockIdx.x] = total;
}

// inclusive prefix of m words in place, one block, chunks of kBlock words with a carry
__global__ void __launch_bounds__(kBlock) k_rs_scan_u64(uint64_t* __restrict__ a, uint64_t m)
{
    __shared__ uint64_t s_w[kWaves];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < m; base += kBlock) {
        const uint64_t i = base + threadIdx.x;
        uint64_t total;
        const uint64_t incl = rs_block_incl_u64(i < m ? a[i] : 0ull, s_w, &total);
        if (i < m) a[i] = carry + incl;
        carry += total;
    }
}

// C: a thread scans kRsItems consecutive particles, the block joins the threads, coarse[t - 1]
// is the sum below the tile
__global__ void __launch_bounds__(kBlock) k_rs_cumsum(DevState s0, DevState s1, uint64_t n, const Ctl* __restrict__ ctl,
                                                      const uint64_t* __restrict__ coarse, uint64_t* __restrict__ C)
{
    __shared__ uint64_t s_w[kWaves];
    const double* __restrict__ w = (ctl->base ? s1 : s0).w;
    const int shift = ctl->scan_shift;
    const uint64_t i0 = (uint64_t)blockIdx.x * kRsTile + (uint64_t)threadIdx.x * kRsItems;
    uint64_t c[kRsItems];
    uint64_t run = 0;
#pragma unroll
    for (int r = 0; r < kRsItems; ++r) {
        if (i0 + r < n) run += dm_fx_shift(w[i0 + r], shift);
        c[r] = run;
    }
    uint64_t total;
    const uint64_t below = rs_block_incl_u64(run, s_w, &total) - run + (blockIdx.x ? coarse[blockIdx.x - 1] : 0ull);
#pragma unroll
    for (int r = 0; r < kRsItems; ++r)
        if (i0 + r < n) C[i0 + r] = below + c[r];
}

// the first index in [lo, hi) with a[index] >= T (hi when there is none)
__device__ __forceinline__ uint64_t rs_lower_bound(const uint64_t* __restrict__ a, uint64_t lo, uint64_t hi, uint64_t T)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < T) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one lane per draw; a block takes kRsTile consecutive draws (the compaction's tile) and counts
// the draws it keeps.  counter[0]: draws beyond the cumulative sum (overruns or dropped)
template <bool MULTI>
__global__ void __launch_bounds__(kBlock) k_rs_draw(uint64_t n, uint64_t samples, double inv_samples, const Ctl* __restrict__ ctl,
                                                    const uint32_t* __restrict__ jt, const uint64_t* __restrict__ coarse,
                                                    uint64_t ntiles, const uint64_t* __restrict__ C,
                                                    uint32_t* __restrict__ anc, uint32_t* __restrict__ kept,
                                                    uint64_t* __restrict__ counter)
{
    __shared__ uint32_t s_c[2][kWaves];
    const int shift = ctl->scan_shift;
    const uint32_t x0 = ctl->minstd_start;
    const double dS = (double)samples;
    const uint64_t base = (uint64_t)blockIdx.x * kRsTile;
    uint32_t nkeep = 0, nover = 0;
    for (int r = 0; r < kRsItems; ++r) {
        const uint64_t k = base + (uint64_t)r * kBlock + threadIdx.x;
        if (k >= samples) break;
        // the (k + 1)-th draw after x0: A^(k + 1) x0 from the jump tables (k + 1 < 2^32)
        const uint32_t x = dm_mulmod31(jump_pow(jt, k + 1), x0);
        const double u = dm_minstd_uniform_fast(x);
        const double q = MULTI ? u : dm_div_recip((double)(uint32_t)k + u, dS, inv_samples);
        const uint64_t T = dm_fx_shift(q, shift);
        const uint64_t t = rs_lower_bound(coarse, 0, ntiles, T);
        uint32_t a;
        if (t == ntiles) {                       // T > C_(n-1)
            a = MULTI ? kRsDropped : (uint32_t)(n - 1);
            ++nover;
        } else {
            const uint64_t b = t * kRsTile, e = b + kRsTile < n ? b + kRsTile : n;
            a = (uint32_t)rs_lower_bound(C, b, e, T);       // < e: C[e - 1] = coarse[t] >= T
        }
        nkeep += a != kRsDropped ? 1u : 0u;
        anc[k] = a;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nkeep += (uint32_t)__shfl_xor((int)nkeep, o, 64);
        nover += (uint32_t)__shfl_xor((int)nover, o, 64);
    }
    if (lane == 0) { s_c[0][wave] = nkeep; s_c[1][wave] = nover; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t ck = 0, co = 0;
        for (int w = 0; w < kWaves; ++w) { ck += s_c[0][w]; co += s_c[1][w]; }
        kept[blockIdx.x] = ck;
        if (co) atomicAdd((unsigned long long*)counter, (unsigned long long)co);
    }
}

// the kept draws' ancestors in draw order: offs is the exclusive prefix of the tiles' counts
__global__ void __launch_bounds__(kBlock) k_rs_compact(uint64_t samples, const uint32_t* __restrict__ anc,
                                                       const uint32_t* __restrict__ offs, uint32_t* __restrict__ out)
{
    __shared__ uint32_t s_w[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kRsTile;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t run = offs[blockIdx.x];
    for (int r = 0; r < kRsItems; ++r) {         // rounds of kBlock consecutive draws, in order
        const uint64_t k = base + (uint64_t)r * kBlock + threadIdx.x;
        const uint32_t a = k < samples ? anc[k] : kRsDropped;
        const bool sel = a != kRsDropped;
        const uint64_t b = __ballot(sel);
        if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pos = run + (uint32_t)__popcll(b & below);
        for (uint32_t w = 0; w < wave; ++w) pos += s_w[w];
        if (sel) out[pos] = a;
        for (int w = 0; w < kWaves; ++w) run += s_w[w];
        __syncthreads();
    }
}

// xi_k.swap(xi_kp) of both resamplers: every field of the ancestor, mprob, the flags and the map
// table's name (copies share it, as after any resample) included.  mprob and the flags are
// carried whatever ESLAM_FLAG_NO_AUX_GATHER says: a set of another size has no old values to keep
__global__ void __launch_bounds__(kBlock) k_rs_gather(DevState s0, DevState s1, const Ctl* __restrict__ ctl, DevState out,
                                                      uint64_t m, const uint32_t* __restrict__ anc, uint32_t set_weight,
                                                      double weight, uint32_t* __restrict__ anc_out)
{
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= m) return;
    const DevState in = ctl->base ? s1 : s0;
    const uint32_t i = anc[k];
    out.x[k] = in.x[i];
    out.y[k] = in.y[i];
    out.th[k] = in.th[i];
    out.z[k] = in.z[i];
    out.zs[k] = in.zs[i];
    out.w[k] = set_weight ? weight : in.w[i];
    out.mprob[k] = in.mprob[i];
    out.flags[k] = in.flags[i];
    if (in.sid) out.sid[k] = in.sid[i];
    if (anc_out) anc_out[k] = i;
}

}  // namespace

extern "C" {

uint64_t eslam_resample_tiles(uint64_t items) { return (items + kRsTile - 1) / kRsTile; }

hipError_t eslam_launch_rs_cumsum(DevState s0, DevState s1, uint64_t n, Ctl* ctl, uint32_t jump_samples, uint64_t* coarse,
                                  uint64_t* C, uint64_t* counter, hipStream_t stream)
{
    const uint64_t tiles = eslam_resample_tiles(n);
    hipLaunchKernelGGL(k_rs_begin, dim3(1), dim3(64), 0, stream, ctl, jump_samples, counter);
    hipLaunchKernelGGL(k_rs_tile_sums, dim3(tiles), dim3(kBlock), 0, stream, s0, s1, n, ctl, coarse);
    hipLaunchKernelGGL(k_rs_scan_u64, dim3(1), dim3(kBlock), 0, stream, coarse, tiles);
    hipLaunchKernelGGL(k_rs_cumsum, dim3(tiles), dim3(kBlock), 0, stream, s0, s1, n, ctl, coarse, C);
    return hipGetLastError();
}

hipError_t eslam_launch_rs_draw(int multinomial, uint64_t n, uint64_t samples, const Ctl* ctl, const uint32_t* jt,
                                const uint64_t* coarse, const uint64_t* C, uint32_t* anc, uint32_t* kept, uint64_t* counter,
                                hipStream_t stream)
{
    const uint64_t tiles = eslam_resample_tiles(samples), ntiles = eslam_resample_tiles(n);
    const double inv = 1.0 / (double)samples;
    if (multinomial)
        hipLaunchKernelGGL(k_rs_draw<true>, dim3(tiles), dim3(kBlock), 0, stream, n, samples, inv, ctl, jt, coarse, ntiles, C, anc,
                           kept, counter);
    else
        hipLaunchKernelGGL(k_rs_draw<false>, dim3(tiles), dim3(kBlock), 0, stream, n, samples, inv, ctl, jt, coarse, ntiles, C, anc,
                           kept, counter);
    return hipGetLastError();
}

hipError_t eslam_launch_rs_compact(uint64_t samples, const uint32_t* anc, const uint32_t* offs, uint32_t* out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_rs_compact, dim3(eslam_resample_tiles(samples)), dim3(kBlock), 0, stream, samples, anc, offs, out);
    return hipGetLastError();
}

hipError_t eslam_launch_rs_gather(DevState s0, DevState s1, const Ctl* ctl, DevState out, uint64_t m, const uint32_t* anc,
                                  int set_weight, double weight, uint32_t* anc_out, hipStream_t stream)
{
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_rs_gather, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, s0, s1, ctl, out, m, anc,
                       set_weight ? 1u : 0u, weight, anc_out);
    return hipGetLastError();
}

}  // extern "C"
