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

// ---------------------------------------------------------------------------------------
// The same resample on a sharded filter (eslam_gpu_resample_stratified_sharded /
// _multinomial_sharded; DESIGN.md 5 "Resample to a count, sharded").  A rank holds C over its own
// shard only; the ranks' totals, all-gathered, give it the slice (off, off + total] of the global
// cumulative sum it owns.  Every rank evaluates every draw's threshold (a jump-ahead and a few
// multiplies, no memory), so all ranks agree on which draws lie beyond the global sum without
// exchanging a word, and none relies on the thresholds' order:
//   k_rss_begin    the shift from the exact global sum; the minstd state is read, not moved (the
//                  host commits it with the new set, so a refused call leaves it alone)
//   k_rss_census   multinomial: the kept draws of every tile of kRsTile draws and the dropped
//                  draws' count; their exclusive prefix (k_scan_excl) numbers the outputs
//   k_rss_route    <false>: the records this rank will send to every rank and will receive (and,
//                  stratified, the overruns); <true>: a draw this rank owns searches its ancestor in the local C
//                  and is written straight into the new shard, or as a Rec for the rank that owns
//                  its output.  A record carries its output's index, so its place among the
//                  records of one destination (a wave's ballot, one atomic add per wave and
//                  destination) changes no result.
//   k_rss_expand   the received records into the new shard
// ---------------------------------------------------------------------------------------
__global__ void k_rss_begin(Ctl* __restrict__ ctl, uint64_t* __restrict__ counter)
{
    if (threadIdx.x < kRsWords) counter[threadIdx.x] = 0;
    if (threadIdx.x != 0) return;
    ctl->scan_shift = 61 - (dm_weight_exp(ctl->S) + 1);
    ctl->minstd_start = ctl->minstd;
}

// the threshold of draw k, as k_rs_draw computes it
template <bool MULTI>
__device__ __forceinline__ uint64_t rss_threshold(uint64_t k, uint32_t x0, const uint32_t* __restrict__ jt, double dS,
                                                  double inv_samples, int shift)
{
    const uint32_t x = dm_mulmod31(jump_pow(jt, k + 1), x0);
    const double u = dm_minstd_uniform_fast(x);
    const double q = MULTI ? u : dm_div_recip((double)(uint32_t)k + u, dS, inv_samples);
    return dm_fx_shift(q, shift);
}

__global__ void __launch_bounds__(kBlock) k_rss_census(RsPlan pl, const Ctl* __restrict__ ctl, const uint32_t* __restrict__ jt,
                                                       uint32_t* __restrict__ kept, uint64_t* __restrict__ counter)
{
    __shared__ uint32_t s_c[kWaves];
    const int shift = ctl->scan_shift;
    const uint32_t x0 = ctl->minstd_start;
    const uint64_t base = (uint64_t)blockIdx.x * kRsTile;
    uint32_t nkeep = 0, ndraw = 0;
    for (int r = 0; r < kRsItems; ++r) {
        const uint64_t k = base + (uint64_t)r * kBlock + threadIdx.x;
        if (k >= pl.samples) break;
        ++ndraw;
        nkeep += rss_threshold<true>(k, x0, jt, 0.0, 0.0, shift) <= pl.gtotal ? 1u : 0u;
    }
    uint32_t ndrop = ndraw - nkeep;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nkeep += (uint32_t)__shfl_xor((int)nkeep, o, 64);
        ndrop += (uint32_t)__shfl_xor((int)ndrop, o, 64);
    }
    if (lane == 0) s_c[wave] = nkeep;
    if (lane == 0 && ndrop) atomicAdd((unsigned long long*)&counter[kRsBeyond], (unsigned long long)ndrop);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t ck = 0;
        for (int w = 0; w < kWaves; ++w) ck += s_c[w];
        kept[blockIdx.x] = ck;
    }
}

// a block takes kRsTile consecutive draws in rounds of kBlock, in order (the multinomial outputs'
// numbers are the kept draws' ranks: offs[tile] + the kept draws before it in the tile)
template <bool MULTI, bool FILL>
__global__ void __launch_bounds__(kBlock) k_rss_route(RsPlan pl, DevState s0, DevState s1, DevState out,
                                                      const Ctl* __restrict__ ctl, const uint32_t* __restrict__ jt,
                                                      const uint64_t* __restrict__ coarse, const uint64_t* __restrict__ C,
                                                      const uint32_t* __restrict__ offs, Rec* __restrict__ send,
                                                      uint32_t* __restrict__ anc_out, uint64_t* __restrict__ counter)
{
    __shared__ uint32_t s_w[kWaves];
    const int shift = ctl->scan_shift;
    const uint32_t x0 = ctl->minstd_start;
    const DevState in = ctl->base ? s1 : s0;
    const double dS = (double)pl.samples;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const uint64_t base = (uint64_t)blockIdx.x * kRsTile;
    const bool last = pl.me == pl.G - 1;
    uint64_t run = MULTI ? offs[blockIdx.x] : 0ull;
    for (int r = 0; r < kRsItems; ++r) {
        const uint64_t k = base + (uint64_t)r * kBlock + threadIdx.x;
        const bool live = k < pl.samples;
        const uint64_t T = live ? rss_threshold<MULTI>(k, x0, jt, dS, pl.inv_samples, shift) : 0ull;
        const bool beyond = live && T > pl.gtotal;
        uint64_t o = k;                          // the draw's output in the new global numbering
        bool keep = live;
        if (MULTI) {
            keep = live && !beyond;
            const uint64_t b = __ballot(keep);
            if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
            __syncthreads();
            o = run + (uint64_t)__popcll(b & below);
            for (uint32_t w = 0; w < wave; ++w) o += s_w[w];
            for (int w = 0; w < kWaves; ++w) run += s_w[w];
            __syncthreads();
        } else if (!FILL) {                      // the overruns, counted once (every rank sees them all)
            const uint64_t b = __ballot(beyond);
            if (lane == 0 && b) atomicAdd((unsigned long long*)&counter[kRsBeyond], (unsigned long long)__popcll(b));
        }
        // the ancestor is this rank's: T in its slice of the sum; a stratified draw beyond the
        // sum takes the last global particle (Q5), the last rank's last
        const bool mine = keep && (beyond ? last : (pl.me == 0 ? T <= pl.total : (T > pl.off && T <= pl.off + pl.total)));
        int d = 0;                               // the rank of the output in the new table
        if (keep)
            while (d < pl.G - 1 && o >= pl.nb[d + 1]) ++d;
        const bool remote = mine && d != pl.me;
        if (!FILL) {                             // this rank's outputs that arrive as records
            const uint64_t b = __ballot(keep && !mine && d == pl.me);
            if (lane == 0 && b) atomicAdd((unsigned long long*)&counter[kRsRecv], (unsigned long long)__popcll(b));
        }
        // a slot among the destination's records: one atomic add per wave and destination
        uint64_t slot = 0;
        uint64_t pending = __ballot(remote);
        while (pending) {
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const int dd = __shfl(d, leader, 64);
            const uint64_t same = __ballot(remote && d == dd);
            uint64_t first = 0;
            if ((int)lane == leader)
                first = atomicAdd((unsigned long long*)&counter[(FILL ? kRsCursor : kRsCount) + dd],
                                  (unsigned long long)__popcll(same));
            first = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(first >> 32), leader, 64) << 32) |
                    (uint32_t)__shfl((int)(uint32_t)first, leader, 64);
            if (remote && d == dd) slot = first + (uint64_t)__popcll(same & below);
            pending &= ~same;
        }
        if (!FILL || !mine) continue;
        uint64_t a;
        if (beyond) {
            a = pl.n - 1;
        } else {
            const uint64_t Tl = T - pl.off;      // rank 0: off = 0
            const uint64_t t = rs_lower_bound(coarse, 0, pl.ntiles, Tl);    // < ntiles: coarse[ntiles - 1] = total >= Tl
            const uint64_t b = t * kRsTile, e = b + kRsTile < pl.n ? b + kRsTile : pl.n;
            a = t < pl.ntiles ? rs_lower_bound(C, b, e, Tl) : pl.n - 1;
            a = a < pl.n ? a : pl.n - 1;
        }
        const double w = pl.set_weight ? pl.weight : in.w[a];
        const uint64_t ol = o - pl.nb[d];        // < nb[d + 1] - nb[d]
        if (!remote) {
            out.x[ol] = in.x[a];
            out.y[ol] = in.y[a];
            out.th[ol] = in.th[a];
            out.z[ol] = in.z[a];
            out.zs[ol] = in.zs[a];
            out.w[ol] = w;
            out.mprob[ol] = in.mprob[a];
            out.flags[ol] = in.flags[a];
            if (anc_out) anc_out[ol] = (uint32_t)(pl.gbase + a);
        } else if (slot < pl.send_off[d + 1] - pl.send_off[d]) {            // the counting pass sized it
            Rec rec;
            rec.x = in.x[a];
            rec.y = in.y[a];
            rec.th = in.th[a];
            rec.z = in.z[a];
            rec.zs = in.zs[a];
            rec.w = w;
            rec.mprob = in.mprob[a];
            rec.lohi = ol;
            rec.src = (uint64_t)in.flags[a] | ((pl.gbase + a) << 8);
            send[pl.send_off[d] + slot] = rec;
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_rss_expand(const Rec* __restrict__ recv, uint64_t nrecv, DevState out, uint64_t n_out,
                                                       uint32_t* __restrict__ anc_out)
{
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nrecv) return;
    const Rec rec = recv[j];
    const uint64_t ol = rec.lohi;
    if (ol >= n_out) return;                     // never: the sender numbers within this shard
    out.x[ol] = rec.x;
    out.y[ol] = rec.y;
    out.th[ol] = rec.th;
    out.z[ol] = rec.z;
    out.zs[ol] = rec.zs;
    out.w[ol] = rec.w;
    out.mprob[ol] = rec.mprob;
    out.flags[ol] = (uint8_t)(rec.src & 0xffu);
    if (anc_out) anc_out[ol] = (uint32_t)(rec.src >> 8);
}

}  // namespace

extern "C" {

hipError_t eslam_launch_rss_cumsum(DevState s0, DevState s1, uint64_t n, Ctl* ctl, uint64_t* coarse, uint64_t* C,
                                   uint64_t* counter, hipStream_t stream)
{
    const uint64_t tiles = eslam_resample_tiles(n);
    hipLaunchKernelGGL(k_rss_begin, dim3(1), dim3(64), 0, stream, ctl, counter);
    hipLaunchKernelGGL(k_rs_tile_sums, dim3(tiles), dim3(kBlock), 0, stream, s0, s1, n, ctl, coarse);
    hipLaunchKernelGGL(k_rs_scan_u64, dim3(1), dim3(kBlock), 0, stream, coarse, tiles);
    hipLaunchKernelGGL(k_rs_cumsum, dim3(tiles), dim3(kBlock), 0, stream, s0, s1, n, ctl, coarse, C);
    return hipGetLastError();
}

hipError_t eslam_launch_rss_census(const RsPlan* pl, const Ctl* ctl, const uint32_t* jt, uint32_t* kept, uint64_t* counter,
                                   hipStream_t stream)
{
    hipLaunchKernelGGL(k_rss_census, dim3(eslam_resample_tiles(pl->samples)), dim3(kBlock), 0, stream, *pl, ctl, jt, kept, counter);
    return hipGetLastError();
}

hipError_t eslam_launch_rss_route(int multinomial, int fill, const RsPlan* pl, DevState s0, DevState s1, DevState out,
                                  const Ctl* ctl, const uint32_t* jt, const uint64_t* coarse, const uint64_t* C,
                                  const uint32_t* offs, void* send, uint32_t* anc_out, uint64_t* counter, hipStream_t stream)
{
    const dim3 grid(eslam_resample_tiles(pl->samples)), block(kBlock);
    Rec* const sr = static_cast<Rec*>(send);
#define ESLAM_RSS(M, F) \
    hipLaunchKernelGGL((k_rss_route<M, F>), grid, block, 0, stream, *pl, s0, s1, out, ctl, jt, coarse, C, offs, sr, anc_out, counter)
    if (multinomial) { if (fill) ESLAM_RSS(true, true); else ESLAM_RSS(true, false); }
    else { if (fill) ESLAM_RSS(false, true); else ESLAM_RSS(false, false); }
#undef ESLAM_RSS
    return hipGetLastError();
}

hipError_t eslam_launch_rss_expand(const void* recv, uint64_t nrecv, DevState out, uint64_t n_out, uint32_t* anc_out,
                                   hipStream_t stream)
{
    if (!nrecv) return hipSuccess;
    hipLaunchKernelGGL(k_rss_expand, dim3((nrecv + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, static_cast<const Rec*>(recv),
                       nrecv, out, n_out, anc_out);
    return hipGetLastError();
}

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
