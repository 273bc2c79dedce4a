/* resample_ref.c -- the CPU reference of eslam_gpu_resample_stratified / _multinomial at the
 * level of arrays (tests/resample_ref.py binds it): weights, count, samples, minstd state and
 * shift in; the ancestors of the kept draws, their count, the overruns or dropped draws and the
 * new minstd state out.  Built with the oracle's flags, on the contract's fixed-point
 * cumulative sum (eslam_detmath.h).
 *
 * Stratified is the reference's sequential walk (src/ParticleFilter.hpp:85-108, as the oracle's
 * contract mode restates it): independent of the device's per-draw search.  Multinomial
 * (:120-148) keeps the reference's rule -- the first i with r_n <= sum_i -- but searches the
 * cumulative sum instead of re-summing per draw: O((N + samples) log N).                    */
#include <stdint.h>
#include <stdlib.h>

#include "eslam_detmath.h"

/* the shift of eslam_gpu_resample: 61 - (dm_weight_exp(S) + 1), S the weight sum */
int rr_shift(double S) { return 61 - (dm_weight_exp(S) + 1); }

/* draw k < samples: T_k = fx((k + U_k) / samples); ancestor: the walk's index, clamped to the
 * last particle (Q5, counted).  Returns the kept count (samples).                          */
uint64_t rr_stratified(const double* w, uint64_t n, uint64_t samples, uint32_t* minstd, int shift, uint32_t* anc,
                       uint64_t* overruns)
{
    uint64_t idx = 0, over = 0;
    uint32_t x = *minstd;
    uint64_t sum_w = dm_fx_shift(w[0], shift);
    for (uint64_t k = 0; k < samples; ++k) {
        x = dm_minstd_next(x);
        const double sum_r = ((double)k + dm_minstd_uniform(x)) / (double)samples;
        const uint64_t t = dm_fx_shift(sum_r, shift);
        while (sum_w < t) {
            if (idx + 1 >= n) { over++; break; }
            ++idx;
            sum_w += dm_fx_shift(w[idx], shift);
        }
        anc[k] = (uint32_t)idx;
    }
    *minstd = x;
    *overruns = over;
    return samples;
}

/* draw k: T_k = fx(U_k); ancestor: the first i with T_k <= C_i; none: dropped.  anc receives
 * the kept draws' ancestors in draw order; returns their count.                             */
uint64_t rr_multinomial(const double* w, uint64_t n, uint64_t samples, uint32_t* minstd, int shift, uint32_t* anc,
                        uint64_t* dropped)
{
    uint64_t* C = malloc((n ? n : 1) * sizeof(uint64_t));
    uint64_t run = 0, m = 0, drop = 0;
    for (uint64_t i = 0; i < n; ++i) { run += dm_fx_shift(w[i], shift); C[i] = run; }
    uint32_t x = *minstd;
    for (uint64_t k = 0; k < samples; ++k) {
        x = dm_minstd_next(x);
        const uint64_t t = dm_fx_shift(dm_minstd_uniform(x), shift);
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (C[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        if (lo == n) drop++;
        else anc[m++] = (uint32_t)lo;
    }
    free(C);
    *minstd = x;
    *dropped = drop;
    return m;
}

/* the boost uniforms of the next `count` minstd draws after x (tests count draws with them) */
void rr_uniforms(uint32_t x, uint64_t count, double* out)
{
    for (uint64_t k = 0; k < count; ++k) {
        x = dm_minstd_next(x);
        out[k] = dm_minstd_uniform(x);
    }
}

uint32_t rr_minstd_seed(uint64_t seed) { return dm_minstd_seed(seed); }
