/* kld_ref.c -- sequential CPU restatement of eslam_gpu_kld_count: the occupied
 * bins of the pose lattice over the particles' (x, y, yaw) and the particle count they ask for.
 * A particle's indices, the bound and the clamps are eslam_detmath.h's (dm_kld_*), shared with
 * the library; the box, the bitmap and its population count are restated here as plain loops.
 * Test infrastructure.                                                                      */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "eslam_gpu.h"
#include "eslam_detmath.h"

/* The info of the n particles (x, y, theta, w) as a filter of n particles reports it.  limit:
 * the largest count the resample accepts (2^32 - 2 on one GPU); capacity: that of a filter with
 * per-particle maps, 0 without.  ESLAM_OK, or ESLAM_ERR_UNSUPPORTED with info filled as far as
 * the box when its bins exceed max_bins.                                                    */
int kld_ref_count(const double* x, const double* y, const double* theta, const double* w, uint64_t n, const eslam_kld_params* p,
                  uint64_t limit, uint64_t capacity, eslam_kld_info* info)
{
    memset(info, 0, sizeof(*info));
    const double inv = 1.0 / p->bin_xy;
    int64_t ix0 = 0, ix1 = 0, iy0 = 0, iy1 = 0;
    uint64_t counted = 0, skipped = 0;
    for (uint64_t i = 0; i < n; ++i) {
        int32_t ix, iy;
        uint32_t it;
        if (!dm_kld_index(x[i], y[i], theta[i], w[i], inv, p->theta_bins, &ix, &iy, &it)) {
            ++skipped;
            continue;
        }
        if (!counted || ix < ix0) ix0 = ix;
        if (!counted || ix > ix1) ix1 = ix;
        if (!counted || iy < iy0) iy0 = iy;
        if (!counted || iy > iy1) iy1 = iy;
        ++counted;
    }
    info->particles_counted = counted;
    info->particles_skipped = skipped;
    info->bins[2] = p->theta_bins;
    uint64_t k = 0;
    if (counted) {
        const uint64_t nx = (uint64_t)(ix1 - ix0 + 1), ny = (uint64_t)(iy1 - iy0 + 1);
        info->origin[0] = ix0;
        info->origin[1] = iy0;
        info->bins[0] = nx;
        info->bins[1] = ny;
        uint64_t cells, total;
        if (__builtin_mul_overflow(nx, ny, &cells) || __builtin_mul_overflow(cells, (uint64_t)p->theta_bins, &total) ||
            total > (p->max_bins ? p->max_bins : 1ull << 27))
            return ESLAM_ERR_UNSUPPORTED;
        uint64_t* bits = (uint64_t*)calloc((total + 63) / 64, sizeof(uint64_t));
        if (!bits) return ESLAM_ERR_OUT_OF_MEMORY;
        for (uint64_t i = 0; i < n; ++i) {
            int32_t ix, iy;
            uint32_t it;
            if (!dm_kld_index(x[i], y[i], theta[i], w[i], inv, p->theta_bins, &ix, &iy, &it)) continue;
            const uint64_t bit = ((uint64_t)(iy - iy0) * nx + (uint64_t)(ix - ix0)) * p->theta_bins + it;
            bits[bit >> 6] |= 1ull << (bit & 63);
        }
        for (uint64_t v = 0; v < (total + 63) / 64; ++v) k += (uint64_t)__builtin_popcountll(bits[v]);
        free(bits);
    }
    info->bins_occupied = k;
    info->bound = dm_kld_bound(k, p->epsilon, p->z_quantile);
    if (p->n_max && p->n_max < limit) limit = p->n_max;
    info->samples = dm_kld_samples(info->bound, p->n_min, limit, capacity, n, p->min_change, &info->clamped);
    return ESLAM_OK;
}

/* the bound and the target count alone (the closed forms of tests/test_kld_ref.py) */
double kld_ref_bound(uint64_t k, double epsilon, double z_quantile) { return dm_kld_bound(k, epsilon, z_quantile); }

uint64_t kld_ref_samples(double bound, uint64_t n_min, uint64_t limit, uint64_t capacity, uint64_t n_global, double min_change,
                         uint32_t* clamped)
{
    return dm_kld_samples(bound, n_min, limit, capacity, n_global, min_change, clamped);
}

double kld_ref_inv_2pi(void) { return DM_INV_2PI; }
