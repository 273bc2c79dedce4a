/* gmm_ref.c -- sequential CPU restatement of eslam_gpu_fit_pose_gmm: the 2-D
 * Gaussian mixture over the particles' (x, y), fitted by EM.  The per-particle arithmetic and
 * the M-step are eslam_detmath.h's (dm_gmm_*), shared with the library; the passes' schedule,
 * pass B and the canonical summation order (a lane's rows in order, the wave butterfly, the
 * fixed pairwise tree over the chunks) are restated here.  Test infrastructure.            */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "eslam_gpu.h"
#include "eslam_detmath.h"

typedef struct {
    double cx, cy, amin, h;
    int E, axis;
} gmm_frame;

/* one pass: hard assignment (c == NULL) or the E-step under c; rec = DM_GMM_REC(K) sums */
static void gmm_pass(const double* x, const double* y, const double* w, uint64_t n, uint32_t J, int K, const gmm_frame* f,
                     const dm_gmm_comp* c, double* rec)
{
    const int R = DM_GMM_REC(K);
    const uint64_t csz = 64ull * J;
    uint64_t m = (n + csz - 1) / csz;
    double* a = (double*)calloc((m ? m : 1) * R, sizeof(double));
    double* b = (double*)calloc((m ? m : 1) * R, sizeof(double));
    for (uint64_t ch = 0; ch < m; ++ch) {
        double lane[64][DM_GMM_REC(DM_GMM_MAX)];
        memset(lane, 0, sizeof(lane));
        for (uint32_t l = 0; l < 64; ++l) {
            double* acc = lane[l];
            for (uint32_t j = 0; j < J; ++j) {
                const uint64_t i = ch * csz + 64ull * j + l;
                if (i >= n) continue;
                double xi = x[i], yi = y[i];
                if (xi == 0.0) xi = 0.0;
                if (yi == 0.0) yi = 0.0;
                if (!dm_gmm_valid(xi, yi, w[i])) continue;
                const double wh = dm_ldexp(w[i], -f->E);
                const double xp = xi - f->cx, yp = yi - f->cy;
                if (!c) {
                    const int kk = dm_gmm_hard(f->axis ? yi : xi, f->amin, f->h, K);
                    dm_gmm_add(&acc[6 * kk], wh, xp, yp);
                    acc[6 * K] = acc[6 * K] + wh;
                } else {
                    double r[DM_GMM_MAX];
                    const double ll = dm_gmm_estep(c, K, xp, yp, r);
                    for (int k = 0; k < K; ++k)
                        if (c[k].live) dm_gmm_add(&acc[6 * k], wh * r[k], xp, yp);
                    acc[6 * K] = acc[6 * K] + wh;
                    acc[6 * K + 1] = acc[6 * K + 1] + wh * ll;
                }
            }
        }
        for (int q = 0; q < R; ++q) {
            double v[64], t[64];
            for (int l = 0; l < 64; ++l) v[l] = lane[l][q];
            for (int o = 32; o >= 1; o >>= 1) {
                for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ o];
                memcpy(v, t, sizeof(v));
            }
            a[ch * R + q] = v[0];
        }
    }
    while (m > 1) {
        const uint64_t h = m / 2;
        for (uint64_t i = 0; i < h; ++i)
            for (int q = 0; q < R; ++q) b[i * R + q] = a[(2 * i) * R + q] + a[(2 * i + 1) * R + q];
        if (m & 1)
            for (int q = 0; q < R; ++q) b[h * R + q] = a[(m - 1) * R + q];
        double* s = a; a = b; b = s;
        m = (m + 1) / 2;
    }
    memcpy(rec, a, R * sizeof(double));
    free(a);
    free(b);
}

/* the fit of n particles summed in chunks of dm_chunk_rows_cfg(n, sum_chunk_rows) rows; out:
 * params->components entries; returns an ESLAM_* code */
int gmm_ref_fit(const double* x, const double* y, const double* w, uint64_t n, uint32_t sum_chunk_rows,
                const eslam_gmm_params* params, eslam_gmm_component* out, eslam_gmm_info* info)
{
    if (!params || !out || !info) return ESLAM_ERR_INVALID_ARG;
    if (params->components < 1 || params->components > ESLAM_GMM_MAX_COMPONENTS || !(params->tolerance >= 0.0) ||
        !dm_isfinite(params->min_variance) || !(params->min_variance > 0.0))
        return ESLAM_ERR_INVALID_ARG;
    if (!n) return ESLAM_ERR_NOT_INITIALISED;
    const int K = (int)params->components;
    const uint32_t J = dm_chunk_rows_cfg(n, sum_chunk_rows);
    memset(out, 0, sizeof(*out) * K);
    memset(info, 0, sizeof(*info));
    /* pass B */
    double maxw = 0.0, xmin = 0.0, xmax = 0.0, ymin = 0.0, ymax = 0.0;
    uint64_t used = 0, skipped = 0;
    for (uint64_t i = 0; i < n; ++i) {
        double xi = x[i], yi = y[i];
        if (xi == 0.0) xi = 0.0;
        if (yi == 0.0) yi = 0.0;
        if (!dm_gmm_valid(xi, yi, w[i])) { ++skipped; continue; }
        if (!used) { maxw = w[i]; xmin = xmax = xi; ymin = ymax = yi; }
        maxw = w[i] > maxw ? w[i] : maxw;
        xmin = xi < xmin ? xi : xmin;
        xmax = xi > xmax ? xi : xmax;
        ymin = yi < ymin ? yi : ymin;
        ymax = yi > ymax ? yi : ymax;
        ++used;
    }
    info->particles_used = used;
    info->particles_skipped = skipped;
    if (!used) return ESLAM_OK;
    gmm_frame f;
    f.E = dm_stat_exp(maxw);
    f.cx = 0.5 * xmin + 0.5 * xmax;
    f.cy = 0.5 * ymin + 0.5 * ymax;
    f.axis = (xmax - xmin) >= (ymax - ymin) ? 0 : 1;
    f.amin = f.axis ? ymin : xmin;
    f.h = ((f.axis ? ymax : xmax) - f.amin) / (double)K;

    dm_gmm_comp comp[DM_GMM_MAX];
    memset(comp, 0, sizeof(comp));
    for (int k = 0; k < K; ++k) comp[k].live = 1;
    double rec[DM_GMM_REC(DM_GMM_MAX)];
    gmm_pass(x, y, w, n, J, K, &f, NULL, rec);
    int nlive = dm_gmm_mstep(rec, K, params->min_variance, comp);
    double L = dm_from_bits(0x7ff8000000000000ull), Lprev = L;
    for (uint32_t t = 1; t <= params->max_iterations && nlive > 0; ++t) {
        dm_gmm_comp cur[DM_GMM_MAX];
        memcpy(cur, comp, sizeof(cur));
        gmm_pass(x, y, w, n, J, K, &f, cur, rec);
        L = rec[6 * K + 1] / rec[6 * K];
        nlive = dm_gmm_mstep(rec, K, params->min_variance, comp);
        info->iterations = t;
        if (t >= 2 && dm_fabs(L - Lprev) <= params->tolerance) { info->converged = 1; break; }
        Lprev = L;
    }
    for (int k = 0; k < K; ++k) {
        if (!comp[k].set) continue;
        out[k].weight = comp[k].weight;
        out[k].mean[0] = comp[k].mx + f.cx;
        out[k].mean[1] = comp[k].my + f.cy;
        out[k].cov[0] = comp[k].cxx;
        out[k].cov[1] = comp[k].cxy;
        out[k].cov[2] = comp[k].cyy;
    }
    info->components_live = (uint32_t)nlive;
    for (int k = 0; k < K; ++k) info->live_mask |= comp[k].live ? 1u << k : 0u;
    info->log_likelihood = L;
    info->centre[0] = f.cx;
    info->centre[1] = f.cy;
    info->weight_exp = f.E;
    return ESLAM_OK;
}
