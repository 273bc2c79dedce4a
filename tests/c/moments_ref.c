/* moments_ref.c -- sequential CPU restatement of eslam_gpu_pose_moments: the pose
 * estimate's mean and 4 x 4 covariance over (x, y, z, yaw), optionally of the particles inside a
 * gate ellipse.  The per-particle arithmetic, the mean and the covariance are eslam_detmath.h's
 * (dm_mom_*), shared with the library; pass B, the passes' schedule and the canonical summation
 * order (a lane's rows in order, the wave butterfly, the fixed pairwise tree over the chunks) are
 * restated here.  Also exports dm_atan2 and dm_wrap_pi for tests/test_detmath_atan2.py.
 * Test infrastructure.                                                                      */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "eslam_gpu.h"
#include "eslam_detmath.h"

typedef struct {
    const double *x, *y, *z, *th, *zs, *w;
    uint64_t n;
} cloud;

/* one pass (1 or 2) over the cloud; rec = its R sums */
static void moments_pass(int pass, const cloud* c, uint32_t J, const dm_mom_gate* g, int E, const double* mean, double* rec)
{
    const int R = pass == 1 ? DM_MOM_REC1 : DM_MOM_REC2;
    const uint64_t csz = 64ull * J;
    uint64_t m = (c->n + csz - 1) / csz;
    double* a = (double*)calloc((m ? m : 1) * R, sizeof(double));
    double* b = (double*)calloc((m ? m : 1) * R, sizeof(double));
    for (uint64_t ch = 0; ch < m; ++ch) {
        double lane[64][DM_MOM_REC2];
        memset(lane, 0, sizeof(lane));
        for (uint32_t l = 0; l < 64; ++l) {
            double* acc = lane[l];
            for (uint32_t j = 0; j < J; ++j) {
                const uint64_t i = ch * csz + 64ull * j + l;
                if (i >= c->n) continue;
                if (!dm_mom_valid(c->x[i], c->y[i], c->z[i], c->th[i], c->zs[i], c->w[i])) continue;
                const double wh = dm_ldexp(c->w[i], -E);
                const int inside = dm_mom_inside(g, c->x[i], c->y[i]);
                if (pass == 1) dm_mom_add1(acc, inside, wh, c->x[i], c->y[i], c->z[i], c->th[i], c->zs[i]);
                else if (inside) dm_mom_add2(acc, wh, mean, c->x[i], c->y[i], c->z[i], c->th[i]);
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

/* the moments of n particles summed in chunks of dm_chunk_rows_cfg(n, sum_chunk_rows) rows; gate
 * may be NULL; returns an ESLAM_* code */
int moments_ref(const double* x, const double* y, const double* z, const double* th, const double* zs, const double* w, uint64_t n,
                uint32_t sum_chunk_rows, const eslam_pose_gate* gate, eslam_pose_moments* out)
{
    if (!out) return ESLAM_ERR_INVALID_ARG;
    dm_mom_gate g;
    memset(&g, 0, sizeof(g));
    if (gate && !dm_mom_gate_set(&g, gate->centre, gate->cov, gate->chi2)) return ESLAM_ERR_INVALID_ARG;
    if (!n) return ESLAM_ERR_NOT_INITIALISED;
    const cloud c = {x, y, z, th, zs, w, n};
    const uint32_t J = dm_chunk_rows_cfg(n, sum_chunk_rows);
    memset(out, 0, sizeof(*out));
    /* pass B */
    double maxw = 0.0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!dm_mom_valid(x[i], y[i], z[i], th[i], zs[i], w[i])) { ++out->particles_skipped; continue; }
        maxw = w[i] > maxw ? w[i] : maxw;
        if (dm_mom_inside(&g, x[i], y[i])) ++out->particles_counted;
        else ++out->particles_gated_out;
    }
    if (out->particles_counted + out->particles_gated_out) out->weight_exp = dm_stat_exp(maxw);
    if (!out->particles_counted) return ESLAM_OK;
    double rec[DM_MOM_REC2], q[4];
    moments_pass(1, &c, J, &g, out->weight_exp, NULL, rec);
    dm_mom_mean(rec, out->mean, q);
    moments_pass(2, &c, J, &g, out->weight_exp, out->mean, rec);
    dm_mom_cov(rec, out->cov);
    out->yaw_resultant = q[0];
    out->effective = q[1];
    out->weight_share = q[2];
    out->z_within = q[3];
    return ESLAM_OK;
}

/* dm_atan2 and dm_wrap_pi over arrays */
void moments_ref_atan2(const double* y, const double* x, double* out, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = dm_atan2(y[i], x[i]);
}

void moments_ref_wrap_pi(const double* d, double* out, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = dm_wrap_pi(d[i]);
}

uint64_t moments_ref_sizeof(int which) { return which ? sizeof(eslam_pose_moments) : sizeof(eslam_pose_gate); }
