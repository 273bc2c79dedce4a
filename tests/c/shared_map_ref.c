/*
 * shared_map_ref.c -- the contract of eslam_gpu_shared_map_update as the sequential loop it
 * is defined by (include/eslam_gpu.h), over host arrays: particles in index
 * order, scan patches in scan order, every placed patch against its cell's current list.
 * The tests compare the device's merged grid with this one bit for bit.
 *
 * Built with the oracle's flags (-O2 -mfma -ffp-contract=off -fno-fast-math), so the
 * arithmetic of eslam_detmath.h rounds as it does on the device.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "eslam_detmath.h"
#include "eslam_gpu.h"

typedef struct {
    float* v;                            /* 3 floats per patch: mean, stdev, height */
    uint32_t len, cap;
} cell_list;

static int cell_push(cell_list* c, float mean, float stdev, float height)
{
    if (c->len == c->cap) {
        const uint32_t cap = c->cap ? 2 * c->cap : 4;
        float* v = realloc(c->v, (size_t)cap * 3 * sizeof(float));
        if (!v) return 0;
        c->v = v;
        c->cap = cap;
    }
    c->v[3 * c->len] = mean;
    c->v[3 * c->len + 1] = stdev;
    c->v[3 * c->len + 2] = height;
    c->len++;
    return 1;
}

/* Merges the scan into the grid g once per particle and writes the merged grid's CSR to
 * cell_start_out (width * height + 1), mean_out, stdev_out and height_out (may be NULL; zeros
 * for a grid without heights), each with room for patch_capacity patches.  Returns ESLAM_OK,
 * ESLAM_ERR_INVALID_ARG, or ESLAM_ERR_OUT_OF_MEMORY when the capacity (info->n_patches holds
 * the need) or the host's memory does not suffice.                                        */
int smr_merge(const eslam_mls_grid* g, uint64_t n, const double* x, const double* y, const double* orientation,
              const double* zpos, const double* zsigma, const eslam_scan_patch* sp, uint32_t count,
              uint32_t* cell_start_out, float* mean_out, float* stdev_out, float* height_out, uint64_t patch_capacity,
              eslam_shared_merge_info* info)
{
    if (!g || !g->cell_start || !cell_start_out || !info || (n && (!x || !y || !orientation || !zpos || !zsigma)) ||
        (count && !sp))
        return ESLAM_ERR_INVALID_ARG;
    memset(info, 0, sizeof(*info));
    const uint64_t ncell = (uint64_t)g->width * g->height;
    cell_list* cells = calloc(ncell ? ncell : 1, sizeof(cell_list));
    uint8_t* touched = calloc(ncell ? ncell : 1, 1);
    int rc = ESLAM_OK;
    if (!cells || !touched) rc = ESLAM_ERR_OUT_OF_MEMORY;
    for (uint64_t c = 0; c < ncell && !rc; ++c)
        for (uint32_t q = g->cell_start[c]; q < g->cell_start[c + 1]; ++q)
            if (!cell_push(&cells[c], g->patch_mean[q], g->patch_stdev[q], g->patch_height ? g->patch_height[q] : 0.0f)) {
                rc = ESLAM_ERR_OUT_OF_MEMORY;
                break;
            }
    const double* A = g->global2local;
    static const double id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    int is_id = 1;
    for (int k = 0; k < 12; ++k) is_id &= A[k] == id[k];
    const double inv_x = 1.0 / g->scale_x, inv_y = 1.0 / g->scale_y;
    for (uint64_t i = 0; i < n && !rc && count; ++i) {
        info->particles_done++;
        const double bx = x[i] - g->offset_x, by = y[i] - g->offset_y;
        if (!(dm_isfinite(bx) && dm_isfinite(by) && dm_isfinite(orientation[i]))) {
            info->patches_off_grid += count;          /* a skipped particle places nothing */
            continue;
        }
        double sn, co;
        dm_sincos(orientation[i], &sn, &co);
        const double zvar = zsigma[i] * zsigma[i];
        for (uint32_t k = 0; k < count; ++k) {
            const double wz = sp[k].position[2] + zpos[i];
            uint32_t cell, cm, cn;
            if (is_id) {
                cell = dm_merge_cell_mn(bx, by, co, sn, sp[k].position[0], sp[k].position[1], inv_x, inv_y, g->width,
                                        g->height, &cm, &cn);
                if (cell == 0xffffffffu) { info->patches_off_grid++; continue; }
            } else {
                const double wx = (co * sp[k].position[0] + (-sn) * sp[k].position[1]) + x[i];
                const double wy = (sn * sp[k].position[0] + co * sp[k].position[1]) + y[i];
                const double lx = ((A[0] * wx + A[1] * wy) + A[2] * wz) + A[3];
                const double ly = ((A[4] * wx + A[5] * wy) + A[6] * wz) + A[7];
                const double fm = floor((lx - g->offset_x) * inv_x);
                const double fn = floor((ly - g->offset_y) * inv_y);
                if (!(fm >= 0.0 && fm < (double)g->width && fn >= 0.0 && fn < (double)g->height)) {
                    info->patches_off_grid++;
                    continue;
                }
                cm = (uint32_t)fm;
                cn = (uint32_t)fn;
                cell = cn * g->width + cm;
            }
            const double var = sp[k].stdev * sp[k].stdev + zvar;
            info->patches_placed++;
            if (!touched[cell]) {
                touched[cell] = 1;
                info->cells_touched++;
            }
            cell_list* c = &cells[cell];
            int taken = 0;
            for (uint32_t q = 0; q < c->len && !taken; ++q) {
                float* p = c->v + 3 * q;
                if (!dm_mls_gate(p[0], p[1], p[2], wz, var)) continue;
                taken = 1;                            /* the first patch that passes takes it */
                float mo, so;
                if (!(p[2] > 0.0f) && dm_lm_fuse(p[0], p[1], wz, var, &mo, &so)) {
                    p[0] = mo;
                    p[1] = so;
                    info->fused++;
                } else {
                    info->absorbed++;                 /* a vertical patch stays as it is */
                }
            }
            if (!taken) {
                if (!cell_push(c, (float)wz, (float)dm_sqrt(var), 0.0f)) { rc = ESLAM_ERR_OUT_OF_MEMORY; break; }
                info->inserted++;
            }
        }
    }
    if (!rc) {
        uint64_t total = 0;
        for (uint64_t c = 0; c < ncell; ++c) total += cells[c].len;
        info->n_patches = total;
        if (total > patch_capacity || total > 0xffffffffull || (total && (!mean_out || !stdev_out))) {
            rc = total > patch_capacity ? ESLAM_ERR_OUT_OF_MEMORY : ESLAM_ERR_INVALID_ARG;
        } else {
            uint32_t at = 0;
            for (uint64_t c = 0; c < ncell; ++c) {
                cell_start_out[c] = at;
                for (uint32_t q = 0; q < cells[c].len; ++q, ++at) {
                    mean_out[at] = cells[c].v[3 * q];
                    stdev_out[at] = cells[c].v[3 * q + 1];
                    if (height_out) height_out[at] = cells[c].v[3 * q + 2];
                }
            }
            cell_start_out[ncell] = at;
        }
    }
    info->runs = 1;
    if (cells)
        for (uint64_t c = 0; c < ncell; ++c) free(cells[c].v);
    free(cells);
    free(touched);
    return rc;
}

size_t smr_info_size(void) { return sizeof(eslam_shared_merge_info); }
