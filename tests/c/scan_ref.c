/*
 * scan_ref.c -- the contract of eslam_gpu_scan_from_laser / eslam_gpu_scan_from_depth as the
 * sequential rule it is defined by (include/eslam_gpu.h), over host arrays: every
 * point in index order, the binned ones sorted by (cell, (float)z, index), every cell's points
 * walked into clusters.  The tests compare the device's patches with these bit for bit.
 *
 * Built with the oracle's flags (-O2 -mfma -ffp-contract=off -fno-fast-math), so the arithmetic
 * of eslam_detmath.h rounds as it does on the device.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "eslam_detmath.h"
#include "eslam_gpu.h"

/* base::removeYaw as the library's host side restates it (Eigen's toRotationMatrix, getYaw) */
static void q_to_mat(const double q[4], double R[9])
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
    R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

static void remove_yaw_mat(const double q[4], double Rw[9])
{
    double R[9];
    q_to_mat(q, R);
    const double x = sqrt(R[8] * R[8] + R[7] * R[7]);
    const double yaw = x > 1e-12 ? atan2(R[3], R[0]) : 0.0;
    const double ha = 0.5 * -yaw;
    const double s = sin(ha);
    const double a[4] = {cos(ha), s * 0.0, s * 0.0, s * 1.0};
    const double w = a[0] * q[0] - a[1] * q[1] - a[2] * q[2] - a[3] * q[3];
    const double qx = a[0] * q[1] + a[1] * q[0] + a[2] * q[3] - a[3] * q[2];
    const double qy = a[0] * q[2] + a[2] * q[0] + a[3] * q[1] - a[1] * q[3];
    const double qz = a[0] * q[3] + a[3] * q[0] + a[1] * q[2] - a[2] * q[1];
    const double yc[4] = {w, qx, qy, qz};
    q_to_mat(yc, Rw);
}

typedef struct {
    uint32_t cell, idx;
    float zf;
    double z, var;
} point;

static int by_cell_z_index(const void* pa, const void* pb)
{
    const point* a = pa;
    const point* b = pb;
    if (a->cell != b->cell) return a->cell < b->cell ? -1 : 1;
    if (a->zf != b->zf) return a->zf < b->zf ? -1 : 1;
    return a->idx < b->idx ? -1 : (a->idx > b->idx ? 1 : 0);
}

static int params_ok(const eslam_scan_params* p)
{
    int fin = 1;
    for (int i = 0; i < 12; ++i) fin = fin && dm_isfinite(p->sensor2body[i]);
    for (int i = 0; i < 4; ++i) fin = fin && dm_isfinite(p->orientation[i]);
    for (int i = 0; i < 3; ++i) fin = fin && dm_isfinite(p->sensor_rot_sigma[i]) && dm_isfinite(p->body_rot_sigma[i]);
    fin = fin && dm_isfinite(p->min_sigma) && dm_isfinite(p->resolution) && dm_isfinite(p->patch_thickness) &&
          dm_isfinite(p->max_sensor_range);
    return fin && p->min_sigma > 0.0 && p->resolution > 0.0 && p->patch_thickness > 0.0 && p->max_sensor_range > 0.0;
}

/* laser (image == NULL) or depth (scan == NULL): the patches to out (up to capacity; info->patches
 * holds the count), and per cluster its number of points to cluster_points (may be NULL; same
 * capacity) so the tests can assert their preconditions                                       */
static int build(const eslam_laser_scan* scan, const eslam_depth_image* image, const eslam_scan_params* p,
                 eslam_scan_patch* out, uint32_t* cluster_points, uint64_t capacity, eslam_scan_info* info)
{
    if (!p || !info || (!out && capacity)) return ESLAM_ERR_INVALID_ARG;
    memset(info, 0, sizeof(*info));
    if (!params_ok(p)) return ESLAM_ERR_INVALID_ARG;
    double ray = 1.0;
    uint64_t n;
    if (image) {
        if (!image->data || !image->width || !image->height) return ESLAM_ERR_INVALID_ARG;
        ray = dm_scan_depth_ray(image->width, image->height, image->scale_x, image->scale_y, image->center_x, image->center_y);
        if (!dm_isfinite(ray)) return ESLAM_ERR_INVALID_ARG;
        n = (uint64_t)image->width * image->height;
    } else {
        if (!scan || (scan->n && !scan->ranges)) return ESLAM_ERR_INVALID_ARG;
        n = scan->n;
    }
    double Rw[9];
    remove_yaw_mat(p->orientation, Rw);
    dm_scan_frame f;
    if (!dm_scan_frame_init(&f, p->sensor2body, Rw, p->sensor_rot_sigma, p->body_rot_sigma, p->min_sigma, p->resolution,
                            p->patch_thickness, p->max_sensor_range, p->max_sensor_range * ray))
        return ESLAM_ERR_INVALID_ARG;
    info->points = n;
    if (!n) return ESLAM_OK;
    point* pts = malloc(n * sizeof(point));
    double* z = malloc(n * sizeof(double));
    double* var = malloc(n * sizeof(double));
    if (!pts || !z || !var) {
        free(pts); free(z); free(var);
        return ESLAM_ERR_OUT_OF_MEMORY;
    }
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; ++i) {
        double q[3];
        int status;
        if (image) {
            const uint32_t v = (uint32_t)(i / image->width), u = (uint32_t)(i % image->width);
            status = dm_scan_depth_point(&f, image->scale_x, image->scale_y, image->center_x, image->center_y, u, v,
                                         image->data[i], q);
        } else {
            status = dm_scan_laser_point(&f, scan->start_angle, scan->angular_resolution, scan->min_range, scan->max_range,
                                         (uint32_t)i, scan->ranges[i], q);
        }
        point pt;
        if (status == DM_SCAN_VALID && !dm_scan_place(&f, q, &pt.z, &pt.var, &pt.cell)) status = DM_SCAN_OUT_OF_RANGE;
        if (status == DM_SCAN_INVALID) info->points_invalid++;
        else if (status == DM_SCAN_OUT_OF_RANGE) info->points_out_of_range++;
        else {
            float zf = (float)pt.z;
            pt.zf = zf == 0.0f ? 0.0f : zf;
            pt.idx = (uint32_t)i;
            pts[m++] = pt;
        }
    }
    info->points_valid = m;
    qsort(pts, m, sizeof(point), by_cell_z_index);
    for (uint64_t j = 0; j < m; ++j) {
        z[j] = pts[j].z;
        var[j] = pts[j].var;
    }
    uint64_t np = 0;
    for (uint64_t j0 = 0; j0 < m;) {
        uint64_t j1 = j0;
        while (j1 < m && pts[j1].cell == pts[j0].cell) ++j1;
        const uint32_t my = pts[j0].cell / f.width, mx = pts[j0].cell % f.width;
        info->cells++;
        for (uint64_t k = j0; k < j1;) {
            const uint32_t len = dm_scan_cluster_len(z + k, (uint32_t)(j1 - k), f.thickness);
            if (np < capacity) {
                double mu, sd;
                dm_scan_cluster_patch(z + k, var + k, len, &mu, &sd);
                out[np].position[0] = dm_scan_cell_centre(&f, mx);
                out[np].position[1] = dm_scan_cell_centre(&f, my);
                out[np].position[2] = mu;
                out[np].stdev = sd;
                if (cluster_points) cluster_points[np] = len;
            }
            ++np;
            k += len;
        }
        j0 = j1;
    }
    info->patches = np;
    free(pts); free(z); free(var);
    return np <= capacity ? ESLAM_OK : ESLAM_ERR_OUT_OF_MEMORY;
}

int scr_from_laser(const eslam_laser_scan* scan, const eslam_scan_params* p, eslam_scan_patch* out, uint32_t* cluster_points,
                   uint64_t capacity, eslam_scan_info* info)
{
    if (!scan) return ESLAM_ERR_INVALID_ARG;
    return build(scan, NULL, p, out, cluster_points, capacity, info);
}

int scr_from_depth(const eslam_depth_image* image, const eslam_scan_params* p, eslam_scan_patch* out, uint32_t* cluster_points,
                   uint64_t capacity, eslam_scan_info* info)
{
    if (!image) return ESLAM_ERR_INVALID_ARG;
    return build(NULL, image, p, out, cluster_points, capacity, info);
}

/* the defaults of eslam_scan_params_default, restated (the tests run without the library too) */
void scr_params_default(double max_sensor_range, eslam_scan_params* p)
{
    memset(p, 0, sizeof(*p));
    p->sensor2body[0] = p->sensor2body[5] = p->sensor2body[10] = 1.0;
    p->orientation[0] = 1.0;
    p->sensor_rot_sigma[0] = 5.0 / 180.0 * M_PI;
    p->body_rot_sigma[0] = p->body_rot_sigma[1] = 3.0 / 180.0 * M_PI;
    p->min_sigma = 1e-3;
    p->resolution = 0.05;
    p->patch_thickness = 0.1;
    p->max_sensor_range = max_sensor_range;
}

/* the contract's sine and cosine (dm_sincos), for the tests' numpy model of the laser beams */
void scr_sincos(double x, double* s, double* c) { dm_sincos(x, s, c); }
