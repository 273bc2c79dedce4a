// eslam_ctx.hip -- host side of libeslam_gpu: the context's lifecycle, the particles (allocation,
// initialisation, the surface hash, upload, download, records), the whole step and the resamplers
// of the C ABI of include/eslam_gpu.h.  The context itself and what crosses the host files:
// eslam_ctx.h.  The maps and the scan build: eslam_host_map.hip; the estimates (centroid, mixture,
// moments, KLD): eslam_host_stats.hip; snapshots: eslam_host_snapshot.hip; the multi-GPU plumbing:
// eslam_host_comm.hip.
//
// Per-step host work is O(1): the reference's per-step scalar preparation
// (src/PoseEstimator.cpp:186-194: yaw, removeYaw, the odometry z delta and variance,
// the sampler's Cholesky factor; src/ContactModel.cpp:21-41: the yaw-compensated feet) and
// the EmbodiedSlamFilter update gate (src/EmbodiedSlamFilter.cpp:360).  Everything that
// touches particles runs on the GPU; the resample decision is taken on the device, so a
// step is four asynchronous launches with no host round trip.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <chrono>
#include <algorithm>
#include <atomic>
#include <functional>
#include <vector>

#include "eslam_ctx.h"
#include "eslam_scratch.h"

// ---------------------------------------------------------------------------------------
// small Eigen / base-types restatements (host, per step)
// ---------------------------------------------------------------------------------------
namespace eslam_host {

void q_to_mat(const double q[4], double R[9])          // QuaternionBase::toRotationMatrix
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

void q_mul(const double a[4], const double b[4], double r[4])
{
    const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    const double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    const double y = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    const double z = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
    r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}

void q_from_yaw(double angle, double q[4])              // Quaternion(AngleAxis(angle, UnitZ))
{
    const double ha = 0.5 * angle;
    q[0] = cos(ha);
    const double s = sin(ha);
    q[1] = s * 0.0; q[2] = s * 0.0; q[3] = s * 1.0;
}

}  // namespace eslam_host

namespace {

void q_rotate(const double q[4], const double v[3], double out[3])   // _transformVector
{
    const double qx = q[1], qy = q[2], qz = q[3], w = q[0];
    double uv[3] = {qy * v[2] - qz * v[1], qz * v[0] - qx * v[2], qx * v[1] - qy * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    const double c[3] = {qy * uv[2] - qz * uv[1], qz * uv[0] - qx * uv[2], qx * uv[1] - qy * uv[0]};
    out[0] = (v[0] + w * uv[0]) + c[0];
    out[1] = (v[1] + w * uv[1]) + c[1];
    out[2] = (v[2] + w * uv[2]) + c[2];
}

double get_yaw(const double q[4])                        // base::getYaw (getEuler()[0])
{
    double R[9];
    q_to_mat(q, R);
    const double x = sqrt(R[8] * R[8] + R[7] * R[7]);
    return x > 1e-12 ? atan2(R[3], R[0]) : 0.0;
}

}  // namespace

void eslam_host::remove_yaw(const double q[4], double out[4])       // base::removeYaw
{
    double a[4];
    q_from_yaw(-get_yaw(q), a);
    q_mul(a, q, out);
}

namespace {

void q_from_mat(const double m[9], double q[4])          // Eigen quaternion from 3x3
{
    double t = m[0] + m[4] + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (m[7] - m[5]) * t;
        q[2] = (m[2] - m[6]) * t;
        q[3] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
        double v[3];
        v[i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[k * 3 + j] - m[j * 3 + k]) * t;
        v[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        v[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
        q[1] = v[0]; q[2] = v[1]; q[3] = v[2];
    }
}

// UpdateThreshold::test(udPose.inverse() * body2odometry)  src/Configuration.hpp:18-26 (Q6)
bool update_gate(double thr_distance, double thr_angle, const double ud[12], const double q_b[4], const double t_b[3])
{
    double Rb[9];
    q_to_mat(q_b, Rb);
    const double Ri[9] = {ud[0], ud[4], ud[8], ud[1], ud[5], ud[9], ud[2], ud[6], ud[10]};
    double ti[3], L[9], t[3];
    for (int r = 0; r < 3; ++r) ti[r] = -((Ri[r * 3 + 0] * ud[3] + Ri[r * 3 + 1] * ud[7]) + Ri[r * 3 + 2] * ud[11]);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
            L[r * 3 + c] = (Ri[r * 3 + 0] * Rb[0 * 3 + c] + Ri[r * 3 + 1] * Rb[1 * 3 + c]) + Ri[r * 3 + 2] * Rb[2 * 3 + c];
        t[r] = ((Ri[r * 3 + 0] * t_b[0] + Ri[r * 3 + 1] * t_b[1]) + Ri[r * 3 + 2] * t_b[2]) + ti[r];
    }
    double q[4];
    q_from_mat(L, q);
    const double n = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double angle = n != 0.0 ? 2.0 * atan2(n, fabs(q[0])) : 0.0;
    const double dist = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    return angle > thr_distance || dist > thr_angle;
}

void lower_cholesky(const double S[9], double L[9])
{
    memset(L, 0, 9 * sizeof(double));
    for (int j = 0; j < 3; ++j) {
        double d = S[j * 3 + j];
        for (int k = 0; k < j; ++k) d -= L[j * 3 + k] * L[j * 3 + k];
        const double ljj = d > 0.0 ? sqrt(d) : 0.0;
        L[j * 3 + j] = ljj;
        for (int i = j + 1; i < 3; ++i) {
            double s = S[i * 3 + j];
            for (int k = 0; k < j; ++k) s -= L[i * 3 + k] * L[j * 3 + k];
            L[i * 3 + j] = ljj > 0.0 ? s / ljj : 0.0;
        }
    }
}

void set_translation_pose(double ud[12], double x, double y, double z)
{
    memset(ud, 0, 12 * sizeof(double));
    ud[0] = ud[5] = ud[10] = 1.0;
    ud[3] = x; ud[7] = y; ud[11] = z;
}

}  // namespace

static ProcessStatics& process_statics()
{
    static ProcessStatics ps;
    return ps;
}
// sharded contexts of this process with the flag: at most one.  Ranks driven from one process
// would advance the shared counter once each per step and draw each other's rand() values, so
// their respawns and hash indices would disagree (eslam_gpu_set_comm refuses a second one)
std::atomic<int> eslam_host::g_statics_sharded{0};

// timing mode (EventRing): event k (0..4) of the current step
static void rec(eslam_ctx* ctx, int k) { ctx->ring.record(ctx->timing, k, ctx->stream); }

extern "C" int eslam_gpu_abi_version(void) { return ESLAM_ABI_VERSION; }

#ifndef ESLAM_BUILD_ID
#define ESLAM_BUILD_ID "unknown"
#endif
// SHA-256 of the sources, headers and flags this library was compiled from (build_lib.py)
extern "C" const char* eslam_gpu_build_id(void) { return ESLAM_BUILD_ID; }

extern "C" void eslam_config_default(eslam_config* c)
{
    memset(c, 0, sizeof(*c));
    c->seed = 42;
    c->particle_count = 250;
    c->min_effective = 50;
    c->initial_rotation_error[2] = 0.1;
    c->initial_translation_error[0] = 0.1;
    c->initial_translation_error[1] = 0.1;
    c->initial_translation_error[2] = 1.0;
    c->measurement_error = 0.1;
    c->discount_factor = 0.9;
    c->spread_threshold = 0.9;
    c->spread_translation_factor = 0.1;
    c->spread_rotation_factor = 0.05;
    c->slip_factor = 0.05;
    c->max_yaw_deviation = 15 * M_PI / 180.0;
    c->measurement_threshold_distance = 0.1;
    c->measurement_threshold_angle = 10 * M_PI / 180.0;
    c->use_slip_update = 0;
    c->use_shape_update = 1;
    c->min_contacts = 3;
    c->contact_likelihood_correction = 0.33;
    c->contact_point_radius = 0.01;
    c->hash_use = 0;
    c->hash_period = 10;
    c->hash_percentage = 0.05;
    c->hash_avg_factor = 0.1;
    c->hash_slope_bins = 20;
    c->hash_angular_steps = 16;
    c->log_debug = 0;
    c->flags = 0;
    c->local_map_pages = 0;
    c->max_sensor_range = 3.0;
    c->local_map_trail = 16;
}

extern "C" const char* eslam_gpu_last_error(const eslam_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

static int store_receive(eslam_ctx* ctx);

static const char* kPoisonMsg =
    "resample scan: a cross-block wait gave up (a preceding tile's total or the finalize never arrived); "
    "the particle set is undefined until the filter is re-initialised";

// a device wait that gave up poisons the filter (kFaultTimeout): seen here from the
// host-mapped word without a synchronisation, so the next call after the faulting launch
// fails instead of building on a corrupt particle set
static const char* kPagesMsg =
    "per-particle maps: the page pool cannot hold a map update's pages even after a collection "
    "(raise eslam_config.local_map_pages); the particle set is undefined until the filter is re-initialised";

static int poison_fail(eslam_ctx* ctx)
{
    return ctx->poison_pages ? fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, kPagesMsg) : fail(ctx, ESLAM_ERR_HIP, kPoisonMsg);
}

int eslam_host::check_poisoned(eslam_ctx* ctx)
{
    if (!ctx->poisoned) {
        const uint32_t f = __atomic_load_n(ctx->fault_host.get(), __ATOMIC_ACQUIRE);
        if (f & (kFaultTimeout | kFaultPages)) {
            ctx->poisoned = true;
            ctx->poison_pages = (f & kFaultPages) != 0;
        }
    }
    return ctx->poisoned ? poison_fail(ctx) : ESLAM_OK;
}

int eslam_host::read_ctl(eslam_ctx* ctx)
{
    HIPCHK(ctx, hipMemcpyAsync(ctx->ctl_host, ctx->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ESLAM_OK;
}

int eslam_host::write_ctl(eslam_ctx* ctx)
{
    HIPCHK(ctx, hipMemcpyAsync(ctx->ctl, ctx->ctl_host, sizeof(Ctl), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ESLAM_OK;
}

extern "C" int eslam_gpu_create(const eslam_config* cfg, int device, eslam_ctx** out)
{
    if (!cfg || !out) return ESLAM_ERR_INVALID_ARG;
    *out = nullptr;
    eslam_ctx* ctx = new eslam_ctx();
    ctx->cfg = *cfg;
    ctx->device = device;
    set_translation_pose(ctx->ud_pose, 1000, 0, 0);
    int rc = ESLAM_OK;
    do {
        // nD <= 64 J and the contact points <= ESLAM_MAX_CONTACTS nD share one 32-bit word (K1)
        if (cfg->sum_chunk_rows > ESLAM_SUM_CHUNK_ROWS_MAX) { rc = fail(ctx, ESLAM_ERR_INVALID_ARG, "sum_chunk_rows: at most 31"); break; }
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) { ctx->err = std::string("hipSetDevice: ") + hipGetErrorString(e); rc = ESLAM_ERR_HIP; break; }
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(ctx, ESLAM_ERR_HIP, "stream"); break; }
        ctx->own_stream = true;
        if (ctx->shards.alloc(sizeof(Shard) * kNShard) != hipSuccess ||
            ctx->ctl.alloc(sizeof(Ctl)) != hipSuccess ||
            ctx->ctl_host.alloc(sizeof(Ctl)) != hipSuccess ||
            ctx->jump.alloc(sizeof(uint32_t) * (2048 + 2048 + 1024)) != hipSuccess ||
            ctx->scratch.alloc(4096) != hipSuccess ||
            ctx->scratch_host.alloc(4096) != hipSuccess ||
            ctx->fault_host.alloc(64) != hipSuccess) {
            rc = fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "device allocation failed");
            break;
        }
        if (hipMemset(ctx->shards, 0, sizeof(Shard) * kNShard) != hipSuccess) { rc = fail(ctx, ESLAM_ERR_HIP, "shard reset"); break; }
        memset(ctx->ctl_host, 0, sizeof(Ctl));
        memset(ctx->fault_host, 0, 64);
        ctx->ctl_host->minstd = dm_minstd_seed(cfg->seed);     // ParticleFilter(seed)
        dm_libc_srand(&ctx->libc, 1);                            // the reference never seeds rand()
        if (cfg->flags & ESLAM_FLAG_PROCESS_STATICS) {
            ProcessStatics& ps = process_statics();
            ctx->hash_ev = &ps.hash_event;
            ctx->libcp = &ps.libc;
        } else {
            ctx->hash_ev = &ctx->hash_event;
            ctx->libcp = &ctx->libc;
        }
        ctx->ctl_host->max_weight = 0.0;                         // PoseEstimator ctor
        ctx->ctl_host->wexp = 1;
        ctx->ctl_host->scan_shift = 60;
        if (hipMemcpy(ctx->ctl, ctx->ctl_host, sizeof(Ctl), hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(ctx, ESLAM_ERR_HIP, "control block upload");
            break;
        }
        // minstd jump tables
        std::vector<uint32_t> jt(2048 + 2048 + 1024);
        uint32_t a = 1;
        for (int i = 0; i < 2048; ++i) { jt[i] = a; a = dm_mulmod31(a, DM_MINSTD_A); }
        const uint32_t a11 = dm_minstd_pow(1ull << 11);
        a = 1;
        for (int i = 0; i < 2048; ++i) { jt[2048 + i] = a; a = dm_mulmod31(a, a11); }
        const uint32_t a22 = dm_minstd_pow(1ull << 22);
        a = 1;
        for (int i = 0; i < 1024; ++i) { jt[4096 + i] = a; a = dm_mulmod31(a, a22); }
        if (hipMemcpy(ctx->jump, jt.data(), jt.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(ctx, ESLAM_ERR_HIP, "jump table upload");
            break;
        }
        bool ev_ok = true;
        for (auto& e2 : ctx->ev) ev_ok &= e2.create(true) == hipSuccess;
        if (!ev_ok) { rc = fail(ctx, ESLAM_ERR_HIP, "event create"); break; }
        if (hipDeviceSynchronize() != hipSuccess) { rc = fail(ctx, ESLAM_ERR_HIP, "device synchronize"); break; }
    } while (0);
    if (rc != ESLAM_OK) {
        fprintf(stderr, "eslam_gpu_create: %s\n", ctx->err.c_str());
        eslam_gpu_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return ESLAM_OK;
}

// ancestors are kept when asked for, while the trajectory log is enabled (its parents are composed
// from them), and always while contact records are (the records of output i are those of its
// ancestor)
static bool record_contacts(const eslam_ctx* ctx)
{
    return (ctx->cfg.flags & ESLAM_FLAG_RECORD_CONTACTS) || ctx->cfg.log_debug;
}
static bool keep_ancestors(const eslam_ctx* ctx)
{
    return (ctx->cfg.flags & ESLAM_FLAG_RECORD_ANCESTORS) || ctx->traj.on || record_contacts(ctx);
}

static void free_debug(eslam_ctx* ctx)
{
    ctx->dbgb = DebugBufs{};
    ctx->dbg = DebugRec{};
    ctx->dbg_cap = 0;
    ctx->dbg_valid = false;
}

static void free_local_maps(eslam_ctx* ctx)
{
    ctx->lmb = LocalMapBufs{};
    ctx->lm = LocalMaps{};
    ctx->lm_ready = false;
}

void eslam_host::free_particles(eslam_ctx* ctx)
{
    free_debug(ctx);
    free_local_maps(ctx);
    ctx->pt = ParticleBufs{};
    ctx->rs_mem.reset();                     // a resample to a count's scratch goes with the set it was sized for
    ctx->st[0].sid = ctx->st[1].sid = nullptr;
    ctx->n = ctx->cap = 0;
    ctx->has_anc = false;
}

static void free_map(eslam_ctx* ctx)
{
    ctx->grid = GridBufs{};
    ctx->pg_out = GridBufs{};
    ctx->pg_out_cap = ctx->pg_out_cells = 0;
    ctx->map_np = ctx->map_np_cap = 0;
    ctx->has_map = false;
}

extern "C" void eslam_gpu_destroy(eslam_ctx* ctx)
{
    if (!ctx) return;
    // never collective: a deferred exchange still pending is dropped (eslam_gpu_finish is the
    // collective that completes it); destroy may run on an error path of one rank or after the
    // caller's communicator is gone, so it must not wait for the other ranks
    ctx->xpend = false;
    if (ctx->statics_sharded) g_statics_sharded.fetch_sub(1);
    ctx->statics_sharded = false;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->xstream) { (void)hipStreamSynchronize(ctx->xstream); (void)hipStreamDestroy(ctx->xstream); }
    rccl_release(ctx);
    // every buffer and event goes with the context, the context's own stream after them
    hipStream_t own = ctx->own_stream ? ctx->stream : nullptr;
    delete ctx;
    if (own) (void)hipStreamDestroy(own);
}

// collective on a sharded filter (every rank calls it at the same point): completes the last
// update's deferred exchange if this rank still owes it; a no-op otherwise
extern "C" int eslam_gpu_finish(eslam_ctx* ctx)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (ctx->poisoned) { ctx->xpend = false; return ESLAM_OK; }
    if (const int rc_ = settle(ctx)) return rc_;
    if (ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ESLAM_OK;
}

extern "C" int eslam_gpu_set_stream(eslam_ctx* ctx, void* s)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (s) {
        if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
        ctx->stream = (hipStream_t)s;
        ctx->own_stream = false;
    }
    return ESLAM_OK;
}

// The particle buffers of one capacity and what points into them: the two state buffers'
// arrays, the fused finalize's epoch word and the tile words' stride
struct ParticleSet {
    ParticleBufs pt;
    DevState st[2] = {};
    uint64_t* fin_word = nullptr;
    uint32_t pub_stride = 0;
};

// 256-byte aligned SoA carve-out: 7 fp64 arrays + 1 byte array, two copies; and everything
// else sized by the capacity.  Fills `ps` only: a failure leaves the context as it was.
static hipError_t alloc_particle_set(const eslam_ctx* ctx, uint64_t cap, ParticleSet& ps)
{
#define ESLAM_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)
    auto carve = [&](Carver& c) {
        for (int k = 0; k < 2; ++k) {
            DevState& s = ps.st[k];
            double** f[7] = {&s.x, &s.y, &s.th, &s.z, &s.zs, &s.w, &s.mprob};
            for (int j = 0; j < 7; ++j) *f[j] = c.take<double>(cap);
            s.flags = c.take<uint8_t>(cap);
        }
    };
    Carver size(nullptr);
    carve(size);
    ESLAM_TRY(ps.pt.state_mem.alloc(size.bytes()));
    Carver place(ps.pt.state_mem.get());
    carve(place);
    const uint64_t ntiles = (cap + kBlock - 1) / kBlock;                // the smallest scan tile (scan_items)
    ESLAM_TRY(ps.pt.marks.alloc(cap * 4));
    ESLAM_TRY(ps.pt.tile_first.alloc(((cap + kRow - 1) / kRow) * 4));
    // the tile words, then (in a line of its own) the fused finalize's epoch word
    // K3's kPubReplicas copies of the tile words (4 KB-aligned regions, 256 B apart beyond
    // that, so the copies fall on different memory channels), then the epoch word's line
    ps.pub_stride = (uint32_t)(((ntiles + 511) & ~511ull) + 32);
    const uint64_t fin_at = (uint64_t)kPubReplicas * ps.pub_stride;
    ESLAM_TRY(ps.pt.tile_sum.alloc((fin_at + 16) * 8));
    ESLAM_TRY(hipMemset(ps.pt.tile_sum, 0, (fin_at + 16) * 8));          // tag / epoch 0: never published
    ps.fin_word = ps.pt.tile_sum + fin_at;
    ESLAM_TRY(hipMemset(ps.pt.marks, 0, cap * 4));
    if (keep_ancestors(ctx)) ESLAM_TRY(ps.pt.anc.alloc(cap * 4));
    if (particle_maps(ctx)) {
        // the table names of both state buffers; the tables and pages come with the map
        // (local_maps_reset: their window size follows the map's cell size)
        ESLAM_TRY(ps.pt.sid_mem.alloc(2 * cap * 4));
        ps.st[0].sid = ps.pt.sid_mem;
        ps.st[1].sid = ps.pt.sid_mem + cap;
        ESLAM_TRY(ps.pt.cow.alloc(cow_words(cap) * 4));
        ESLAM_TRY(ps.pt.merge_cnt.alloc(kMergeCounters * kMergeCounterSlots * sizeof(uint64_t)));
        ESLAM_TRY(hipMemset(ps.pt.merge_cnt, 0, kMergeCounters * kMergeCounterSlots * sizeof(uint64_t)));
    }
    if (ctx->sharded) ESLAM_TRY(ps.pt.range.alloc(cap * sizeof(uint2)));
#undef ESLAM_TRY
    return hipSuccess;
}

// the context takes a particle set over (whatever it held is freed)
static void adopt_particle_set(eslam_ctx* ctx, ParticleSet& ps, uint64_t cap)
{
    ctx->pt = std::move(ps.pt);
    ctx->st[0] = ps.st[0];
    ctx->st[1] = ps.st[1];
    ctx->fin_word = ps.fin_word;
    ctx->pub_stride = ps.pub_stride;
    ctx->cap = cap;
}

int eslam_host::alloc_particles(eslam_ctx* ctx, uint64_t n)
{
    if (n >= (1ull << 32) - 1) return fail(ctx, ESLAM_ERR_INVALID_ARG, "particle count must be < 2^32 - 1");
    if (ctx->sharded && n != ctx->gall[ctx->comm.rank + 1] - ctx->gall[ctx->comm.rank])
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "sharded context: particle count must equal this rank's shard size");
    if (ctx->traj.on && n > ctx->traj.max_particles)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory log: particle count must not exceed its max_particles");
    free_particles(ctx);
    const uint64_t cap = n ? n : 1;
    ParticleSet ps;
    HIPCHK(ctx, alloc_particle_set(ctx, cap, ps));
    adopt_particle_set(ctx, ps, cap);
    ctx->n = n;
    if (!ctx->sharded) {
        ctx->n_global = n;
        ctx->gbase = 0;
    }
    // a new particle set starts the trajectory log over: no lineage leads into it
    if (ctx->traj.on) {
        const int rc = trajectory_reset(ctx);
        if (rc) return rc;
    }
    return local_maps_reset(ctx);
}

// Per-particle maps, sized for the current map and particle count: every
// particle names its own empty table (cloneMaps of the reference's empty grid template,
// src/EmbodiedSlamFilter.cpp:131-134), every page free.  A window of (2h + 1)^2 tiles reaching
// maxSensorRange (dm_lm_half of the cell size); a pool of 2 x cap tables and local_map_pages
// pages per particle.  Runs at particle allocation and at set_map (the tables name cells of
// the map, so a new map starts them over).
int eslam_host::local_maps_reset(eslam_ctx* ctx)
{
    free_local_maps(ctx);
    if (!particle_maps(ctx) || !ctx->has_map || !ctx->n) return ESLAM_OK;
    const double r = ctx->cfg.max_sensor_range;
    if (!(r == r) || r < 0.0 || r > 1e6) return fail(ctx, ESLAM_ERR_INVALID_ARG, "max_sensor_range must be finite and >= 0");
    LocalMaps& lm = ctx->lm;
    LocalMapBufs& b = ctx->lmb;
    lm.hx = dm_lm_half(r, ctx->map_scale[0]);
    lm.hy = dm_lm_half(r, ctx->map_scale[1]);
    lm.wx = 2 * lm.hx + 1;
    lm.wy = 2 * lm.hy + 1;
    if (ctx->cfg.local_map_trail > 4096) return fail(ctx, ESLAM_ERR_INVALID_ARG, "local_map_trail: at most 4096 tiles");
    lm.V = ctx->cfg.local_map_trail;
    // a table's row: the window's W = wx * wy slots, two bookkeeping words (the shadow flag and
    // the trail's high-water mark, the last two words before the trail), padded (NONE) to whole
    // 16-byte words, then the trail's V 16-byte entries.  W is odd: W = 1 (mod 4) when hx and hy
    // have the same parity (every square-cell window), and then ((W + 2 + 3) & ~3) = W + 3 =
    // ((W + 3) & ~3), e.g. 81 -> 84 either way: no such row grows by the two reserved words.
    // W = 3 (mod 4) when the parities differ: padding W alone would leave one word for the two,
    // so the row takes W + 5, e.g. 99 -> 104.
    lm.S = dm_lm_row_words(lm.wx * lm.wy, lm.V);
    lm.mx = lm_magic(lm.wx);
    lm.my = lm_magic(lm.wy);
    lm.bx = lm.wx * (((1u << 29) + lm.wx - 1) / lm.wx);
    lm.by = lm.wy * (((1u << 29) + lm.wy - 1) / lm.wy);
    const uint64_t cap = ctx->cap, pool = store_pool(cap);
    const uint64_t per = ctx->cfg.local_map_pages ? ctx->cfg.local_map_pages : kDefaultMapPages;
    lm.ntables = pool;
    lm.npages = cap * per;
    if (lm.npages >= 0xffffffffull) return fail(ctx, ESLAM_ERR_INVALID_ARG, "per-particle map pool: at most 2^32 - 1 pages");
    const uint64_t ptiles = (lm.npages + kCompactTileItems - 1) / kCompactTileItems;
    HIPCHK(ctx, b.ctr.alloc(pool * sizeof(int2), &lm.ctr));
    HIPCHK(ctx, b.slot.alloc(pool * lm.S * 4, &lm.slot));
    HIPCHK(ctx, b.tgen.alloc(pool * 4, &lm.tgen));
    HIPCHK(ctx, b.page.alloc(lm.npages * DM_LM_PAGE_CELLS * sizeof(float2), &lm.page));
    HIPCHK(ctx, b.owner.alloc(lm.npages * 8, &lm.owner));
    HIPCHK(ctx, b.frees.alloc(lm.npages * 4, &lm.frees));
    HIPCHK(ctx, b.mark.alloc(((lm.npages + 15) / 16) * 16, &lm.mark));
    HIPCHK(ctx, b.off.alloc(cap * 4));
    HIPCHK(ctx, b.job.alloc(cap * sizeof(MergeJob)));
    HIPCHK(ctx, b.codes.alloc(cap * 2 * kScanPartSmall));
    HIPCHK(ctx, b.poff.alloc(((cap + kLmBlock - 1) / kLmBlock + 1) * 4));
    HIPCHK(ctx, b.pgc.alloc((ptiles + 1) * 4));
    HIPCHK(ctx, eslam_launch_store_init(ctx->pt.sid_mem, &lm, cap, pool, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // the free list holds every page (k_store_init: frees[p] = p)
    int rc = read_ctl(ctx);
    if (rc) return rc;
    ctx->ctl_host->pg_cursor = 0;
    ctx->ctl_host->pg_nfree = lm.npages;
    ctx->ctl_host->pg_total = 0;
    ctx->ctl_host->pg_gc = 0;
    rc = write_ctl(ctx);
    if (rc) return rc;
    ctx->lm_ready = true;
    return ESLAM_OK;
}

static PlanParams plan_params(eslam_ctx* ctx)
{
    PlanParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.n_global = ctx->n_global;
    pp.rank = ctx->comm.rank;
    pp.nranks = ctx->comm.nranks;
    for (int r = 0; r <= ctx->comm.nranks; ++r) pp.gbase[r] = ctx->gall[r];
    pp.chunk_sel = ctx->mg + mg::kChunks;
    pp.n_local = ctx->n;
    pp.J = dm_chunk_rows_cfg(ctx->n_global, ctx->cfg.sum_chunk_rows);
    return pp;
}

extern "C" int eslam_gpu_set_map(eslam_ctx* ctx, const eslam_mls_grid* g)
{
    if (!ctx || !g || !g->cell_start || !g->patch_mean || !g->patch_stdev) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (g->width == 0 || g->height == 0) return fail(ctx, ESLAM_ERR_NO_MLS_GRID, "The provided environment does not contain an mls grid.");
    const uint64_t ncell = (uint64_t)g->width * g->height;
    if ((uint64_t)g->cell_start[ncell] != g->n_patches) return fail(ctx, ESLAM_ERR_INVALID_ARG, "cell_start[width*height] != n_patches");
    // a pending resample gather, and on a sharded filter the received maps it names, land in
    // the old pool first; local_maps_reset below then starts every map over, empty
    if (const int rc_ = materialize(ctx)) return rc_;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    free_map(ctx);
    const uint64_t np = g->n_patches ? g->n_patches : 1;
    std::vector<float2> patch(np);
    for (uint64_t k = 0; k < g->n_patches; ++k) patch[k] = make_float2(g->patch_mean[k], g->patch_stdev[k]);
    HIPCHK(ctx, ctx->grid.cells.alloc((ncell + 1) * 4));
    HIPCHK(ctx, ctx->grid.patch.alloc(np * sizeof(float2)));
    HIPCHK(ctx, hipMemcpy(ctx->grid.cells, g->cell_start, (ncell + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->grid.patch, patch.data(), np * sizeof(float2), hipMemcpyHostToDevice));
    if (g->patch_height) {
        HIPCHK(ctx, ctx->grid.height.alloc(np * 4));
        HIPCHK(ctx, hipMemcpy(ctx->grid.height, g->patch_height, g->n_patches * 4, hipMemcpyHostToDevice));
    }
    {
        // one bit per cell: the shared grid holds patches there (the map merge's per-patch test
        // is one 4-byte load instead of the cell's two range words)
        std::vector<uint32_t> occ((ncell + 31) / 32, 0u);
        for (uint64_t c = 0; c < ncell; ++c)
            if (g->cell_start[c] != g->cell_start[c + 1]) occ[c >> 5] |= 1u << (c & 31);
        HIPCHK(ctx, ctx->grid.occ.alloc(occ.size() * 4));
        HIPCHK(ctx, hipMemcpy(ctx->grid.occ, occ.data(), occ.size() * 4, hipMemcpyHostToDevice));
    }
    {
        // MapView::cell_tab: the cell's range and first patch in one 16-byte record
        std::vector<uint4> tab(ncell);
        for (uint64_t c = 0; c < ncell; ++c) {
            const uint32_t b = g->cell_start[c], e = g->cell_start[c + 1];
            const float2 f = e > b ? patch[b] : make_float2(0.0f, 0.0f);
            uint32_t fm, fs;
            memcpy(&fm, &f.x, 4);
            memcpy(&fs, &f.y, 4);
            tab[c] = make_uint4(fm, fs, b, e - b);
        }
        HIPCHK(ctx, ctx->grid.cell_tab.alloc(ncell * sizeof(uint4)));
        HIPCHK(ctx, hipMemcpy(ctx->grid.cell_tab, tab.data(), ncell * sizeof(uint4), hipMemcpyHostToDevice));
    }
    MapView& m = ctx->map;
    m.cell_start = ctx->grid.cells;
    m.occ = ctx->grid.occ;
    m.cell_tab = ctx->grid.cell_tab;
    m.patch = ctx->grid.patch;
    m.height = ctx->grid.height;
    m.has_height = ctx->grid.height ? 1u : 0u;
    ctx->map_np = g->n_patches;
    ctx->map_np_cap = np;
    m.width = g->width;
    m.height_cells = g->height;
    m.inv_scale_x = 1.0 / g->scale_x;
    m.inv_scale_y = 1.0 / g->scale_y;
    ctx->map_scale[0] = g->scale_x;
    ctx->map_scale[1] = g->scale_y;
    ctx->has_hash = false;                   // a new map invalidates the pose hash
    m.offset_x = g->offset_x;
    m.offset_y = g->offset_y;
    memcpy(m.g2l, g->global2local, sizeof(m.g2l));
    static const double kId[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    m.g2l_identity = 1;
    for (int k = 0; k < 12; ++k)
        if (!(g->global2local[k] == kId[k])) m.g2l_identity = 0;
    ctx->has_map = true;
    // per-particle maps name cells of the previous grid: they start over, empty
    return local_maps_reset(ctx);
}

int eslam_host::reset_ctl_for_new_particles(eslam_ctx* ctx, int wexp)
{
    int rc = read_ctl(ctx);
    if (rc) return rc;
    if (ctx->poisoned || (ctx->ctl_host->err & (kFaultTimeout | kFaultPages))) {
        // a poisoned filter starts over: the fault cleared, no partial segment marks left
        ctx->ctl_host->err &= ~(uint64_t)(kFaultTimeout | kFaultPages);
        ctx->poison_pages = false;
        __atomic_store_n(ctx->fault_host.get(), 0u, __ATOMIC_RELAXED);
        HIPCHK(ctx, hipMemsetAsync(ctx->pt.marks, 0, ctx->cap * 4, ctx->stream));
        ctx->poisoned = false;
    }
    ctx->ctl_host->base = 0;
    ctx->ctl_host->flip = 0;
    ctx->ctl_host->gather = 0;               // a pending gather of the old set is dropped
    ctx->ctl_host->wexp = wexp;
    ctx->has_anc = false;
    return write_ctl(ctx);
}

extern "C" int eslam_gpu_init_gaussian(eslam_ctx* ctx, uint64_t n, const double mu[3], const double sigma[3], double zpos,
                                       double zsigma)
{
    if (!ctx || !mu || !sigma) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    int rc = alloc_particles(ctx, n);
    if (rc) return rc;
    rc = reset_ctl_for_new_particles(ctx, 1);
    if (rc) return rc;
    HIPCHK(ctx, eslam_launch_init_gaussian(ctx->st[0], n, ctx->gbase, ctx->cfg.seed, ctx->init_event, mu, sigma, zpos, zsigma,
                                           ctx->stream));
    ctx->init_event++;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_init_pose(eslam_ctx* ctx, const double pos[3], const double q[4])
{
    if (!ctx || !pos || !q) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (!ctx->has_map) return fail(ctx, ESLAM_ERR_NO_MLS_GRID, "The provided environment does not contain an mls grid.");
    double R[9];
    q_to_mat(q, R);
    double angle = atan2(R[3], R[0]);          // eulerAngles(2,1,0)[0], folded into [0, pi]
    if (angle < 0.0) angle += M_PI;
    const double mu[3] = {pos[0], pos[1], angle};
    const double sg[3] = {ctx->cfg.initial_translation_error[0], ctx->cfg.initial_translation_error[1],
                          ctx->cfg.initial_rotation_error[2]};
    uint64_t n = ctx->cfg.particle_count;
    if (ctx->sharded) {
        if (n != ctx->n_global) return fail(ctx, ESLAM_ERR_INVALID_ARG, "sharded context: particle_count must be n_global");
        n = ctx->gall[ctx->comm.rank + 1] - ctx->gall[ctx->comm.rank];
    }
    int rc;
    if (ctx->cfg.hash_use) {                   // hash.create(gridTemplate); filter.init(N, &hash)
        rc = ctx->has_hash ? ESLAM_OK : eslam_gpu_hash_create(ctx);
        if (!rc) rc = eslam_gpu_init_hash(ctx, n);
    } else {
        rc = eslam_gpu_init_gaussian(ctx, n, mu, sg, pos[2], ctx->cfg.initial_translation_error[2] + 1e-3);
    }
    set_translation_pose(ctx->ud_pose, 1000, 0, 0);
    return rc;
}

// ---------------------------------------------------------------------------------------
// SurfaceHash (src/SurfaceHash.hpp:155-231, src/PoseEstimator.cpp:75-86, 130-182)
// ---------------------------------------------------------------------------------------
static dm_hash_grid hash_grid(eslam_ctx* ctx)
{
    dm_hash_grid g;
    memset(&g, 0, sizeof(g));
    g.cell_start = ctx->grid.cells;
    g.mean = ctx->grid.patch.as<const float>();   // float2 {mean, stdev}
    g.mean_stride = 2;
    g.width = ctx->map.width;
    g.height = ctx->map.height_cells;
    g.bins = (uint32_t)ctx->cfg.hash_slope_bins;
    g.scale_x = ctx->map_scale[0];
    g.scale_y = ctx->map_scale[1];
    g.offset_x = ctx->map.offset_x;
    g.offset_y = ctx->map.offset_y;
    g.inv_scale_x = ctx->map.inv_scale_x;
    g.inv_scale_y = ctx->map.inv_scale_y;
    dm_affine_inverse(ctx->map.g2l, g.g2w);
    return g;
}

extern "C" int eslam_gpu_hash_create(eslam_ctx* ctx)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (!ctx->has_map) return fail(ctx, ESLAM_ERR_NO_MLS_GRID, "The provided environment does not contain an mls grid.");
    const uint32_t steps = (uint32_t)ctx->cfg.hash_angular_steps, bins = (uint32_t)ctx->cfg.hash_slope_bins;
    if (steps == 0 || bins == 0 || bins > 4096) return fail(ctx, ESLAM_ERR_INVALID_ARG, "hash_angular_steps / hash_slope_bins");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const dm_hash_grid g = hash_grid(ctx);
    std::vector<double> pts(8 * steps), orient(steps);
    dm_hash_segments(steps, g.g2w, pts.data(), orient.data());
    const uint64_t cells = (uint64_t)g.width * g.height, total = cells * steps;
    Dev<double> d_seg;
    Dev<int32_t> d_out;
    Dev<uint64_t> d_ids;
    std::vector<int32_t> out(total);
    if (d_seg.alloc(sizeof(double) * 9 * steps) != hipSuccess ||
        d_out.alloc(sizeof(int32_t) * (total ? total : 1)) != hipSuccess)
        return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "hash sweep buffers");
    if (hipMemcpy(d_seg, pts.data(), sizeof(double) * 8 * steps, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_seg + 8 * steps, orient.data(), sizeof(double) * steps, hipMemcpyHostToDevice) != hipSuccess ||
        eslam_launch_hash_sweep(&g, d_seg, d_seg + 8 * steps, steps, d_out, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(out.data(), d_out, sizeof(int32_t) * total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return fail(ctx, ESLAM_ERR_HIP, "hash sweep");
    // compact in sweep order; bucket lists by a stable counting sort
    std::vector<uint64_t> ids;
    ctx->hash_bucket.clear();
    for (uint64_t id = 0; id < total; ++id)
        if (out[id] >= 0) { ids.push_back(id); ctx->hash_bucket.push_back(out[id]); }
    const uint64_t n = ids.size();
    const uint32_t nb = bins * bins;
    ctx->hash_bstart.assign(nb + 1, 0);
    for (uint64_t i = 0; i < n; ++i) ctx->hash_bstart[ctx->hash_bucket[i] + 1]++;
    for (uint32_t b = 0; b < nb; ++b) ctx->hash_bstart[b + 1] += ctx->hash_bstart[b];
    std::vector<uint32_t> blist(n ? n : 1), fill(ctx->hash_bstart.begin(), ctx->hash_bstart.end() - 1);
    for (uint64_t i = 0; i < n; ++i) blist[fill[ctx->hash_bucket[i]]++] = (uint32_t)i;
    ctx->d_hash.reset();
    ctx->d_hash_blist.reset();
    const uint64_t cap = n ? n : 1;
    if (ctx->d_hash.alloc(sizeof(double) * 4 * cap) != hipSuccess ||
        ctx->d_hash_blist.alloc(sizeof(uint32_t) * cap) != hipSuccess ||
        d_ids.alloc(sizeof(uint64_t) * cap) != hipSuccess)
        return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "hash pose buffers");
    double* hx = ctx->d_hash;
    if ((n && hipMemcpy(d_ids, ids.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice) != hipSuccess) ||
        (n && hipMemcpy(ctx->d_hash_blist, blist.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice) != hipSuccess) ||
        eslam_launch_hash_poses(&g, d_seg, d_seg + 8 * steps, d_ids, n, hx, hx + cap, hx + 2 * cap, hx + 3 * cap,
                                ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return fail(ctx, ESLAM_ERR_HIP, "hash poses");
    ctx->hash_n = n;
    ctx->has_hash = true;
    return ESLAM_OK;
}

const double* eslam_host::hash_field(eslam_ctx* ctx, int f)
{
    return ctx->d_hash + (uint64_t)f * (ctx->hash_n ? ctx->hash_n : 1);
}

extern "C" int eslam_gpu_init_hash(eslam_ctx* ctx, uint64_t n)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (!ctx->has_hash || ctx->hash_n == 0) return fail(ctx, ESLAM_ERR_HASH_SAMPLE, "could not sample from pose hash.");
    int rc = alloc_particles(ctx, n);
    if (rc) return rc;
    rc = reset_ctl_for_new_particles(ctx, 1);
    if (rc) return rc;
    // rand() % poses.size() per particle, in global particle order (every rank walks all)
    const uint64_t total = ctx->sharded ? ctx->n_global : n, skip = ctx->gbase;
    std::vector<uint32_t> idx(n ? n : 1);
    for (uint64_t gi = 0; gi < total; ++gi) {
        const uint32_t v = (uint32_t)((uint64_t)(uint32_t)dm_libc_rand(ctx->libcp) % ctx->hash_n);
        if (gi >= skip && gi < skip + n) idx[gi - skip] = v;
    }
    Dev<uint32_t> d_idx;
    HIPCHK(ctx, d_idx.alloc(sizeof(uint32_t) * (n ? n : 1)));
    hipError_t e = hipMemcpy(d_idx, idx.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = eslam_launch_init_from_hash(ctx->st[0], d_idx, n, hash_field(ctx, 0), hash_field(ctx, 1), hash_field(ctx, 2),
                                        hash_field(ctx, 3), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    HIPCHK(ctx, e);
    return ESLAM_OK;
}

extern "C" int eslam_gpu_hash_info(eslam_ctx* ctx, uint64_t* n_poses, uint32_t* bucket_sizes)
{
    if (!ctx || !n_poses) return ESLAM_ERR_INVALID_ARG;
    *n_poses = ctx->has_hash ? ctx->hash_n : 0;
    if (bucket_sizes && ctx->has_hash)
        for (size_t b = 0; b + 1 < ctx->hash_bstart.size(); ++b) bucket_sizes[b] = ctx->hash_bstart[b + 1] - ctx->hash_bstart[b];
    return ESLAM_OK;
}

extern "C" int eslam_gpu_hash_poses(eslam_ctx* ctx, double* x, double* y, double* theta, double* z, int32_t* bucket)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (!ctx->has_hash) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no pose hash");
    const uint64_t n = ctx->hash_n;
    double* dst[4] = {x, y, theta, z};
    for (int f = 0; f < 4; ++f)
        if (dst[f] && n) HIPCHK(ctx, hipMemcpy(dst[f], hash_field(ctx, f), n * 8, hipMemcpyDeviceToHost));
    if (bucket && n) memcpy(bucket, ctx->hash_bucket.data(), n * 4);
    return ESLAM_OK;
}

extern "C" int eslam_gpu_particle_count(const eslam_ctx* ctx, uint64_t* n)
{
    if (!ctx || !n) return ESLAM_ERR_INVALID_ARG;
    *n = ctx->n;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_upload_particles(eslam_ctx* ctx, uint64_t n, const eslam_particles* p)
{
    if (!ctx || !p || !p->x || !p->y || !p->orientation || !p->zpos || !p->zsigma || !p->weight) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    int rc = alloc_particles(ctx, n);
    if (rc) return rc;
    const DevState& s = ctx->st[0];
    const uint64_t b = n * 8;
    if (n) {
        HIPCHK(ctx, hipMemcpy(s.x, p->x, b, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(s.y, p->y, b, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(s.th, p->orientation, b, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(s.z, p->zpos, b, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(s.zs, p->zsigma, b, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(s.w, p->weight, b, hipMemcpyHostToDevice));
        if (p->mprob) HIPCHK(ctx, hipMemcpy(s.mprob, p->mprob, b, hipMemcpyHostToDevice));
        else HIPCHK(ctx, hipMemset(s.mprob, 0, b));
        std::vector<uint8_t> fl(n);
        for (uint64_t i = 0; i < n; ++i) {
            const uint8_t f = p->floating ? (p->floating[i] ? 1 : 0) : 1;
            const uint8_t c = p->n_contact_points ? (p->n_contact_points[i] & 0x7f) : 0;
            fl[i] = (uint8_t)(c | (f << 7));
        }
        HIPCHK(ctx, hipMemcpy(s.flags, fl.data(), n, hipMemcpyHostToDevice));
    }
    double mx = 0;
    for (uint64_t i = 0; i < n; ++i) if (p->weight[i] > mx) mx = p->weight[i];
    if (ctx->sharded) {                      // the statistics scale must agree on every rank
        uint64_t* h = ctx->mg_host;
        memcpy(&h[mg::kMaxW], &mx, 8);
        HIPCHK(ctx, hipMemcpy(ctx->mg + mg::kMaxW, &h[mg::kMaxW], 8, hipMemcpyHostToDevice));
        rc = comm_allgather(ctx, ctx->mg + mg::kMaxW, ctx->mg + mg::kMaxWAll, 8);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpy(&h[mg::kMaxWAll], ctx->mg + mg::kMaxWAll, 8 * ctx->comm.nranks, hipMemcpyDeviceToHost));
        for (int r = 0; r < ctx->comm.nranks; ++r) {
            double v;
            memcpy(&v, &h[mg::kMaxWAll + r], 8);
            if (v > mx) mx = v;
        }
    }
    return reset_ctl_for_new_particles(ctx, dm_stat_exp(mx));
}

extern "C" int eslam_gpu_download_particles(eslam_ctx* ctx, eslam_particles* p)
{
    if (!ctx || !p) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (check_poisoned(ctx)) return ESLAM_ERR_HIP;
    int rc = materialize(ctx);
    if (!rc) rc = read_ctl(ctx);
    if (rc) return rc;
    const DevState& s = ctx->st[ctx->ctl_host->base ^ ctx->ctl_host->flip];
    const uint64_t n = ctx->n, b = n * 8;
    if (!n) return ESLAM_OK;
    if (p->x) HIPCHK(ctx, hipMemcpy(p->x, s.x, b, hipMemcpyDeviceToHost));
    if (p->y) HIPCHK(ctx, hipMemcpy(p->y, s.y, b, hipMemcpyDeviceToHost));
    if (p->orientation) HIPCHK(ctx, hipMemcpy(p->orientation, s.th, b, hipMemcpyDeviceToHost));
    if (p->zpos) HIPCHK(ctx, hipMemcpy(p->zpos, s.z, b, hipMemcpyDeviceToHost));
    if (p->zsigma) HIPCHK(ctx, hipMemcpy(p->zsigma, s.zs, b, hipMemcpyDeviceToHost));
    if (p->weight) HIPCHK(ctx, hipMemcpy(p->weight, s.w, b, hipMemcpyDeviceToHost));
    if (p->mprob) HIPCHK(ctx, hipMemcpy(p->mprob, s.mprob, b, hipMemcpyDeviceToHost));
    if (p->floating || p->n_contact_points) {
        std::vector<uint8_t> fl(n);
        HIPCHK(ctx, hipMemcpy(fl.data(), s.flags, n, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; ++i) {
            if (p->floating) p->floating[i] = fl[i] >> 7;
            if (p->n_contact_points) p->n_contact_points[i] = fl[i] & 0x7f;
        }
    }
    return ESLAM_OK;
}

// the largest weight of this context's particles (NaN and negative weights skipped), as
// eslam_gpu_upload_particles computes the weight scale
static int max_weight_local(eslam_ctx* ctx, double* out)
{
    const DevState& s = ctx->st[ctx->ctl_host->base ^ ctx->ctl_host->flip];
    std::vector<double> w(ctx->n);
    HIPCHK(ctx, hipMemcpy(w.data(), s.w, ctx->n * 8, hipMemcpyDeviceToHost));
    double mx = 0;
    for (uint64_t i = 0; i < ctx->n; ++i) if (w[i] > mx) mx = w[i];
    *out = mx;
    return ESLAM_OK;
}

// eslam_gpu_write_particles' rank-local part: the fields of p into [first, first + count)
static int write_particles_local(eslam_ctx* ctx, uint64_t first, uint64_t count, const eslam_particles* p)
{
    if (!count) return ESLAM_OK;
    const DevState& s = ctx->st[ctx->ctl_host->base ^ ctx->ctl_host->flip];
    const uint64_t b = count * 8;
    const double* src[7] = {p->x, p->y, p->orientation, p->zpos, p->zsigma, p->weight, p->mprob};
    double* dst[7] = {s.x, s.y, s.th, s.z, s.zs, s.w, s.mprob};
    for (int k = 0; k < 7; ++k)
        if (src[k]) HIPCHK(ctx, hipMemcpyAsync(dst[k] + first, src[k], b, hipMemcpyHostToDevice, ctx->stream));
    if (p->floating || p->n_contact_points) {
        std::vector<uint8_t> fl(count);
        HIPCHK(ctx, hipMemcpyAsync(fl.data(), s.flags + first, count, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (uint64_t i = 0; i < count; ++i) {
            uint8_t f = fl[i];
            if (p->floating) f = (uint8_t)((f & 0x7f) | ((p->floating[i] ? 1 : 0) << 7));
            if (p->n_contact_points) f = (uint8_t)((f & 0x80) | (p->n_contact_points[i] & 0x7f));
            fl[i] = f;
        }
        HIPCHK(ctx, hipMemcpyAsync(s.flags + first, fl.data(), count, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // the weight scale of the next update, from the largest weight of the whole set exactly
    // as eslam_gpu_upload_particles computes it (one GPU: only when weights were written)
    if (p->weight && !ctx->sharded) {
        double mx = 0;
        const int rc = max_weight_local(ctx, &mx);
        if (rc) return rc;
        ctx->ctl_host->wexp = dm_stat_exp(mx);
        return write_ctl(ctx);
    }
    return ESLAM_OK;
}

extern "C" int eslam_gpu_write_particles(eslam_ctx* ctx, uint64_t first, uint64_t count, const eslam_particles* p)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    // sharded: a collective (every rank calls it, count may be 0).  A rank whose own part fails
    // still takes part in the weight-scale all_gather, with a NaN that tells the others to fail
    // too, so no rank is left waiting in it (include/eslam_gpu.h)
    int rc = (!p || first > ctx->n || count > ctx->n - first) ? fail(ctx, ESLAM_ERR_INVALID_ARG, "write_particles: bad range")
                                                              : ESLAM_OK;
    if (!rc) rc = settle(ctx);                          // a deferred sharded exchange first
    if (!rc) rc = check_poisoned(ctx);
    if (!rc) rc = materialize(ctx);                     // the particles the caller saw: any pending gather done
    if (!rc) rc = read_ctl(ctx);
    if (!rc) rc = write_particles_local(ctx, first, count, p);
    if (!ctx->sharded) return rc;
    double mx = 0;
    if (!rc) rc = max_weight_local(ctx, &mx);
    if (rc) mx = NAN;
    uint64_t* h = ctx->mg_host;
    memcpy(&h[mg::kMaxW], &mx, 8);
    HIPCHK(ctx, hipMemcpy(ctx->mg + mg::kMaxW, &h[mg::kMaxW], 8, hipMemcpyHostToDevice));
    const int crc = comm_allgather(ctx, ctx->mg + mg::kMaxW, ctx->mg + mg::kMaxWAll, 8);
    if (crc) return rc ? rc : crc;
    HIPCHK(ctx, hipMemcpy(&h[mg::kMaxWAll], ctx->mg + mg::kMaxWAll, 8 * ctx->comm.nranks, hipMemcpyDeviceToHost));
    bool peer_failed = false;
    for (int r = 0; r < ctx->comm.nranks; ++r) {
        double v;
        memcpy(&v, &h[mg::kMaxWAll + r], 8);
        if (v != v) peer_failed = true;
        else if (v > mx) mx = v;
    }
    if (rc) return rc;
    if (peer_failed) return fail(ctx, ESLAM_ERR_COMM, "write_particles failed on another rank");
    ctx->ctl_host->wexp = dm_stat_exp(mx);
    return write_ctl(ctx);
}

constexpr uint64_t kRecRemote = 1ull << 63;     // k_pack_records: a slot naming a fetched item

// logDebug records on a sharded filter: particle i's records are those of its ancestor at the
// last update's resample, which may have sat on another rank.  Those are fetched from their
// ranks: the request counts all_gathered, then two all_to_all_v (the global indices asked for,
// the items: meas 4, ncp, maxc x 6 contact-point doubles).  slot[k]: the record's position on
// this rank, or kRecRemote | its item in *d_remote.  Every rank takes part; one whose own part
// failed (rc) sends counts that make every rank fail, so no rank is left waiting.
static int fetch_remote_records(eslam_ctx* ctx, int rc, uint64_t first, uint64_t stride, uint64_t count,
                                std::vector<uint64_t>& slot, Dev<double>* d_remote)
{
    const int G = ctx->comm.nranks, me = ctx->comm.rank;
    const uint64_t gb = ctx->gbase, item = 8ull * (5 + 6ull * (ctx->dbg.maxc ? ctx->dbg.maxc : 1));
    std::vector<std::vector<uint32_t>> req(G);
    std::vector<uint32_t> owner_of;             // per remote slot: its owner
    auto resolve = [&]() -> int {
        if (!ctx->dbg_valid || !count) return ESLAM_OK;
        uint32_t resampled = 0;
        HIPCHK(ctx, hipMemcpy(&resampled, ctx->dbg.resampled, 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> anc;
        if (resampled) {
            anc.resize(ctx->n);
            HIPCHK(ctx, hipMemcpy(anc.data(), ctx->pt.anc, ctx->n * 4, hipMemcpyDeviceToHost));
        }
        slot.resize(count);
        for (uint64_t k = 0; k < count; ++k) {
            const uint64_t i = first + k * stride, g = resampled ? anc[i] : gb + i;
            if (g >= gb && g < gb + ctx->n) {
                slot[k] = g - gb;
                continue;
            }
            const int o = (int)(std::upper_bound(ctx->gall.begin(), ctx->gall.end(), g) - ctx->gall.begin()) - 1;
            if (o < 0 || o >= G || o == me) return fail(ctx, ESLAM_ERR_HIP, "download_records: ancestor outside the filter");
            slot[k] = kRecRemote | req[o].size();
            owner_of.push_back((uint32_t)o);
            req[o].push_back((uint32_t)g);
        }
        return ESLAM_OK;
    };
    if (!rc) rc = resolve();
    // the request counts: row r of the gathered matrix is what rank r asks of each rank
    uint64_t* h = ctx->mg_host;
    for (int d = 0; d < G; ++d) h[mg::kCounts + d] = rc ? ~0ull : (uint64_t)req[d].size();
    HIPCHK(ctx, hipMemcpy(ctx->mg + mg::kCounts, &h[mg::kCounts], 8ull * G, hipMemcpyHostToDevice));
    const int crc = comm_allgather(ctx, ctx->mg + mg::kCounts, ctx->mg + mg::kCountsAll, 8ull * G);
    if (crc) return rc ? rc : crc;
    HIPCHK(ctx, hipMemcpy(&h[mg::kCountsAll], ctx->mg + mg::kCountsAll, 8ull * G * G, hipMemcpyDeviceToHost));
    bool peer_failed = false;
    uint64_t nin[kMaxRanks], tin = 0, tout = 0, off[kMaxRanks + 1];
    for (int r = 0; r < G; ++r) {
        for (int d = 0; d < G; ++d) peer_failed |= h[mg::kCountsAll + r * G + d] == ~0ull;
        nin[r] = h[mg::kCountsAll + r * G + me];
    }
    if (rc) return rc;
    if (peer_failed) return fail(ctx, ESLAM_ERR_COMM, "download_records failed on another rank");
    off[0] = 0;
    for (int r = 0; r < G; ++r) {
        tin += nin[r];
        off[r + 1] = off[r] + req[r].size();
    }
    tout = off[G];
    // the requests out, this rank's items for the others back
    std::vector<uint32_t> hreq;
    hreq.reserve(tout);
    for (int d = 0; d < G; ++d) hreq.insert(hreq.end(), req[d].begin(), req[d].end());
    Dev<uint32_t> d_out, d_in;
    Dev<double> d_items;
    HIPCHK(ctx, d_out.alloc((tout + 1) * 4));
    HIPCHK(ctx, d_in.alloc((tin + 1) * 4));
    HIPCHK(ctx, d_items.alloc((tin + 1) * item));
    HIPCHK(ctx, d_remote->alloc((tout + 1) * item));
    if (tout) HIPCHK(ctx, hipMemcpy(d_out, hreq.data(), tout * 4, hipMemcpyHostToDevice));
    uint64_t sb[kMaxRanks], rb[kMaxRanks];
    for (int r = 0; r < G; ++r) { sb[r] = 4 * req[r].size(); rb[r] = 4 * nin[r]; }
    int e = comm_alltoallv(ctx, d_out, sb, d_in, rb);
    if (e) return e;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (tin && ctx->dbg_valid) HIPCHK(ctx, eslam_launch_gather_records(d_in, tin, gb, &ctx->dbg, d_items, ctx->stream));
    else if (tin) HIPCHK(ctx, hipMemsetAsync(d_items, 0, tin * item, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < G; ++r) { sb[r] = item * nin[r]; rb[r] = item * req[r].size(); }
    e = comm_alltoallv(ctx, d_items, sb, d_remote->get(), rb);
    if (e) return e;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // the fetched items in rank order: rank o's start off[o]
    uint64_t r = 0;
    for (uint64_t k = 0; k < slot.size(); ++k)
        if (slot[k] & kRecRemote) slot[k] = kRecRemote | (off[owner_of[r++]] + (slot[k] & ~kRecRemote));
    return ESLAM_OK;
}

extern "C" int eslam_gpu_download_records(eslam_ctx* ctx, uint64_t first, uint64_t stride, uint64_t count,
                                          eslam_particle_record* out, eslam_cpoint* cpoints, uint32_t max_cpoints)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    // sharded with logDebug records: a collective (every rank calls it; count may be 0)
    const bool coll = ctx->sharded && record_contacts(ctx);
    if (!stride) stride = 1;
    int rc = (!out && count) ? fail(ctx, ESLAM_ERR_INVALID_ARG, "download_records: no output") : ESLAM_OK;
    if (!rc && count && (first >= ctx->n || (count - 1) > (ctx->n - 1 - first) / stride))
        rc = fail(ctx, ESLAM_ERR_INVALID_ARG, "download_records: range beyond the particles");
    if (!rc || coll) {
        const int s = settle(ctx);                // a deferred sharded exchange first
        if (!rc) rc = s;
    }
    if (!rc && check_poisoned(ctx)) rc = ESLAM_ERR_HIP;
    if (!rc) rc = materialize(ctx);               // the pending gather writes the ancestors too
    std::vector<uint64_t> slot;
    Dev<double> d_remote;
    if (coll) {
        const int frc = fetch_remote_records(ctx, rc, first, stride, count, slot, &d_remote);
        if (!rc) rc = frc;
    }
    if (rc || !count) return rc;
    if (!cpoints) max_cpoints = 0;
    const DebugRec none = {};
    const DebugRec& d = ctx->dbg_valid ? ctx->dbg : none;
    Dev<eslam_particle_record> d_out;
    Dev<eslam_cpoint> d_cp;
    Dev<uint64_t> d_slot;
    hipError_t e = d_out.alloc(count * sizeof(eslam_particle_record));
    if (e == hipSuccess && max_cpoints) {
        e = d_cp.alloc(count * max_cpoints * sizeof(eslam_cpoint));
        if (e == hipSuccess) e = hipMemsetAsync(d_cp, 0, count * max_cpoints * sizeof(eslam_cpoint), ctx->stream);
    }
    if (e == hipSuccess && !slot.empty()) {
        e = d_slot.alloc(count * 8);
        if (e == hipSuccess) e = hipMemcpy(d_slot, slot.data(), count * 8, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess)
        e = eslam_launch_pack_records(ctx->st[0], ctx->st[1], ctx->ctl, first, stride, count, ctx->gbase, ctx->pt.anc, &d, d_out,
                                      d_cp, max_cpoints, d_slot, d_remote, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, count * sizeof(eslam_particle_record), hipMemcpyDeviceToHost);
    if (e == hipSuccess && max_cpoints) e = hipMemcpy(cpoints, d_cp, count * max_cpoints * sizeof(eslam_cpoint), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, ESLAM_ERR_HIP, (std::string("download_records: ") + hipGetErrorString(e)).c_str());
    return ESLAM_OK;
}

// the map-update parameters every copy-on-write pass shares (the merge, a sharded receive)
MergeParams eslam_host::merge_params(eslam_ctx* ctx, const CowScratch& cs)
{
    MergeParams mp;
    memset(&mp, 0, sizeof(mp));
    mp.cnt = ctx->pt.merge_cnt;
    mp.ref = cs.ref;
    mp.frees = cs.frees;
    mp.off = ctx->lmb.off;
    mp.job = ctx->lmb.job;
    mp.codes = ctx->lmb.codes;
    mp.poff = ctx->lmb.poff;
    mp.fault = ctx->fault_host;
    mp.n = ctx->n;
    return mp;
}

// ---------------------------------------------------------------------------------------
// the hot path
// ---------------------------------------------------------------------------------------
// the pending resample gather (consumed by the next k_project_weight or materialised)
GatherView eslam_host::gather_view(eslam_ctx* ctx)
{
    GatherView gv;
    memset(&gv, 0, sizeof(gv));
    gv.marks = ctx->pt.marks;
    gv.row_first = ctx->pt.tile_first;
    gv.anc = ctx->pt.anc;
    gv.recs = ctx->sharded ? ctx->recvbuf.as<const Rec>() : nullptr;
    gv.record = keep_ancestors(ctx) ? 1u : 0u;
    gv.multi = ctx->sharded ? 1u : 0u;
    return gv;
}

// before the particle state is read or replaced outside the hot path: run a pending
// gather (device decides; a no-op otherwise) and commit the buffer flip
// cloneMaps (src/PoseEstimator.cpp:31-47) as copy on write: a resample's copies of a particle
// share its store until a map update changes one of them (k_map_merge).  Particles received
// from another rank (sid = kSidRecord | record) get free stores filled from their records'
// payloads before anything reads a store.
static int store_receive(eslam_ctx* ctx)
{
    const SidRef sr{ctx->st[0].sid, ctx->st[1].sid, ctx->ctl};
    const CowScratch cs = cow_layout(ctx->pt.cow, ctx->cap);
    HIPCHK(ctx, eslam_launch_store_refs(sr, ctx->n, store_pool(ctx->cap), &cs, nullptr, ctx->lm.tgen, ctx->stream));
    int rc = grow(ctx, ctx->payoff, (ctx->nrecv_maps + 1) * 4);
    if (!rc) rc = grow(ctx, ctx->rhead, (ctx->nrecv_maps + 1) * 4);
    if (rc) return rc;
    const MergeParams mp = merge_params(ctx, cs);
    HIPCHK(ctx, eslam_launch_store_receive(sr, ctx->ctl, &ctx->lm, &mp, ctx->n, &cs, ctx->recvhdr, ctx->nrecv_maps, ctx->payoff,
                                           ctx->rhead, ctx->recvpay, ctx->lmb.pgc, ctx->stream));
    ctx->cow_pending = false;
    return ESLAM_OK;
}

int eslam_host::materialize(eslam_ctx* ctx)
{
    if (!ctx->n) return ESLAM_OK;
    const GatherView gv = gather_view(ctx);
    const uint32_t aux = (ctx->cfg.flags & ESLAM_FLAG_NO_AUX_GATHER) ? 0u : 1u;
    HIPCHK(ctx, eslam_launch_resample_gather(ctx->st[0], ctx->st[1], ctx->n, ctx->gbase, ctx->ctl, &gv, aux, ctx->stream));
    // a sharded resample handed this rank particles whose stores are still in the received
    // payloads: they get local stores before anything reads a store
    if (ctx->cow_pending) return store_receive(ctx);
    return ESLAM_OK;
}

static void fill_step_params(eslam_ctx* ctx, const eslam_step_input* in, StepParams& p)
{
    memset(&p, 0, sizeof(p));
    const eslam_config& c = ctx->cfg;
    const double* q = in->body2odometry_rot;
    // PoseEstimator::project preamble  src/PoseEstimator.cpp:186-194
    p.yaw = get_yaw(q);
    double R[9];
    q_to_mat(q, R);
    const double* t = in->pose_delta_trans;
    p.z_delta = (R[6] * t[0] + R[7] * t[1]) + R[8] * t[2];
    p.z_var = in->position_error_zz * 2.0;
    for (int i = 0; i < 3; ++i) p.mu[i] = in->sample_mean[i];
    double L[9];
    lower_cholesky(in->sample_cov, L);
    p.L00 = L[0]; p.L10 = L[3]; p.L11 = L[4]; p.L20 = L[6]; p.L21 = L[7]; p.L22 = L[8];
    p.slip_factor = c.slip_factor;
    p.max_yaw_dev = c.max_yaw_deviation;
    p.spread_threshold = c.spread_threshold;
    p.spread_trans = c.spread_translation_factor;
    p.spread_rot = c.spread_rotation_factor;
    p.hash_use = c.hash_use ? 1u : 0u;
    p.seed = c.seed;
    // ContactModel::setContactPoints  src/ContactModel.cpp:21-41
    double yc[4];
    remove_yaw(q, yc);
    memcpy(ctx->zcomp, yc, sizeof(yc));
    const uint32_t m = in->n_contacts < ESLAM_MAX_CONTACTS ? in->n_contacts : ESLAM_MAX_CONTACTS;
    p.m = m;
    uint32_t ends = 0;
    for (uint32_t i = 0; i < m; ++i) {
        double pos[3];
        q_rotate(yc, in->contacts[i].position, pos);
        p.c[i].px = pos[0]; p.c[i].py = pos[1]; p.c[i].pz = pos[2];
        p.c[i].zp = 0.0 * pos[2];
        p.c[i].zz = 0.0 * pos[0] + 0.0 * pos[1];
        p.c[i].eval = !((double)in->contacts[i].contact < 0.2) ? 1u : 0u;
        const int32_t g = in->contacts[i].group_id;
        p.c[i].end = (g == -1 || i + 1 == m || g != in->contacts[i + 1].group_id) ? 1u : 0u;
        ends += p.c[i].end;
        p.eval_mask |= p.c[i].eval << i;
        p.end_mask |= p.c[i].end << i;
    }
    ctx->maxp = ends;
    // LDS window margin: foot reach + mean motion + 6 sigma of the sampled motion + 2 cells
    double reach = 0.0;
    for (uint32_t i = 0; i < m; ++i) {
        const double r = sqrt(p.c[i].px * p.c[i].px + p.c[i].py * p.c[i].py);
        reach = r > reach ? r : reach;
    }
    const double motion = sqrt(p.mu[0] * p.mu[0] + p.mu[1] * p.mu[1]) +
                          6.0 * sqrt(in->sample_cov[0] + in->sample_cov[4]);
    p.win_margin = reach + motion + 0.05;
    p.use_window = (c.flags & ESLAM_FLAG_NO_MAP_LDS) ? 0u : 1u;
    p.me2 = c.measurement_error * c.measurement_error;
    p.radius = c.contact_point_radius;
    p.corr = c.contact_likelihood_correction;
    p.min_contacts = c.min_contacts;
    p.use_shape = c.use_shape_update ? 1u : 0u;
    p.use_slip = c.use_slip_update ? 1u : 0u;
    p.n = ctx->n;
    p.gbase = ctx->gbase;
    p.n_global = ctx->n_global;
    p.J = dm_chunk_rows_cfg(ctx->n_global, ctx->cfg.sum_chunk_rows);
}

// particles per thread of the one-GPU K3: small filters take small tiles so the scan still
// spreads over every CU (256k particles: 1024 blocks instead of 128).  Exact integer tile
// totals: the tile size never changes a result.
static uint32_t scan_items(uint64_t n)
{
    // measured (round-2 A/B, profiles/r02/ab_items_256k_fused.log; bench step at 64k / 256k / 1M / 4M / 16M): 1 item +5 % at
    // 64k and 256k (over 2 items, themselves +19 % over 8 at 256k), 2 or 4 items +4 % at 1M,
    // 8 items best from 4M on (fewer tiles_before re-sums)
    if (n <= (1ull << 18)) return 1u;
    return n <= (1ull << 19) ? 2u : (n <= (2ull << 20) ? 4u : (uint32_t)kScanItems);
}

static ScanParams scan_params(eslam_ctx* ctx, uint32_t phase_b, uint32_t normalize, bool multi)
{
    ScanParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.spin_limit = ctx->spin_limit;
    sp.fault = ctx->fault_host;
    sp.n = ctx->n;
    sp.gbase = ctx->gbase;
    sp.n_global = ctx->n_global;
    sp.phase_b = phase_b;
    sp.normalize = normalize;
    sp.items = multi ? (uint32_t)kScanItems : (ctx->debug_scan_items ? ctx->debug_scan_items : scan_items(ctx->n));
    const uint64_t tile = (uint64_t)kBlock * sp.items;
    sp.ntiles = (uint32_t)((ctx->n + tile - 1) / tile);
    sp.pub_stride = ctx->pub_stride;
    return sp;
}

static FinParams fin_params(eslam_ctx* ctx, uint32_t mode)
{
    FinParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.n_global = ctx->n_global;
    fp.min_effective = ctx->cfg.min_effective;
    fp.discount = ctx->cfg.discount_factor;
    fp.spread_threshold = ctx->cfg.spread_threshold;
    fp.mode = mode;
    if (ctx->jump_n_for != ctx->n_global) {
        ctx->jump_n = dm_minstd_pow(ctx->n_global);
        ctx->jump_n_for = ctx->n_global;
    }
    fp.minstd_jump_n = ctx->jump_n;
    return fp;
}

// multi-GPU update tail:
//   the rank's 16 statistics shards -> all_gather -> every rank finalises the same global
//   scalars from all ranks' shards
//   -> normalise + this rank's fixed-point weight total -> all_gather of the totals
//   -> global stratified segments (outputs in this rank's slice are marked directly),
//      while the host reads the totals and derives every rank's output range (the
//      all_to_all_v sizes: one record per output that lands in another slice)
//   -> pack -> all_to_all_v -> expand; the gather is fused into the next k_project_weight
// a sharded step that fails after k_segments_multi has written own-slice segment marks:
// the marks buffer must be all zero for the next gather (flush_marks stores only segment
// starts) and no gather may stay pending on partial marks, so both are reset before the
// error is returned (the filter keeps the pre-resample particles)
static int abort_pending_gather(eslam_ctx* ctx, hipError_t e, int rc = ESLAM_ERR_HIP)
{
    if (e != hipSuccess) fail(ctx, ESLAM_ERR_HIP, (std::string("sharded resample: ") + hipGetErrorString(e)).c_str());
    (void)hipMemsetAsync(ctx->pt.marks, 0, ctx->cap * 4, ctx->stream);
    (void)hipMemsetAsync(&ctx->ctl->flip, 0, sizeof(uint32_t), ctx->stream);
    (void)hipMemsetAsync(&ctx->ctl->gather, 0, sizeof(uint32_t), ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// host spin bound of the sharded step's wait for the slice totals: the wait starts while the
// step's weighting kernel still runs; a 2 ms bound (which covers K1 + the exchanges of a 4M
// shard) measured the same as 200 us on one rank at 2M and 4M (profiles/r02/ab_spin.log)
constexpr long kSpinBoundUs = 200;

// Per-particle maps on a sharded filter: every record's map travels with it:
// a header per record (its source's table centre and page count), then the pages, each with
// its slot.  The page counts per destination come from the headers' prefix; the receivers learn
// theirs from an all_gather.  The received maps get local tables and pages in store_receive.
static int exchange_maps(eslam_ctx* ctx, uint64_t nsend, uint64_t nrecv, const uint64_t* sb, const uint64_t* rb,
                         const PlanParams& pp, hipStream_t xs)
{
    const int G = ctx->comm.nranks, me = ctx->comm.rank;
    const uint64_t R = eslam_record_bytes(), H = sizeof(MapPayHdr), P = sizeof(MapPayPage);
    int rc = grow(ctx, ctx->sendhdr, (nsend ? nsend : 1) * H);
    if (!rc) rc = grow(ctx, ctx->recvhdr, (nrecv ? nrecv : 1) * H);
    if (!rc) rc = grow(ctx, ctx->payoff, (nsend + nrecv + 2) * 4);
    if (rc) return rc;
    PaySeg seg;
    memset(&seg, 0, sizeof(seg));
    for (int d = 0; d <= G; ++d) seg.off[d] = pp.send_off[d];
    seg.n = G;
    HIPCHK(ctx, eslam_launch_pay_hdr(ctx->st[0], ctx->st[1], ctx->ctl, ctx->sendbuf, nsend, ctx->gbase, &ctx->lm, &seg,
                                     ctx->sendhdr, ctx->payoff, xs));
    // the page counts per destination (records [send_off[d], send_off[d + 1]) go to rank d)
    std::vector<uint32_t> bound(G + 1);
    for (int d = 0; d <= G; ++d)
        HIPCHK(ctx, hipMemcpyAsync(&bound[d], ctx->payoff + pp.send_off[d], 4, hipMemcpyDeviceToHost, xs));
    HIPCHK(ctx, hipStreamSynchronize(xs));
    uint64_t* h = ctx->mg_host;
    uint64_t spg[kMaxRanks], rpg[kMaxRanks], totr = 0;
    for (int d = 0; d < G; ++d) h[mg::kCounts + d] = spg[d] = bound[d + 1] - bound[d];
    HIPCHK(ctx, hipMemcpyAsync(ctx->mg + mg::kCounts, &h[mg::kCounts], 8 * G, hipMemcpyHostToDevice, xs));
    HIPCHK(ctx, hipStreamSynchronize(xs));
    rc = comm_allgather(ctx, ctx->mg + mg::kCounts, ctx->mg + mg::kCountsAll, 8ull * G);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(&h[mg::kCountsAll], ctx->mg + mg::kCountsAll, 8ull * G * G, hipMemcpyDeviceToHost));
    for (int r = 0; r < G; ++r) { rpg[r] = h[mg::kCountsAll + r * G + me]; totr += rpg[r]; }
    rc = grow(ctx, ctx->sendpay, ((uint64_t)bound[G] + 1) * P);
    if (!rc) rc = grow(ctx, ctx->recvpay, (totr + 1) * P);
    if (rc) return rc;
    HIPCHK(ctx, eslam_launch_pay_pack(ctx->st[0], ctx->st[1], ctx->ctl, ctx->sendbuf, nsend, ctx->gbase, &ctx->lm, ctx->sendhdr,
                                      ctx->payoff, ctx->sendpay, xs));
    uint64_t hs[kMaxRanks], hr[kMaxRanks], ps[kMaxRanks], pr[kMaxRanks];
    for (int d = 0; d < G; ++d) {
        hs[d] = sb[d] / R * H; hr[d] = rb[d] / R * H;
        ps[d] = spg[d] * P; pr[d] = rpg[d] * P;
    }
    rc = comm_alltoallv(ctx, ctx->sendhdr, hs, ctx->recvhdr, hr, xs);
    if (!rc) rc = comm_alltoallv(ctx, ctx->sendpay, ps, ctx->recvpay, pr, xs);
    if (rc) return rc;
    ctx->nrecv_maps = nrecv;
    ctx->cow_pending = nrecv > 0;
    return ESLAM_OK;
}

static int exchange_tail(eslam_ctx* ctx, uint64_t epoch, PlanParams& pp, uint64_t* own_lo, uint64_t* own_hi,
                         hipStream_t xs = nullptr, bool* queued = nullptr);

static int run_update_tail_multi(eslam_ctx* ctx, uint32_t mode, bool timed)
{
    const int G = ctx->comm.nranks;
    int rc = comm_allgather(ctx, ctx->shards, ctx->recs, sizeof(Shard) * kNShard);
    if (rc) return rc;
    FinParams fp = fin_params(ctx, mode);
    fp.local_shards = ctx->shards;
    fp.mirror = ctx->mg + mg::kMirror;
    // an update step folds the finalize (over every rank's shards) into K3a's block 0
    const bool fused = mode == FIN_UPDATE;
    if (!fused) HIPCHK(ctx, eslam_launch_finalize(ctx->recs, G * kNShard, ctx->ctl, &fp, ctx->stream));
    if (timed) rec(ctx, 2);
    if (mode == FIN_SUM) return ESLAM_OK;
    ScanParams sp = scan_params(ctx, mode == FIN_UPDATE, mode == FIN_UPDATE || mode == FIN_NORMALIZE, true);
    sp.multi = 1;
    sp.tag = ctx->scan_tag = ctx->scan_tag % 7u + 1u;         // differs from the previous launch's
    const FusedFin ff{ctx->recs, fp, ctx->fin_word, ++ctx->fin_epoch, G * kNShard};
    HIPCHK(ctx, eslam_launch_normalize_scan(ctx->st[0], ctx->st[1], &sp, ctx->ctl, ctx->pt.tile_sum, ctx->mg + mg::kTotal,
                                            fused ? &ff : nullptr, ctx->stream));
    rc = comm_allgather(ctx, ctx->mg + mg::kTotal, ctx->mg + mg::kTotals, 8);
    if (rc) return rc;
    uint64_t* h = ctx->mg_host;
    // the gathered totals and the finalize mirror reach the host without a copy on the
    // stream: the segments kernel's first thread writes them to the host-mapped mg_host and
    // then the launch's epoch (system-scope release)
    PlanParams pp = plan_params(ctx);
    const uint64_t epoch = ++ctx->seg_epoch;
    HIPCHK(ctx, eslam_launch_segments_multi(ctx->st[0], ctx->st[1], &sp, &pp, ctx->ctl, ctx->pt.tile_sum, ctx->pt.marks,
                                            ctx->pt.tile_first, ctx->mg + mg::kTotals, ctx->jump, ctx->pt.range,
                                            ctx->mg + mg::kFirstLast, h + mg::kTotals, h + mg::kHostEpoch, epoch,
                                            ctx->stream));
    if (timed) rec(ctx, 3);
    if (keep_ancestors(ctx)) ctx->has_anc = true;
    // an update defers the exchange to the next call, which first runs the chunks of the rank's
    // own outputs while the host waits for the totals (no particle maps: their stores travel
    // with the records and are placed by the map update)
    if (mode == FIN_UPDATE && !particle_maps(ctx)) {
        if (G > 1) {                         // one rank exchanges nothing: no side stream
            if (!ctx->xstream) {
                HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->xstream, hipStreamNonBlocking));
                HIPCHK(ctx, ctx->ev_seg.create(false));
                HIPCHK(ctx, ctx->ev_x.create(false));
            }
            HIPCHK(ctx, hipEventRecord(ctx->ev_seg, ctx->stream));
        }
        ctx->xpend = true;
        ctx->xpend_epoch = epoch;
        ctx->xpend_pp = pp;
        if (timed) rec(ctx, 4);
        return ESLAM_OK;
    }
    uint64_t own_lo = 0, own_hi = 0;
    rc = exchange_tail(ctx, epoch, pp, &own_lo, &own_hi);
    if (timed) rec(ctx, 4);
    return rc;
}

// The exchange of a sharded resample, after k_segments_multi: wait for the gathered totals
// (host-mapped words the segments kernel writes), derive every rank's output range (the
// all_to_all_v sizes: one record per output that lands in another slice), pack, exchange,
// expand.  own_lo / own_hi: the chunks of this slice holding only its own outputs (the
// segments kernel's PlanParams::chunk_sel, computed alike).
// xs: the stream of the pack / exchange / expand (the context's stream by default; the split
// step's side stream, which waits for ev_seg, overlapping the own chunks' weighting launch)
static int exchange_tail(eslam_ctx* ctx, uint64_t epoch, PlanParams& pp, uint64_t* own_lo, uint64_t* own_hi,
                         hipStream_t xs, bool* queued)
{
    if (!xs) xs = ctx->stream;
    if (queued) *queued = false;
    const int G = ctx->comm.nranks, me = ctx->comm.rank;
    int rc = ESLAM_OK;
    uint64_t* h = ctx->mg_host;
    {
        const uint64_t csz = 64ull * pp.J;
        *own_lo = 0;
        *own_hi = (ctx->n + csz - 1) / csz;
    }
    {
        // spin on the epoch word: a blocking synchronize wakes the thread tens of microseconds
        // late, and the GPU runs dry before the next step's launches if the host is late here
        // (the segments kernel is all it has queued).  Bounded (kSpinBoundUs): past it (a hung
        // collective or kernel, or a late GPU) fall back to a blocking wait instead of burning
        // a host core next to the RCCL proxy threads.
        const auto t0 = std::chrono::steady_clock::now();
        const auto bound = std::chrono::microseconds(kSpinBoundUs);
        while (__atomic_load_n(h + mg::kHostEpoch, __ATOMIC_ACQUIRE) != epoch) {
            if (std::chrono::steady_clock::now() - t0 > bound) {
                const hipError_t q = xs == ctx->stream ? hipStreamSynchronize(xs) : hipEventSynchronize(ctx->ev_seg);
                if (q != hipSuccess) return abort_pending_gather(ctx, q);
                break;
            }
        }
        if (__atomic_load_n(h + mg::kHostEpoch, __ATOMIC_ACQUIRE) != epoch)
            return abort_pending_gather(ctx, hipErrorUnknown);
    }
    // a rank whose slice-total wait gave up all-gathers ~0: every rank stops here
    for (int r = 0; r < G; ++r)
        if (h[mg::kTotals + r] == ~0ull) {
            ctx->poisoned = true;
            (void)abort_pending_gather(ctx, hipSuccess);
            return fail(ctx, ESLAM_ERR_HIP, kPoisonMsg);
        }
    const uint64_t c_resample = h[mg::kMirror];
    const uint32_t c_minstd_start = (uint32_t)h[mg::kMirror + 1];
    const int c_scan_shift = (int)(int64_t)h[mg::kMirror + 2];
    uint64_t nrecv = 0;
    if (c_resample && G > 1) {
        // every rank's outputs [O0_r, O1_r), the same counts the device computes
        const uint64_t N = ctx->n_global;
        uint64_t O0[kMaxRanks], O1[kMaxRanks], off = 0;
        for (int r = 0; r < G; ++r) {
            const uint64_t t = h[mg::kTotals + r];
            O0[r] = r == 0 ? 0 : dm_count_draws_le(off, N, c_minstd_start, c_scan_shift);
            O1[r] = r == G - 1 ? N : dm_count_draws_le(off + t, N, c_minstd_start, c_scan_shift);
            off += t;
        }
        auto overlap = [&](int r, int d) -> uint64_t {
            const uint64_t a = O0[r] > ctx->gall[d] ? O0[r] : ctx->gall[d];
            const uint64_t b = O1[r] < ctx->gall[d + 1] ? O1[r] : ctx->gall[d + 1];
            return b > a ? b - a : 0;
        };
        const uint64_t R = eslam_record_bytes();
        uint64_t sb[kMaxRanks], rb[kMaxRanks], nsend = 0, any = 0;
        pp.send_off[0] = 0;
        for (int d = 0; d < G; ++d) {
            const uint64_t ns = d == me ? 0 : overlap(me, d);
            const uint64_t nr = d == me ? 0 : overlap(d, me);
            pp.sd[d] = O0[me] > ctx->gall[d] ? O0[me] : ctx->gall[d];
            pp.ed[d] = pp.sd[d] + ns;
            pp.send_off[d + 1] = pp.send_off[d] + ns;
            sb[d] = ns * R;
            rb[d] = nr * R;
            nsend += ns;
            nrecv += nr;
            for (int r = 0; r < G; ++r) any |= (r == d ? 0 : overlap(r, d));
        }
        if (any) {
            const bool maps = particle_maps(ctx);
            rc = grow(ctx, ctx->sendbuf, nsend * R);
            if (!rc) rc = grow(ctx, ctx->recvbuf, nrecv * R);
            if (rc) return abort_pending_gather(ctx, hipSuccess, rc);
            // a side stream starts after the segments kernel (its records and ranges)
            if (xs != ctx->stream) HIPCHK(ctx, hipStreamWaitEvent(xs, ctx->ev_seg, 0));
            if (queued) *queued = true;
            const hipError_t e = eslam_launch_pack(ctx->st[0], ctx->st[1], ctx->ctl, &pp, ctx->pt.range, ctx->mg + mg::kFirstLast,
                                                   nsend, ctx->sendbuf, xs);
            if (e != hipSuccess) return abort_pending_gather(ctx, e);
            rc = comm_alltoallv(ctx, ctx->sendbuf, sb, ctx->recvbuf, rb, xs);
            if (!rc && maps) rc = exchange_maps(ctx, nsend, nrecv, sb, rb, pp, xs);
            if (rc) return abort_pending_gather(ctx, hipSuccess, rc);
        } else {
            nrecv = 0;
        }
    }
    if (c_resample) {
        // the own-output chunks (the same function of the same totals as on the device)
        const uint64_t N = ctx->n_global;
        uint64_t off = 0;
        for (int r = 0; r < me; ++r) off += h[mg::kTotals + r];
        const uint64_t O0 = me == 0 ? 0 : dm_count_draws_le(off, N, c_minstd_start, c_scan_shift);
        const uint64_t O1 = me == G - 1 ? N : dm_count_draws_le(off + h[mg::kTotals + me], N, c_minstd_start, c_scan_shift);
        own_chunks(O0, O1, ctx->gbase, ctx->n, pp.J, own_lo, own_hi);
    }
    // marks of the migrated outputs; the gather is fused into the next k_project_weight
    HIPCHK(ctx, eslam_launch_expand(ctx->recvbuf, nrecv, ctx->gbase, ctx->pt.marks, ctx->pt.tile_first, xs));
    return ESLAM_OK;
}

// complete a deferred exchange before anything else reads the particles or the marks
int eslam_host::settle(eslam_ctx* ctx)
{
    if (!ctx->xpend) return ESLAM_OK;
    ctx->xpend = false;
    uint64_t lo = 0, hi = 0;
    return exchange_tail(ctx, ctx->xpend_epoch, ctx->xpend_pp, &lo, &hi);
}

static int run_update_tail(eslam_ctx* ctx, uint32_t mode, bool timed)
{
    if (ctx->sharded) return run_update_tail_multi(ctx, mode, timed);
    const FinParams fp = fin_params(ctx, mode);
    // an update step folds the finalize into K3's block 0 (one launch fewer per step); the
    // standalone normalise / resample / sum keep k_finalize
    const bool fused = mode == FIN_UPDATE;
    if (!fused) HIPCHK(ctx, eslam_launch_finalize(ctx->shards, kNShard, ctx->ctl, &fp, ctx->stream));
    if (timed) rec(ctx, 2);
    ScanParams sp = scan_params(ctx, mode == FIN_UPDATE, mode == FIN_UPDATE || mode == FIN_NORMALIZE, false);
    sp.tag = ctx->scan_tag = ctx->scan_tag % 7u + 1u;         // differs from the previous launch's
    FusedFin ff{ctx->shards, fp, ctx->fin_word, ++ctx->fin_epoch, kNShard};
    HIPCHK(ctx, eslam_launch_normalize_segments(ctx->st[0], ctx->st[1], &sp, ctx->ctl, ctx->pt.tile_sum, ctx->pt.marks,
                                                ctx->pt.tile_first, ctx->jump, fused ? &ff : nullptr, ctx->stream));
    if (timed) rec(ctx, 3);
    // the gather itself is fused into the next k_project_weight (or materialize())
    if (timed) rec(ctx, 4);
    if (keep_ancestors(ctx)) ctx->has_anc = true;
    return ESLAM_OK;
}

// PoseEstimator::sampleFromHash  src/PoseEstimator.cpp:130-182 (after the project kernel)
static int sample_from_hash(eslam_ctx* ctx, const eslam_step_input* in, const StepParams& p)
{
    double pos[3 * ESLAM_MAX_CONTACTS], low[3 * ESLAM_MAX_CONTACTS];
    int32_t grp[ESLAM_MAX_CONTACTS];
    for (uint32_t i = 0; i < p.m; ++i) {                      // setContactPoints: yaw-compensated feet
        pos[3 * i] = p.c[i].px; pos[3 * i + 1] = p.c[i].py; pos[3 * i + 2] = p.c[i].pz;
        grp[i] = in->contacts[i].group_id;
    }
    const uint32_t nlow = dm_lowest_points(pos, grp, p.m, low);  // getLowestPointPerGroup
    double sx, sy;
    dm_surface_param(low, nlow, &sx, &sy);
    const int bins = (int)ctx->cfg.hash_slope_bins;
    const int b = dm_bucket_index(bins, -1.0, 1.0, sx) * bins + dm_bucket_index(bins, -1.0, 1.0, sy);
    const uint32_t bsize = ctx->hash_bstart[b + 1] - ctx->hash_bstart[b];
    const double rel = dm_pow(1.0 - 1.0 * (double)bsize / (double)ctx->hash_n, 3.0);   // getRelevance^3
    const uint64_t N = ctx->n_global;
    uint64_t k = (uint64_t)(((double)N * ctx->cfg.hash_percentage) * rel);
    if (rel < 0.8) k = 0;
    if (k > N) k = N;
    if (k == 0 || bsize == 0) return ESLAM_OK;                // nothing replaced, no rand() drawn
    double S = 0.0;
    int rc = eslam_gpu_get_weights_sum(ctx, &S);
    if (rc) return rc;
    const double weight = ((S / (double)N) * ctx->cfg.hash_avg_factor) * rel;   // getWeightAvg() * avgFactor * rel
    const uint64_t n = ctx->n;
    if (ctx->sort_cap < n) {
        ctx->d_sort.reset(); ctx->sort_cap = 0;
        ctx->sort_tmp.reset(); ctx->sort_tmp_bytes = 0;
        HIPCHK(ctx, ctx->d_sort.alloc(sizeof(uint32_t) * 4 * n));
        size_t bytes = 0;
        HIPCHK(ctx, eslam_hash_sort(ctx->st[0], ctx->st[1], ctx->ctl, n, nullptr, nullptr, nullptr, nullptr, nullptr, &bytes,
                                    ctx->stream));
        HIPCHK(ctx, ctx->sort_tmp.alloc(bytes ? bytes : 1));
        ctx->sort_tmp_bytes = bytes;
        ctx->sort_cap = n;
    }
    uint32_t* keys = ctx->d_sort;
    uint32_t* vals = keys + n;
    uint32_t* keys_out = vals + n;
    uint32_t* order = keys_out + n;
    size_t bytes = ctx->sort_tmp_bytes;
    HIPCHK(ctx, eslam_hash_sort(ctx->st[0], ctx->st[1], ctx->ctl, n, keys, vals, keys_out, order, ctx->sort_tmp, &bytes,
                                ctx->stream));
    // sharded: the global order of the k lowest.  Rank r contributes its min(k, n_r) lowest
    // pairs (any of the k lowest lies among them); every rank sorts the same concatenation.
    const uint32_t* gorder = order;
    if (ctx->sharded) {
        const int G = ctx->comm.nranks, me = ctx->comm.rank;
        std::vector<uint64_t> cnt(G), sb(G), rb(G);
        uint64_t total = 0;
        for (int r = 0; r < G; ++r) {
            const uint64_t nr = ctx->gall[r + 1] - ctx->gall[r];
            cnt[r] = k < nr ? k : nr;
            total += cnt[r];
        }
        for (int d = 0; d < G; ++d) { sb[d] = cnt[me] * 8; rb[d] = cnt[d] * 8; }
        rc = grow(ctx, ctx->hsend, G * cnt[me] * 8 + 8);
        if (!rc) rc = grow(ctx, ctx->hrecv, total * 8 + 8);
        size_t sbytes = 0;
        (void)eslam_radix_sort_pairs(nullptr, nullptr, nullptr, nullptr, total, nullptr, &sbytes, ctx->stream);
        if (!rc) rc = grow(ctx, ctx->hsort, 16 * (total + 1) + sbytes);
        if (rc) return rc;
        HIPCHK(ctx, eslam_launch_hash_candidates(keys_out, order, cnt[me], ctx->gbase, G, ctx->hsend, ctx->stream));
        rc = comm_alltoallv(ctx, ctx->hsend, sb.data(), ctx->hrecv, rb.data());
        if (rc) return rc;
        uint32_t* ck = ctx->hsort.as<uint32_t>();
        uint32_t* cv = ck + total + 1;
        uint32_t* sk = cv + total + 1;
        uint32_t* so = sk + total + 1;
        HIPCHK(ctx, eslam_launch_hash_unpack(ctx->hrecv, total, ck, cv, ctx->stream));
        HIPCHK(ctx, eslam_radix_sort_pairs(ck, cv, sk, so, total, so + total + 1, &sbytes, ctx->stream));
        gorder = so;
    }
    std::vector<uint32_t> draws(k);
    for (uint64_t j = 0; j < k; ++j) draws[j] = (uint32_t)((uint64_t)(uint32_t)dm_libc_rand(ctx->libcp) % bsize);
    if (ctx->d_draws.cap() < sizeof(uint32_t) * k) HIPCHK(ctx, ctx->d_draws.alloc(sizeof(uint32_t) * k));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_draws, draws.data(), sizeof(uint32_t) * k, hipMemcpyHostToDevice, ctx->stream));
    if (ctx->sharded)
        HIPCHK(ctx, eslam_launch_hash_replace_global(ctx->st[0], ctx->st[1], ctx->ctl, gorder, ctx->d_draws, k, ctx->gbase,
                                                     ctx->n, ctx->d_hash_blist, ctx->hash_bstart[b], hash_field(ctx, 0),
                                                     hash_field(ctx, 1), hash_field(ctx, 2), hash_field(ctx, 3), weight,
                                                     ctx->stream));
    else
        HIPCHK(ctx, eslam_launch_hash_replace(ctx->st[0], ctx->st[1], ctx->ctl, order, ctx->d_draws, k, ctx->d_hash_blist,
                                              ctx->hash_bstart[b], hash_field(ctx, 0), hash_field(ctx, 1), hash_field(ctx, 2),
                                              hash_field(ctx, 3), weight, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // draws (host) must outlive the copy
    return ESLAM_OK;
}

// the device's zero-measurement-variance flag (k_finalize aborted the update): clear it and
// report the reference's exception text.  A timeout fault stays set (poisoned filter).
static int take_update_error(eslam_ctx* ctx)
{
    int rc = read_ctl(ctx);
    if (rc) return rc;
    const uint64_t err = ctx->ctl_host->err;
    if (err & (kFaultTimeout | kFaultPages)) {
        ctx->poisoned = true;
        ctx->poison_pages = (err & kFaultPages) != 0;
        return poison_fail(ctx);
    }
    if (!(err & 1ull)) return ESLAM_OK;
    ctx->ctl_host->err = 0;
    rc = write_ctl(ctx);
    if (rc) return rc;
    return fail(ctx, ESLAM_ERR_ZERO_MEAS_VAR, "using a zero measurement variance leads to singularities");
}

// the accepted domain of the sampler's Gaussian (eslam_step_input): checked on the host, in front
// of every launch, so no kernel sees a NaN pose delta or a NaN window margin
static bool step_input_ok(const eslam_step_input* in)
{
    for (int i = 0; i < 3; ++i)
        if (!dm_isfinite(in->sample_mean[i])) return false;
    for (int i = 0; i < 9; ++i)
        if (!dm_isfinite(in->sample_cov[i])) return false;
    return !(in->sample_cov[0] < 0.0 || in->sample_cov[4] < 0.0 || in->sample_cov[8] < 0.0);
}

// `track`: the call ends a step (eslam_gpu_step, eslam_gpu_update), so an enabled trajectory log
// takes its record once the step's kernels are enqueued
static int launch_step(eslam_ctx* ctx, const eslam_step_input* in, bool project, bool weight, bool track)
{
    track = track && ctx->traj.on;
    if (!step_input_ok(in))
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "step input: sample_mean and sample_cov must be finite, the variances not negative");
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (check_poisoned(ctx)) return ESLAM_ERR_HIP;
    if (weight && !ctx->has_map) return fail(ctx, ESLAM_ERR_NO_ENVIRONMENT, "No environment attached.");
    StepParams p;
    fill_step_params(ctx, in, p);
    p.proj_event = ctx->proj_event;
    // the hash respawn (static counter of src/PoseEstimator.cpp:239, per context) runs on
    // the first project and every period-th after it, between project and update
    bool respawn = false;
    if (project && ctx->cfg.hash_use && ctx->has_hash) {
        const uint64_t period = ctx->cfg.hash_period ? ctx->cfg.hash_period : 1;
        respawn = ((*ctx->hash_ev)++ % period) == 0;
    }
    // logDebug records: the update's contact points are recorded on the projected state
    const bool records = weight && record_contacts(ctx);
    // a deferred sharded exchange: the weighting launch is split around it (own-output chunks,
    // the exchange, the other chunks) unless the step takes another path first
    const bool split = ctx->xpend && !respawn && !records && !particle_maps(ctx);
    if (ctx->xpend && !split) {
        const int rc = settle(ctx);
        if (rc) return rc;
    }
    // per-particle maps: the resample gather is materialised (it carries the store names), so
    // no k_project_weight consumes one
    if (particle_maps(ctx)) {
        const int rc = materialize(ctx);
        if (rc) return rc;
    }
    // logDebug records: the project runs as its own launch first (bit-identical to the fused
    // kernel)
    if (respawn || (records && project)) {
        const GatherView gv0 = gather_view(ctx);
        HIPCHK(ctx, eslam_launch_project_weight(1, 0, (int)ctx->maxp, ctx->st[0], ctx->st[1], &ctx->map, &p, ctx->ctl,
                                                ctx->shards, &gv0, nullptr, ctx->stream, nullptr, nullptr));
        HIPCHK(ctx, eslam_launch_commit(ctx->ctl, ctx->stream));
        ctx->proj_event++;
        if (gv0.record) ctx->has_anc = true;
        if (respawn) {
            const int rc = sample_from_hash(ctx, in, p);
            if (rc) return rc;
        }
        project = false;                      // done; the update below is weight-only
        if (!weight) return track ? trajectory_record(ctx, false) : ESLAM_OK;
    }
    if (records) {
        const uint32_t maxc = p.m ? p.m : 1u;
        if (ctx->dbg_cap < ctx->n || ctx->dbg.maxc < maxc) {
            free_debug(ctx);
            HIPCHK(ctx, ctx->dbgb.meas.alloc(ctx->cap * 32, &ctx->dbg.meas));
            HIPCHK(ctx, ctx->dbgb.ncp.alloc(ctx->cap, &ctx->dbg.ncp));
            HIPCHK(ctx, ctx->dbgb.cp.alloc(ctx->cap * 48ull * maxc, &ctx->dbg.cp));
            HIPCHK(ctx, ctx->dbgb.resampled.alloc(4, &ctx->dbg.resampled));
            ctx->dbg.maxc = maxc;
            ctx->dbg_cap = ctx->cap;
        }
        HIPCHK(ctx, eslam_launch_contact_records(ctx->st[0], ctx->st[1], &ctx->map, &p, ctx->ctl, &ctx->dbg, store_of(ctx),
                                                 ctx->stream));
    }
    if (weight) {
        // K1's parked per-bucket sums (K1Args::bspill): one slot per chunk of this context
        const uint64_t csz = 64ull * p.J;
        const int rc = grow(ctx, ctx->bspill, k1_bspill_bytes((ctx->n + csz - 1) / csz));
        if (rc) return rc;
    }
    rec(ctx, 0);
    const GatherView gv = gather_view(ctx);
    ChunkSel sel;
    memset(&sel, 0, sizeof(sel));
    if (split) {
        sel.mode = 1;                         // the own-output chunks (the segments kernel's chunk_sel)
        sel.cdev = ctx->mg + mg::kChunks;
    }
    HIPCHK(ctx, eslam_launch_project_weight(project, weight, (int)ctx->maxp, ctx->st[0], ctx->st[1], &ctx->map, &p, ctx->ctl,
                                            ctx->shards, &gv, store_of(ctx), ctx->stream, split ? &sel : nullptr, ctx->bspill));
    if (split) {
        // the previous update's exchange (its host wait overlaps the launch above), then the
        // chunks that needed its records.  A failure here leaves a half-weighted step: the
        // filter is poisoned rather than continued.
        ctx->xpend = false;
        uint64_t own_lo = 0, own_hi = 0;
        bool queued = false;
        hipStream_t xs = ctx->comm.nranks > 1 ? ctx->xstream : ctx->stream;
        const int rc = exchange_tail(ctx, ctx->xpend_epoch, ctx->xpend_pp, &own_lo, &own_hi, xs, &queued);
        if (rc) {
            ctx->poisoned = true;
            if (xs != ctx->stream) (void)hipStreamSynchronize(xs);
            return rc;
        }
        if (queued && xs != ctx->stream) {
            // the main stream continues once the records and their marks are in place
            HIPCHK(ctx, hipEventRecord(ctx->ev_x, xs));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_x, 0));
        }
        const uint64_t csz = 64ull * p.J, nch = (ctx->n + csz - 1) / csz;
        if (own_lo > 0 || own_hi < nch) {
            sel.mode = 2;
            sel.c_lo = own_lo;
            sel.c_hi = own_hi;
            sel.cdev = nullptr;
            // the exchange may have grown (reallocated) the receive buffer: the records are read
            // through the gather view taken now, not the one of the first launch
            const GatherView gve = gather_view(ctx);
            HIPCHK(ctx, eslam_launch_project_weight(project, weight, (int)ctx->maxp, ctx->st[0], ctx->st[1], &ctx->map, &p,
                                                    ctx->ctl, ctx->shards, &gve, store_of(ctx), ctx->stream, &sel, ctx->bspill));
        }
    }
    rec(ctx, 1);
    if (project) ctx->proj_event++;
    if (gv.record) ctx->has_anc = true;
    if (weight) {
        const int rc = run_update_tail(ctx, FIN_UPDATE, true);   // finalize commits the flip
        if (rc) return rc;
        if (records) {
            // the records describe this update; its resample decision maps outputs to them
            HIPCHK(ctx, hipMemcpyAsync(ctx->dbg.resampled, &ctx->ctl->resample, 4, hipMemcpyDeviceToDevice, ctx->stream));
            ctx->dbg_valid = true;
        }
        // the trajectory log: the gather is materialised now (no later kernel fuses it) and the
        // record reads this update's resample decision on the device, all behind K3 on the stream
        if (track) {
            const int rc2 = trajectory_record(ctx, true);
            if (rc2) return rc2;
        }
        // measVar = zSigma^2 + measurementError^2 is zero only when measurementError^2 is: in
        // that configuration the update is checked at once, so the error surfaces from this
        // call like the reference's throw (src/ContactModel.cpp:122-123) and the caller's
        // update gate pose is not advanced (src/EmbodiedSlamFilter.cpp:361-362)
        if (p.me2 == 0.0) return take_update_error(ctx);
        return ESLAM_OK;
    }
    HIPCHK(ctx, eslam_launch_commit(ctx->ctl, ctx->stream));
    rec(ctx, 2); rec(ctx, 3); rec(ctx, 4);
    return track ? trajectory_record(ctx, false) : ESLAM_OK;
}

extern "C" int eslam_gpu_project(eslam_ctx* ctx, const eslam_step_input* in)
{
    if (!ctx || !in) return ESLAM_ERR_INVALID_ARG;
    return launch_step(ctx, in, true, false, false);
}

extern "C" int eslam_gpu_update(eslam_ctx* ctx, const eslam_step_input* in)
{
    if (!ctx || !in) return ESLAM_ERR_INVALID_ARG;
    return launch_step(ctx, in, false, true, true);
}

extern "C" int eslam_gpu_step(eslam_ctx* ctx, const eslam_step_input* in, int* updated)
{
    if (!ctx || !in) return ESLAM_ERR_INVALID_ARG;
    const bool gate = update_gate(ctx->cfg.measurement_threshold_distance, ctx->cfg.measurement_threshold_angle, ctx->ud_pose,
                                  in->body2odometry_rot, in->body2odometry_trans) ||
                      in->ltc_count > 0;
    const int rc = launch_step(ctx, in, true, gate, true);
    if (rc) return rc;
    if (gate) {
        double R[9];
        q_to_mat(in->body2odometry_rot, R);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) ctx->ud_pose[r * 4 + c] = R[r * 3 + c];
            ctx->ud_pose[r * 4 + 3] = in->body2odometry_trans[r];
        }
    }
    if (updated) *updated = gate ? 1 : 0;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_debug_set_spin_limit(eslam_ctx* ctx, uint32_t polls)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    ctx->spin_limit = polls;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_debug_set_scan_items(eslam_ctx* ctx, uint32_t items)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (items != 0 && items != 1 && items != 2 && items != 4 && items != (uint32_t)kScanItems) return ESLAM_ERR_INVALID_ARG;
    ctx->debug_scan_items = items;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_set_min_effective(eslam_ctx* ctx, uint64_t min_effective)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    ctx->cfg.min_effective = min_effective;  // fin_params reads it at every update
    return ESLAM_OK;
}

extern "C" int eslam_gpu_sync(eslam_ctx* ctx, eslam_update_info* info)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    int rc = read_ctl(ctx);
    if (rc) return rc;
    const Ctl& c = *ctx->ctl_host;
    if (info) {
        info->effective = c.eff;
        info->weight_sum = c.S;
        info->floating_weight = c.fw;
        info->max_weight = c.max_weight;
        info->data_particles = c.data_particles;
        info->total_points = c.total_points;
        info->resampled = (int32_t)c.resample;
        info->uniform_reset = (int32_t)c.uniform;
        info->resample_overruns = c.overruns;
        info->update_count = c.update_count;
        info->map_patches_dropped = c.map_dropped;
        info->map_stores_copied = c.map_copied;
        info->map_patches_covered = c.map_covered;
        info->map_stores_changed = c.map_changed;
        info->map_cells_written = c.map_written;
        info->map_pages_taken = c.map_taken;
        info->map_tiles_evicted = c.map_evicted;
        info->map_pages_free = c.pg_nfree > c.pg_cursor ? c.pg_nfree - c.pg_cursor : 0;
    }
    double acc[5];
    eslam_kernel_times& t = ctx->times;
    if (const uint32_t steps = ctx->timing ? ctx->ring.sums(acc) : 0) {
        const double inv = 1.0 / steps;
        t.project_weight_ms = (float)(acc[0] * inv);
        t.finalize_ms = (float)(acc[1] * inv);
        t.normalize_scan_ms = (float)(acc[2] * inv);
        t.resample_ms = (float)(acc[3] * inv);
        t.total_ms = (float)(acc[4] * inv);
    }
    if (const uint32_t steps = ctx->timing ? ctx->mring.sums(acc) : 0) {
        const double inv = 1.0 / steps;
        t.map_gather_ms = (float)(acc[0] * inv);
        t.map_cow_ms = (float)(acc[1] * inv);
        t.map_plan_ms = (float)(acc[2] * inv);
        t.map_merge_ms = (float)(acc[3] * inv);
        t.map_total_ms = (float)(acc[4] * inv);
    }
    if (const uint32_t steps = ctx->timing ? ctx->xring.sums(acc) : 0) t.map_match_ms = (float)(acc[0] / steps);
    return take_update_error(ctx);
}

// ---------------------------------------------------------------------------------------
// ParticleFilter<T> API
// ---------------------------------------------------------------------------------------
static int standalone(eslam_ctx* ctx, uint32_t mode)
{
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (check_poisoned(ctx)) return ESLAM_ERR_HIP;
    const int rc = materialize(ctx);
    if (rc) return rc;
    const uint32_t J = dm_chunk_rows_cfg(ctx->n_global, ctx->cfg.sum_chunk_rows);
    HIPCHK(ctx, eslam_launch_weight_stats(ctx->st[0], ctx->st[1], ctx->n, J, ctx->ctl, ctx->shards, ctx->stream));
    if (mode == FIN_SUM && !ctx->sharded) {
        const FinParams fp = fin_params(ctx, mode);
        HIPCHK(ctx, eslam_launch_finalize(ctx->shards, kNShard, ctx->ctl, &fp, ctx->stream));
        return ESLAM_OK;
    }
    return run_update_tail(ctx, mode, false);
}

extern "C" int eslam_gpu_get_weights_sum(eslam_ctx* ctx, double* sum)
{
    if (!ctx || !sum) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    int rc = standalone(ctx, FIN_SUM);
    if (rc) return rc;
    rc = read_ctl(ctx);
    if (rc) return rc;
    *sum = ctx->ctl_host->S;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_normalize_weights(eslam_ctx* ctx, double* effective)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    int rc = standalone(ctx, FIN_NORMALIZE);
    if (rc) return rc;
    rc = read_ctl(ctx);
    if (rc) return rc;
    if (effective) *effective = ctx->ctl_host->eff;
    return ESLAM_OK;
}

// the stand-alone resample at the current count, which always resamples.  With the trajectory log
// enabled its gather runs at once (it writes pt.anc) and the link is composed with the ancestors
static int resample_in_place(eslam_ctx* ctx)
{
    ctx->dbg_valid = false;                  // the records no longer follow the particles
    int rc = standalone(ctx, FIN_RESAMPLE);
    if (rc || !ctx->traj.on) return rc;
    rc = materialize(ctx);
    return rc ? rc : trajectory_compose(ctx);
}

extern "C" int eslam_gpu_resample(eslam_ctx* ctx)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    return resample_in_place(ctx);
}

// ParticleFilter<T>::resample_stratified(samples) / resample_multinomial(samples)
// (src/ParticleFilter.hpp:85-108, 120-148): resample the weights as they stand to `samples`
// particles (DESIGN.md 2 "Resample to a count").  A stratified call at the current count is
// eslam_gpu_resample.  Otherwise (eslam_resample.hip): the exact weight sum fixes the shift, the
// cumulative sum is written out, every draw searches its ancestor, and the gather runs at once
// into the other state buffer, or, beyond the capacity, into a new particle set allocated before
// anything changes.
int eslam_host::resample_to(eslam_ctx* ctx, uint64_t samples, bool multi, eslam_resample_info* info)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (samples == 0 || samples >= (1ull << 32) - 1)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "resample: samples must be in [1, 2^32 - 2]");
    // the shard boundaries are fixed by set_comm; refused before any collective (settle is one)
    if (ctx->sharded && (multi || samples != ctx->n_global))
        return fail(ctx, ESLAM_ERR_UNSUPPORTED, "resample: a sharded filter resamples to its own count only (stratified)");
    // (a sharded filter's log counts per rank, and a resample here keeps every shard's size)
    if (ctx->traj.on && !ctx->traj.sharded && samples > ctx->traj.max_particles)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "resample: samples may not exceed the trajectory log's max_particles");
    if (const int rc_ = settle(ctx)) return rc_;
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (check_poisoned(ctx)) return ESLAM_ERR_HIP;
    const uint64_t n = ctx->n;
    int rc;
    // the current count (a sharded filter's global one: its capacity is the shard's): the resample itself
    if (!multi && samples == ctx->n_global) {
        rc = resample_in_place(ctx);
        if (rc || !info) return rc;
        rc = read_ctl(ctx);
        if (rc) return rc;
        info->n_before = info->n_after = ctx->n_global;
        info->overruns = ctx->ctl_host->overruns;
        return ESLAM_OK;
    }
    if (particle_maps(ctx) && samples > ctx->cap)
        return fail(ctx, ESLAM_ERR_UNSUPPORTED,
                    "resample: per-particle maps are sized at init; samples may not exceed that capacity");
    rc = materialize(ctx);
    if (rc) return rc;
    // everything the call allocates, first: a failure returns with the filter as it was
    const uint64_t tn = eslam_resample_tiles(n), ts = eslam_resample_tiles(samples);
    ResampleScratch rs;
    Carver size(nullptr);
    carve_resample(size, n, tn, samples, ts, multi, &rs);
    hipError_t he = hipSuccess;
    rc = ctx->rs_mem.grow_keep(size.bytes(), 1, ctx->stream, &he);
    if (rc == ESLAM_ERR_HIP) return fail(ctx, rc, hipGetErrorString(he));
    if (rc) return fail(ctx, rc, "resample: no device memory for the cumulative sum and the draws");
    const bool growing = samples > ctx->cap;
    ParticleSet ps;
    if (growing) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (alloc_particle_set(ctx, samples, ps) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "resample: no device memory for the larger particle set");
        }
        HIPCHK(ctx, hipDeviceSynchronize());     // the new buffers' resets, before the stream uses them
    }
    Carver place(ctx->rs_mem.get());
    carve_resample(place, n, tn, samples, ts, multi, &rs);
    uint64_t *const C = rs.C, *const coarse = rs.coarse, *const counter = rs.counter;
    uint32_t *const anc = rs.anc, *const anc_kept = rs.anc_kept, *const kept = rs.kept;
    ctx->dbg_valid = false;                      // the records no longer follow the particles
    const uint32_t J = dm_chunk_rows_cfg(ctx->n_global, ctx->cfg.sum_chunk_rows);
    HIPCHK(ctx, eslam_launch_weight_stats(ctx->st[0], ctx->st[1], n, J, ctx->ctl, ctx->shards, ctx->stream));
    const FinParams fp = fin_params(ctx, FIN_SUM);
    HIPCHK(ctx, eslam_launch_finalize(ctx->shards, kNShard, ctx->ctl, &fp, ctx->stream));
    HIPCHK(ctx, eslam_launch_rs_cumsum(ctx->st[0], ctx->st[1], n, ctx->ctl, dm_minstd_pow(samples), coarse, C, counter,
                                       ctx->stream));
    HIPCHK(ctx, eslam_launch_rs_draw(multi ? 1 : 0, n, samples, ctx->ctl, ctx->jump, coarse, C, anc, kept, counter, ctx->stream));
    if (multi) {
        HIPCHK(ctx, eslam_launch_scan_excl(kept, ts + 1, ctx->stream));
        HIPCHK(ctx, eslam_launch_rs_compact(samples, anc, kept, anc_kept, ctx->stream));
    }
    rc = read_ctl(ctx);                          // waits for the draws
    if (rc) return rc;
    uint64_t beyond = 0;
    HIPCHK(ctx, hipMemcpy(&beyond, counter, 8, hipMemcpyDeviceToHost));
    const uint64_t n_after = multi ? samples - beyond : samples;
    Ctl* c = ctx->ctl_host;
    const uint32_t base = c->base ^ c->flip;
    const DevState out = growing ? ps.st[0] : ctx->st[base ^ 1u];
    const bool record = keep_ancestors(ctx) && n_after;
    uint32_t* anc_out = record ? (growing ? ps.pt.anc.get() : ctx->pt.anc.get()) : nullptr;
    HIPCHK(ctx, eslam_launch_rs_gather(ctx->st[0], ctx->st[1], ctx->ctl, out, n_after, anc_kept, multi ? 1 : 0, 1.0 / (double)n,
                                       anc_out, ctx->stream));
    // K3's tile words carry the tag of the launch that wrote them; a launch over another count
    // writes other words, so none may keep a tag from before the count changed
    if (!growing)
        HIPCHK(ctx, hipMemsetAsync(ctx->pt.tile_sum, 0, ((uint64_t)kPubReplicas * ctx->pub_stride + 16) * 8, ctx->stream));
    c->base = growing ? 0u : base ^ 1u;
    c->flip = 0;
    c->gather = 0;
    rc = write_ctl(ctx);                         // waits for the gather: the old set may go
    if (rc) return rc;
    if (growing) adopt_particle_set(ctx, ps, samples);
    ctx->n = ctx->n_global = n_after;
    ctx->has_anc = record;
    if (info) {
        info->n_before = n;
        info->n_after = n_after;
        if (multi) info->dropped = beyond;
        else info->overruns = beyond;
    }
    // the trajectory log: the gather above wrote the outputs' ancestors; the link follows them
    return ctx->traj.on ? trajectory_compose(ctx) : ESLAM_OK;
}

extern "C" int eslam_gpu_resample_stratified(eslam_ctx* ctx, uint64_t samples, eslam_resample_info* info)
{
    return resample_to(ctx, samples, false, info);
}

extern "C" int eslam_gpu_resample_multinomial(eslam_ctx* ctx, uint64_t samples, eslam_resample_info* info)
{
    return resample_to(ctx, samples, true, info);
}

// The same on a sharded filter, to any count (DESIGN.md 5 "Resample to a count, sharded";
// eslam_resample.hip k_rss_*).  Collective.  The exchanges: the statistics all_gather of the
// exact global sum; one all_gather of the ranks' 8-byte fixed-point totals; one of the records
// every rank sends to every rank (G words); one all_to_all_v of the records.  The two small
// all_gathers carry the ranks' status too (~0 for a rank that could not allocate), so a
// rank-local failure ends the call on every rank before anything has changed.  Nothing of the
// filter changes before the commit at the end: the minstd state included.
int eslam_host::resample_sharded(eslam_ctx* ctx, uint64_t samples, bool multi, eslam_resample_info* info)
{
    if (!ctx) {
        if (info) memset(info, 0, sizeof(*info));
        return ESLAM_ERR_INVALID_ARG;
    }
    if (!ctx->sharded) return resample_to(ctx, samples, multi, info);
    if (info) memset(info, 0, sizeof(*info));
    // every refusal the arguments, the flags and the table decide: before any collective (settle is one)
    if (samples == 0 || samples > (1ull << 30) - 64)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "resample_sharded: samples must be in [1, 2^30 - 64]");
    if (particle_maps(ctx))
        return fail(ctx, ESLAM_ERR_UNSUPPORTED, "resample_sharded: per-particle maps do not travel with a count-changing resample");
    const int G = ctx->comm.nranks, me = ctx->comm.rank;
    uint64_t nb[kMaxRanks + 1] = {};
    if (!multi && eslam_gpu_shard_bounds(samples, G, ctx->cfg.sum_chunk_rows, nb) != ESLAM_OK)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "resample_sharded: samples cannot be split into nranks chunk-aligned shards");
    // the trajectory log: the stratified call's new shards are known from the arguments
    if (!multi && !trajectory_holds(ctx, nb))
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "resample_sharded: a rank's new shard would exceed its trajectory log's max_particles");
    if (const int rc_ = settle(ctx)) return rc_;
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (check_poisoned(ctx)) return ESLAM_ERR_HIP;
    // the current count on the canonical table: the sharded resample itself
    if (!multi && samples == ctx->n_global && std::equal(nb, nb + G + 1, ctx->gall.begin()))
        return resample_to(ctx, samples, false, info);
    const uint64_t n = ctx->n, n_before = ctx->n_global;
    // the exact global sum (the statistics all_gather + FIN_SUM); runs a pending gather first
    int rc = standalone(ctx, FIN_SUM);
    if (rc) return rc;
    // this rank's C and total.  A rank without memory for them gathers ~0: every rank stops
    const uint64_t tn = eslam_resample_tiles(n), ts = eslam_resample_tiles(samples);
    ResampleShardScratch rs;
    Carver size(nullptr);
    carve_resample_sharded(size, n, tn, ts, multi, &rs);
    hipError_t he = hipSuccess;
    int mine = ctx->rs_mem.grow_keep(size.bytes(), 1, ctx->stream, &he);
    if (mine == ESLAM_ERR_HIP) return fail(ctx, mine, hipGetErrorString(he));
    uint64_t* h = ctx->mg_host;
    if (!mine) {
        Carver place(ctx->rs_mem.get());
        carve_resample_sharded(place, n, tn, ts, multi, &rs);
        HIPCHK(ctx, eslam_launch_rss_cumsum(ctx->st[0], ctx->st[1], n, ctx->ctl, rs.coarse, rs.C, rs.counter, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->mg + mg::kTotal, rs.coarse + (tn - 1), 8, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        h[mg::kTotal] = ~0ull;
        HIPCHK(ctx, hipMemcpyAsync(ctx->mg + mg::kTotal, &h[mg::kTotal], 8, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = comm_allgather(ctx, ctx->mg + mg::kTotal, ctx->mg + mg::kTotals, 8);
    if (rc) return rc;
    uint64_t tot[kMaxRanks];
    HIPCHK(ctx, hipMemcpyAsync(tot, ctx->mg + mg::kTotals, 8ull * G, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    auto peer_failed = [&](const uint64_t* words, uint64_t stride) -> int {
        for (int r = 0; r < G; ++r)
            if (words[(uint64_t)r * stride] == ~0ull) return r;
        return -1;
    };
    if (mine) return fail(ctx, mine, "resample_sharded: no device memory for the cumulative sum");
    if (const int r = peer_failed(tot, 1); r >= 0)
        return fail(ctx, ESLAM_ERR_COMM, ("resample_sharded: rank " + std::to_string(r) + " failed (no device memory)").c_str());
    RsPlan pl;
    memset(&pl, 0, sizeof(pl));
    for (int r = 0; r < G; ++r) {
        if (r < me) pl.off += tot[r];
        pl.gtotal += tot[r];
    }
    pl.total = tot[me];
    pl.n = n;
    pl.ntiles = tn;
    pl.samples = samples;
    pl.inv_samples = 1.0 / (double)samples;
    pl.gbase = ctx->gbase;
    pl.G = G;
    pl.me = me;
    pl.set_weight = multi ? 1u : 0u;
    pl.weight = 1.0 / (double)n_before;
    // multinomial: the dropped draws fix n_after and the table; every rank counts the same
    uint64_t beyond = 0, n_after = samples;
    if (multi) {
        HIPCHK(ctx, eslam_launch_rss_census(&pl, ctx->ctl, ctx->jump, rs.kept, rs.counter, ctx->stream));
        HIPCHK(ctx, eslam_launch_scan_excl(rs.kept, ts + 1, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(&beyond, rs.counter + kRsBeyond, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        n_after = samples - beyond;
        if (n_after == 0 || eslam_gpu_shard_bounds(n_after, G, ctx->cfg.sum_chunk_rows, nb) != ESLAM_OK)
            return fail(ctx, ESLAM_ERR_INVALID_ARG,
                        "resample_sharded: the kept draws cannot be split into nranks chunk-aligned shards (nothing changed)");
        // every rank counted the same draws: all of them stop here
        if (!trajectory_holds(ctx, nb))
            return fail(ctx, ESLAM_ERR_INVALID_ARG,
                        "resample_sharded: a rank's new shard would exceed its trajectory log's max_particles (nothing changed)");
    }
    for (int d = 0; d <= G; ++d) pl.nb[d] = nb[d];
    // the records this rank sends to every rank
    const DevState none = {};
    HIPCHK(ctx, eslam_launch_rss_route(multi ? 1 : 0, 0, &pl, ctx->st[0], ctx->st[1], none, ctx->ctl, ctx->jump, rs.coarse, rs.C,
                                       rs.kept, nullptr, nullptr, rs.counter, ctx->stream));
    uint64_t cnt[kMaxRanks] = {}, nrecv = 0;
    HIPCHK(ctx, hipMemcpyAsync(cnt, rs.counter + kRsCount, 8ull * G, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&nrecv, rs.counter + kRsRecv, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (!multi) HIPCHK(ctx, hipMemcpyAsync(&beyond, rs.counter + kRsBeyond, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t nsend = 0;
    for (int d = 0; d < G; ++d) {
        pl.send_off[d] = nsend;
        nsend += cnt[d];
    }
    pl.send_off[G] = nsend;
    // everything the call still allocates, before the counts are exchanged: the larger particle
    // set, the records' buffers (every rank evaluates every draw, so it has counted the records
    // it will receive itself), the new table's buffers
    const uint64_t n_new = nb[me + 1] - nb[me];
    const bool growing = n_new > ctx->cap;
    ParticleSet ps;
    const uint64_t R = eslam_record_bytes();
    if (growing && alloc_particle_set(ctx, n_new, ps) != hipSuccess) {
        (void)hipGetLastError();
        ps = ParticleSet{};
        mine = fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "resample_sharded: no device memory for the larger particle set");
    }
    if (growing && !mine) HIPCHK(ctx, hipDeviceSynchronize());     // the new buffers' resets, before the stream uses them
    if (!mine && (mine = ctx->sendbuf.grow_keep((nsend ? nsend : 1) * R, 1, ctx->stream, &he)) != ESLAM_OK)
        fail(ctx, mine, "resample_sharded: no device memory for the records to send");
    if (!mine && (mine = ctx->recvbuf.grow_keep((nrecv ? nrecv : 1) * R, 1, ctx->stream, &he)) != ESLAM_OK)
        fail(ctx, mine, "resample_sharded: no device memory for the records to receive");
    if (!mine) mine = reserve_shard_table(ctx, G, n_after, nb);
    const std::string msg = ctx->err;
    for (int d = 0; d < G; ++d) h[mg::kCounts + d] = mine ? ~0ull : cnt[d];
    HIPCHK(ctx, hipMemcpyAsync(ctx->mg + mg::kCounts, &h[mg::kCounts], 8ull * G, hipMemcpyHostToDevice, ctx->stream));
    rc = comm_allgather(ctx, ctx->mg + mg::kCounts, ctx->mg + mg::kCountsAll, 8ull * G);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(&h[mg::kCountsAll], ctx->mg + mg::kCountsAll, 8ull * G * G, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (mine) return fail(ctx, mine, msg.c_str());
    if (const int r = peer_failed(&h[mg::kCountsAll], (uint64_t)G); r >= 0)
        return fail(ctx, ESLAM_ERR_COMM, ("resample_sharded: rank " + std::to_string(r) + " failed (no device memory)").c_str());
    uint64_t sb[kMaxRanks], rb[kMaxRanks], told = 0;
    for (int r = 0; r < G; ++r) {
        const uint64_t c = h[mg::kCountsAll + r * G + me];
        sb[r] = cnt[r] * R;
        rb[r] = c * R;
        told += c;
    }
    if (told != nrecv) return fail(ctx, ESLAM_ERR_COMM, "resample_sharded: the ranks' record counts disagree");
    rc = read_ctl(ctx);
    if (rc) return rc;
    Ctl* c = ctx->ctl_host;
    const uint32_t base = c->base ^ c->flip;
    const DevState out = growing ? ps.st[0] : ctx->st[base ^ 1u];
    const bool record = keep_ancestors(ctx);
    uint32_t* anc_out = record ? (growing ? ps.pt.anc.get() : ctx->pt.anc.get()) : nullptr;
    ctx->dbg_valid = false;                      // the records no longer follow the particles
    HIPCHK(ctx, eslam_launch_rss_route(multi ? 1 : 0, 1, &pl, ctx->st[0], ctx->st[1], out, ctx->ctl, ctx->jump, rs.coarse, rs.C,
                                       rs.kept, ctx->sendbuf, anc_out, rs.counter, ctx->stream));
    rc = comm_alltoallv(ctx, ctx->sendbuf, sb, ctx->recvbuf, rb);
    if (rc) return rc;
    HIPCHK(ctx, eslam_launch_rss_expand(ctx->recvbuf, nrecv, out, n_new, anc_out, ctx->stream));
    // K3's tile words carry the tag of the launch that wrote them (resample_to)
    if (!growing)
        HIPCHK(ctx, hipMemsetAsync(ctx->pt.tile_sum, 0, ((uint64_t)kPubReplicas * ctx->pub_stride + 16) * 8, ctx->stream));
    c->base = growing ? 0u : base ^ 1u;
    c->flip = 0;
    c->gather = 0;
    c->minstd = dm_mulmod31(dm_minstd_pow(samples), c->minstd);    // moved on by exactly `samples` draws
    rc = write_ctl(ctx);                         // waits for the expand: the old set may go
    if (rc) return rc;
    if (growing) adopt_particle_set(ctx, ps, n_new);
    rc = apply_shard_table(ctx, G, me, n_after, nb);                // reserved above: cannot fail
    if (rc) return rc;
    ctx->n = n_new;
    ctx->has_anc = record;
    if (info) {
        info->n_before = n_before;
        info->n_after = n_after;
        if (multi) info->dropped = beyond;
        else info->overruns = beyond;
    }
    // the trajectory log: the route and the expand wrote the outputs' ancestors (old global
    // indices); the link follows them across the ranks, from the old table to the new one
    return ctx->traj.on ? trajectory_compose(ctx) : ESLAM_OK;
}

extern "C" int eslam_gpu_resample_stratified_sharded(eslam_ctx* ctx, uint64_t samples, eslam_resample_info* info)
{
    return resample_sharded(ctx, samples, false, info);
}

extern "C" int eslam_gpu_resample_multinomial_sharded(eslam_ctx* ctx, uint64_t samples, eslam_resample_info* info)
{
    return resample_sharded(ctx, samples, true, info);
}

extern "C" int eslam_gpu_get_rng_state(eslam_ctx* ctx, eslam_rng_state* st)
{
    if (!ctx || !st) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    int rc = read_ctl(ctx);
    if (rc) return rc;
    memset(st, 0, sizeof(*st));
    st->minstd_x = ctx->ctl_host->minstd;
    st->project_count = ctx->proj_event;
    st->init_count = ctx->init_event;
    st->hash_count = *ctx->hash_ev;
    st->max_weight = ctx->ctl_host->max_weight;
    memcpy(st->ud_pose, ctx->ud_pose, sizeof(ctx->ud_pose));
    memcpy(st->libc_rand, ctx->libcp->r, sizeof(st->libc_rand));
    st->libc_rand_pos = ctx->libcp->i;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_set_rng_state(eslam_ctx* ctx, const eslam_rng_state* st)
{
    if (!ctx || !st) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    int rc = read_ctl(ctx);
    if (rc) return rc;
    ctx->ctl_host->minstd = st->minstd_x;
    ctx->proj_event = st->project_count;
    ctx->init_event = st->init_count;
    *ctx->hash_ev = st->hash_count;
    ctx->ctl_host->max_weight = st->max_weight;
    memcpy(ctx->ud_pose, st->ud_pose, sizeof(ctx->ud_pose));
    memcpy(ctx->libcp->r, st->libc_rand, sizeof(st->libc_rand));
    ctx->libcp->i = st->libc_rand_pos % 34u;
    return write_ctl(ctx);
}

extern "C" int eslam_gpu_get_ancestors(eslam_ctx* ctx, uint32_t* out, uint64_t n)
{
    if (!ctx || !out) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (!ctx->has_anc || !ctx->pt.anc) return fail(ctx, ESLAM_ERR_INVALID_ARG, "no ancestors recorded (ESLAM_FLAG_RECORD_ANCESTORS)");
    if (const int rc = materialize(ctx)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, ctx->pt.anc, (n < ctx->n ? n : ctx->n) * 4, hipMemcpyDeviceToHost));
    return ESLAM_OK;
}

extern "C" int eslam_gpu_enable_timing(eslam_ctx* ctx, int enable)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timing = enable != 0;
    ctx->ring.clear();
    ctx->mring.clear();
    ctx->xring.clear();
    return ESLAM_OK;
}

extern "C" int eslam_gpu_get_kernel_times(eslam_ctx* ctx, eslam_kernel_times* t)
{
    if (!ctx || !t) return ESLAM_ERR_INVALID_ARG;
    *t = ctx->times;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_selftest_bm_radius(int device, uint64_t* mismatches)
{
    if (!mismatches) return ESLAM_ERR_INVALID_ARG;
    if (hipSetDevice(device) != hipSuccess) return ESLAM_ERR_HIP;
    Dev<unsigned long long> d;
    if (d.alloc(8) != hipSuccess) return ESLAM_ERR_OUT_OF_MEMORY;
    hipError_t e = hipMemset(d, 0, 8);
    if (e == hipSuccess) e = eslam_launch_selftest_bm_radius(d, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
    *mismatches = h;
    return e == hipSuccess ? ESLAM_OK : ESLAM_ERR_HIP;
}

extern "C" int eslam_gpu_selftest_sort(int device, const uint32_t* keys, const uint32_t* vals, uint64_t n, uint32_t* keys_out,
                                       uint32_t* vals_out)
{
    if ((!keys || !vals || !keys_out || !vals_out) && n) return ESLAM_ERR_INVALID_ARG;
    if (hipSetDevice(device) != hipSuccess) return ESLAM_ERR_HIP;
    size_t bytes = 0;
    (void)eslam_radix_sort_pairs(nullptr, nullptr, nullptr, nullptr, n, nullptr, &bytes, nullptr);
    const uint64_t b = (n ? n : 1) * 4;
    Dev<uint32_t> d;
    Dev<void> tmp;
    if (d.alloc(4 * b) != hipSuccess || tmp.alloc(bytes) != hipSuccess) return ESLAM_ERR_OUT_OF_MEMORY;
    hipError_t e = hipMemcpy(d, keys, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + b / 4, vals, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = eslam_radix_sort_pairs(d, d + b / 4, d + 2 * b / 4, d + 3 * b / 4, n, tmp, &bytes, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(keys_out, d + 2 * b / 4, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(vals_out, d + 3 * b / 4, n * 4, hipMemcpyDeviceToHost);
    return e == hipSuccess ? ESLAM_OK : ESLAM_ERR_HIP;
}

extern "C" int eslam_gpu_selftest_math(int device, int fn, const double* x, const double* y, double* out, uint64_t n)
{
    if (hipSetDevice(device) != hipSuccess) return ESLAM_ERR_HIP;
    Dev<double> dx, dy, dout;
    const uint64_t b = (n ? n : 1) * 8;
    if (dx.alloc(b) != hipSuccess || dy.alloc(b) != hipSuccess || dout.alloc(b) != hipSuccess)
        return ESLAM_ERR_OUT_OF_MEMORY;
    hipError_t e = n ? hipMemcpy(dx, x, n * 8, hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess) e = (y && n) ? hipMemcpy(dy, y, n * 8, hipMemcpyHostToDevice) : hipMemset(dy, 0, b);
    if (e == hipSuccess) e = eslam_launch_selftest_math(fn, dx, dy, dout, n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? ESLAM_OK : ESLAM_ERR_HIP;
}
