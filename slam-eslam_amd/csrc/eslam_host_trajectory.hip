// eslam_host_trajectory.hip -- host side of libeslam_gpu: the trajectory log.  Its
// lifecycle, the record at the end of a step, the link's composition after a resample outside the
// step, and the two queries: a particle's lineage and the smoothed trajectory.  No kernels.
#include <hip/hip_runtime.h>

#include <string.h>

#include <vector>

#include "eslam_ctx.h"
#include "eslam_scratch.h"

namespace {
const char* kOffMsg = "trajectory: the log is not enabled (eslam_gpu_trajectory_enable)";

// the log's scratch of at least `bytes` (the new block exists before the old one goes)
int traj_scratch(eslam_ctx* ctx, uint64_t bytes)
{
    hipError_t he = hipSuccess;
    const int rc = ctx->traj.scratch.grow_keep(bytes, 1, ctx->stream, &he);
    if (rc == ESLAM_ERR_HIP) return fail(ctx, rc, hipGetErrorString(he));
    if (rc) return fail(ctx, rc, "trajectory: no device memory for the query's scratch");
    return ESLAM_OK;
}

// the j-th newest held entry as the kernels walk it
TrajLevel traj_level(const TrajectoryLog& t, uint32_t j)
{
    TrajLevel L;
    memset(&L, 0, sizeof(L));
    L.e = t.entry[t.at(j)];
    L.count = t.count[t.at(j)];
    return L;
}
}  // namespace

int eslam_host::trajectory_reset(eslam_ctx* ctx)
{
    TrajectoryLog& t = ctx->traj;
    t.head = t.held = 0;
    t.cur = 0;
    t.link_n = ctx->n;
    HIPCHK(ctx, eslam_launch_traj_iota(t.link[0], t.link_n, ctx->stream));
    return ESLAM_OK;
}

int eslam_host::trajectory_record(eslam_ctx* ctx, bool updated)
{
    TrajectoryLog& t = ctx->traj;
    if (ctx->n > t.max_particles) return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory: more particles than the log's max_particles");
    const int rc = materialize(ctx);                 // the device decides; writes pt.anc
    if (rc) return rc;
    const uint32_t e = t.head;
    HIPCHK(ctx, eslam_launch_traj_record(ctx->st[0], ctx->st[1], ctx->ctl, ctx->n, updated ? 1 : 0, ctx->pt.anc, t.link[t.cur],
                                         t.link_n, t.link[t.cur ^ 1u], &t.entry[e], ctx->stream));
    t.cur ^= 1u;
    t.link_n = ctx->n;
    t.count[e] = (uint32_t)ctx->n;
    t.step[e] = t.next_step++;
    t.head = (e + 1u) % t.capacity;
    if (t.held < t.capacity) t.held++;
    return ESLAM_OK;
}

int eslam_host::trajectory_compose(eslam_ctx* ctx)
{
    TrajectoryLog& t = ctx->traj;
    if (ctx->n > t.max_particles) return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory: more particles than the log's max_particles");
    HIPCHK(ctx, eslam_launch_traj_compose(ctx->pt.anc, t.link[t.cur], t.link_n, t.link[t.cur ^ 1u], ctx->n, ctx->stream));
    t.cur ^= 1u;
    t.link_n = ctx->n;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_trajectory_enable(eslam_ctx* ctx, uint32_t capacity_steps, uint64_t max_particles)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (ctx->sharded)
        return fail(ctx, ESLAM_ERR_UNSUPPORTED, "trajectory_enable: a sharded filter keeps no trajectory log (it needs a per-entry exchange)");
    if (capacity_steps == 0) return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory_enable: capacity_steps must be at least 1");
    const uint64_t slots = max_particles ? max_particles : (ctx->n ? ctx->cap : 0);
    if (slots == 0) return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory_enable: max_particles 0 needs an initialised filter");
    if (slots >= (1ull << 32) - 1 || slots < ctx->n)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory_enable: max_particles must hold the current particles and be below 2^32 - 1");
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    // a gather pending from before the log runs now: the link starts as the identity over the
    // particles as they stand
    if (const int rc_ = materialize(ctx)) return rc_;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // everything the call allocates, first: a failure leaves the context as it was
    TrajectoryLog t;
    uint32_t* link[2];
    Carver size(nullptr);
    carve_traj_log(size, capacity_steps, slots, nullptr, link);
    Dev<uint32_t> anc;
    if (t.mem.alloc(size.bytes()) != hipSuccess || (ctx->n && !ctx->pt.anc && anc.alloc(ctx->cap * 4) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "trajectory_enable: no device memory for the log");
    }
    t.bytes = size.bytes();
    t.entry.resize(capacity_steps);
    t.count.assign(capacity_steps, 0);
    t.step.assign(capacity_steps, 0);
    Carver place(t.mem.get());
    carve_traj_log(place, capacity_steps, slots, t.entry.data(), t.link);
    t.on = true;
    t.capacity = capacity_steps;
    t.max_particles = slots;
    if (anc) ctx->pt.anc = std::move(anc);           // kept from now on, as with ESLAM_FLAG_RECORD_ANCESTORS
    ctx->traj = std::move(t);
    return trajectory_reset(ctx);
}

extern "C" int eslam_gpu_trajectory_disable(eslam_ctx* ctx)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (!ctx->traj.on) return ESLAM_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the records in flight write the ring
    ctx->traj = TrajectoryLog{};
    return ESLAM_OK;
}

extern "C" int eslam_gpu_trajectory_clear(eslam_ctx* ctx)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (!ctx->traj.on) return fail(ctx, ESLAM_ERR_INVALID_ARG, kOffMsg);
    // the link names slots of the entries dropped: a pending gather runs first, then the
    // particles as they stand are the lineages' new start
    if (const int rc_ = materialize(ctx)) return rc_;
    return trajectory_reset(ctx);
}

extern "C" int eslam_gpu_trajectory_info(eslam_ctx* ctx, eslam_trajectory_info* info)
{
    if (!ctx || !info) return ESLAM_ERR_INVALID_ARG;
    memset(info, 0, sizeof(*info));
    const TrajectoryLog& t = ctx->traj;
    if (!t.on) return ESLAM_OK;
    info->enabled = 1;
    info->capacity_steps = t.capacity;
    info->max_particles = t.max_particles;
    info->entries = t.held;
    info->bytes = t.bytes;
    if (t.held) {
        info->first_step = t.step[t.at(t.held - 1u)];
        info->last_step = t.step[t.at(0)];
        info->particles = t.count[t.at(0)];
    }
    return ESLAM_OK;
}

extern "C" int eslam_gpu_get_trajectories(eslam_ctx* ctx, const uint64_t* indices, uint64_t count, eslam_trajectory_pose* out,
                                          uint64_t capacity, uint64_t* steps)
{
    if (steps) *steps = 0;
    if (!ctx || !steps || (count && !indices)) return ESLAM_ERR_INVALID_ARG;
    const TrajectoryLog& t = ctx->traj;
    if (!t.on) return fail(ctx, ESLAM_ERR_INVALID_ARG, kOffMsg);
    if (const int rc_ = settle(ctx)) return rc_;
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    std::vector<uint32_t> leaf(count);
    for (uint64_t k = 0; k < count; ++k) {
        if (indices[k] >= ctx->n) return fail(ctx, ESLAM_ERR_INVALID_ARG, "get_trajectories: an index is not below the particle count");
        leaf[k] = (uint32_t)indices[k];
    }
    const uint32_t m = (uint32_t)(t.held < capacity ? t.held : capacity);
    if (!m || !count) return ESLAM_OK;
    if (!out) return ESLAM_ERR_INVALID_ARG;
    int rc = materialize(ctx);                       // like the other queries; the log's link already stands
    if (rc) return rc;
    TrajTraceScratch s;
    Carver size(nullptr);
    carve_traj_trace(size, count, m, &s);
    rc = traj_scratch(ctx, size.bytes());
    if (rc) return rc;
    Carver place(ctx->traj.scratch.get());
    carve_traj_trace(place, count, m, &s);
    std::vector<TrajLevel> lv(m);
    for (uint32_t j = 0; j < m; ++j) lv[j] = traj_level(t, j);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(s.lv, lv.data(), m * sizeof(TrajLevel), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(s.leaf, leaf.data(), count * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, eslam_launch_traj_trace(s.leaf, count, t.link[t.cur], t.link_n, s.lv, m, s.nodes, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<TrajNode> nodes(count * m);
    HIPCHK(ctx, hipMemcpy(nodes.data(), s.nodes, nodes.size() * sizeof(TrajNode), hipMemcpyDeviceToHost));
    for (uint64_t k = 0; k < count; ++k) {
        for (uint32_t j = 0; j < m; ++j) {           // oldest first
            const TrajNode& nd = nodes[k * m + j];
            const uint32_t ring = t.at(m - 1u - j);
            eslam_trajectory_pose& o = out[k * capacity + j];
            o.step = t.step[ring];
            o.slot = nd.slot;
            o.particles = t.count[ring];
            o.x = nd.x;
            o.y = nd.y;
            o.z = nd.z;
            o.yaw = nd.yaw;
            o.zsigma = nd.zs;
        }
    }
    *steps = m;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_trajectory_smoothed(eslam_ctx* ctx, eslam_trajectory_estimate* out, uint64_t capacity, uint64_t* entries)
{
    if (entries) *entries = 0;
    if (!ctx || !entries) return ESLAM_ERR_INVALID_ARG;
    const TrajectoryLog& t = ctx->traj;
    if (!t.on) return fail(ctx, ESLAM_ERR_INVALID_ARG, kOffMsg);
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    if (const int rc_ = settle(ctx)) return rc_;
    const uint32_t m = (uint32_t)(t.held < capacity ? t.held : capacity);
    if (!m) return ESLAM_OK;
    if (!out) return ESLAM_ERR_INVALID_ARG;
    int rc = materialize(ctx);                       // the particles and weights as they stand
    if (!rc) rc = read_ctl(ctx);
    if (rc) return rc;
    const uint64_t n = ctx->n;
    TrajSmoothScratch s;
    Carver size(nullptr);
    carve_traj_smooth(size, n, t.max_particles, &s);
    rc = traj_scratch(ctx, size.bytes());
    if (rc) return rc;
    Carver place(ctx->traj.scratch.get());
    carve_traj_smooth(place, n, t.max_particles, &s);
    // the scratch state: the level's ancestors' columns under the current weights, as both buffers
    DevState S;
    memset(&S, 0, sizeof(S));
    S.x = s.x; S.y = s.y; S.th = s.th; S.z = s.z; S.zs = s.zs; S.w = s.w;
    const DevState& cur = ctx->st[ctx->ctl_host->base ^ ctx->ctl_host->flip];
    HIPCHK(ctx, hipMemcpyAsync(s.w, cur.w, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s.a, t.link[t.cur], n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    for (uint32_t j = 0; j < m; ++j) {               // newest first; s.a moves one entry back per level
        const TrajLevel L = traj_level(t, j);
        eslam_trajectory_estimate& o = out[m - 1u - j];
        memset(&o, 0, sizeof(o));
        o.step = t.step[t.at(j)];
        HIPCHK(ctx, eslam_launch_traj_level(n, &L, s.a, S, s.k.bits, ctx->stream));
        HIPCHK(ctx, eslam_launch_kld_popcount(s.k.bits, ((uint64_t)L.count + 63) / 64, s.k.part, s.k.out, ctx->stream));
        MomPass P;
        memset(&P, 0, sizeof(P));
        rc = pose_moments_of(ctx, S, S, P, ESLAM_OK, &o.moments);
        if (rc) return rc;
        int64_t rec[kKldWords];
        HIPCHK(ctx, hipMemcpy(rec, s.k.out, sizeof(rec), hipMemcpyDeviceToHost));   // the passes have synchronised
        o.distinct_ancestors = (uint64_t)rec[kKldCounted];
    }
    *entries = m;
    return ESLAM_OK;
}
