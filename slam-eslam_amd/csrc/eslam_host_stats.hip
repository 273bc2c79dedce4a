// eslam_host_stats.hip -- host side of libeslam_gpu: what is read off the particle set.  The best
// particle, the centroid, the pose distribution's Gaussian mixture, the pose moments, and the KLD
// count with the resample it sizes.  No kernels.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "eslam_ctx.h"
#include "eslam_scratch.h"

extern "C" int eslam_gpu_get_best_particle_index(eslam_ctx* ctx, uint64_t* index)
{
    if (!ctx || !index) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (!ctx->n) { *index = 0; return ESLAM_OK; }
    if (const int rc0 = materialize(ctx)) return rc0;
    uint64_t* out = ctx->scratch.as<uint64_t>();
    HIPCHK(ctx, eslam_launch_best_index(ctx->st[0], ctx->st[1], ctx->n, ctx->ctl, out, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->scratch_host, ctx->scratch, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t* h = ctx->scratch_host.as<const uint64_t>();
    if (!ctx->sharded) {
        *index = h[1] == ~0ull ? 0 : h[1];
        return ESLAM_OK;
    }
    // sharded: the first global maximum = the lowest rank holding the largest key
    uint64_t* m = ctx->mg_host;
    m[mg::kBest] = h[0];
    m[mg::kBest + 1] = h[1] == ~0ull ? ~0ull : ctx->gbase + h[1];
    HIPCHK(ctx, hipMemcpy(ctx->mg + mg::kBest, &m[mg::kBest], 16, hipMemcpyHostToDevice));
    const int rc = comm_allgather(ctx, ctx->mg + mg::kBest, ctx->mg + mg::kBestAll, 16);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(&m[mg::kBestAll], ctx->mg + mg::kBestAll, 16ull * ctx->comm.nranks, hipMemcpyDeviceToHost));
    uint64_t best = 0, idx = ~0ull;
    for (int r = 0; r < ctx->comm.nranks; ++r) {
        const uint64_t k = m[mg::kBestAll + 2 * r], i = m[mg::kBestAll + 2 * r + 1];
        if (i == ~0ull) continue;
        if (idx == ~0ull || k > best) { best = k; idx = i; }
    }
    *index = idx == ~0ull ? 0 : idx;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_get_centroid(eslam_ctx* ctx, double position[3], double orientation[4])
{
    if (!ctx || !position || !orientation) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    int rc = eslam_gpu_normalize_weights(ctx, nullptr);     // side effect, Q15
    if (rc) return rc;
    const uint32_t J = dm_chunk_rows_cfg(ctx->n_global, ctx->cfg.sum_chunk_rows);
    if (!ctx->sharded) {
        // the chunk records and the tree's second level, in the context's own buffer
        const uint64_t csz = 64ull * J, chunks = (ctx->n + csz - 1) / csz;
        rc = grow(ctx, ctx->cent, 2 * (chunks ? chunks : 1) * 5 * sizeof(double));
        if (rc) return rc;
        HIPCHK(ctx, eslam_launch_centroid(ctx->st[0], ctx->st[1], ctx->n, J, ctx->ctl, ctx->cent, ctx->scratch, ctx->stream));
    } else {
        // the shards are chunk-aligned: every rank's chunk records, all-gathered (padded to
        // the largest shard) and laid out in global chunk order, feed the same fixed tree
        // as on one GPU, so every rank computes the one-GPU centroid bit for bit
        rc = materialize(ctx);
        if (rc) return rc;
        const int G = ctx->comm.nranks;
        uint64_t nch[kMaxRanks], maxch, total;
        chunk_shape(ctx->gall.data(), G, J, nch, &maxch, &total);
        const uint64_t rec = 5 * sizeof(double);
        if (centroid_bytes(ctx->gall.data(), G, J) > ctx->cent.cap())
            return fail(ctx, ESLAM_ERR_HIP, "getCentroid: buffer not sized by set_comm");
        double* mine = ctx->cent;
        double* all = mine + maxch * 5;
        double* a = all + G * maxch * 5;
        double* b = a + (total ? total : 1) * 5;
        hipError_t e = hipMemsetAsync(mine, 0, maxch * rec, ctx->stream);
        if (e == hipSuccess) e = eslam_launch_centroid_chunks(ctx->st[0], ctx->st[1], ctx->n, J, ctx->ctl, mine, ctx->stream);
        if (e != hipSuccess) return fail(ctx, ESLAM_ERR_HIP, hipGetErrorString(e));
        rc = gather_chunks(ctx, nch, maxch, 5, mine, all, a);
        if (rc) return rc;
        e = eslam_launch_centroid_tree(a, b, total, ctx->scratch, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, ESLAM_ERR_HIP, hipGetErrorString(e));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->scratch_host, ctx->scratch, 5 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const double* h = ctx->scratch_host;       // sum x w, y w, theta w, z w, w
    const double sw = h[4];
    position[0] = h[0] / sw;
    position[1] = h[1] / sw;
    position[2] = h[3] / sw;
    const double mo = h[2] / sw;
    double a[4];
    q_from_yaw(mo, a);
    q_mul(a, ctx->zcomp, orientation);
    return ESLAM_OK;
}

extern "C" int eslam_gpu_get_z_compensated_orientation(eslam_ctx* ctx, double orientation[4])
{
    if (!ctx || !orientation) return ESLAM_ERR_INVALID_ARG;
    memcpy(orientation, ctx->zcomp, sizeof(ctx->zcomp));
    return ESLAM_OK;
}

// ---------------------------------------------------------------------------------------
// PoseDistribution::gmm: the 2-D Gaussian mixture over (x, y), fitted on the device
// ---------------------------------------------------------------------------------------
extern "C" void eslam_gmm_params_default(eslam_gmm_params* p)
{
    if (!p) return;
    p->components = 3;
    p->max_iterations = 10;
    p->tolerance = 1e-5;
    p->min_variance = 1e-6;
}

namespace {
// the fit's arrays within ctx->gmm: pass B's words (sharded: then every rank's), this rank's chunk
// records padded to the largest shard and all ranks' (sharded only), and the tree's two levels
// over the global chunks
struct GmmBufs {
    uint64_t* words;
    uint64_t* words_all;
    uint64_t* part;                      // pass B: every wave's words
    double* mine;
    double* all;
    double* a;
    double* b;
    uint64_t maxch = 1, total = 0;
    std::vector<uint64_t> nch;
};

uint64_t gmm_carve(const eslam_ctx* ctx, uint32_t R, uint32_t J, void* base, GmmBufs* g)
{
    const int G = ctx->sharded ? ctx->comm.nranks : 1;
    const uint64_t one[2] = {0, ctx->n};             // an unsharded filter's table
    g->nch.assign(G, 0);
    chunk_shape(ctx->sharded ? ctx->gall.data() : one, G, J, g->nch.data(), &g->maxch, &g->total);
    Carver c(base);
    g->words = c.take<uint64_t>(kGmmWords);
    g->words_all = c.take<uint64_t>((uint64_t)kGmmWords * G);
    g->part = c.take<uint64_t>((uint64_t)kGmmBoundsBlocks * kWaves * kGmmWords);
    g->mine = c.take<double>(ctx->sharded ? g->maxch * R : 0);
    g->all = c.take<double>(ctx->sharded ? (uint64_t)G * g->maxch * R : 0);
    g->a = c.take<double>((g->total ? g->total : 1) * R);
    g->b = c.take<double>((g->total ? g->total : 1) * R);
    return c.bytes();
}

// one pass of R sums per chunk: `launch(dst)` leaves the chunk records of this context at dst
// (sharded: those of every rank are then all-gathered into global chunk order), then the one-GPU
// tree; rec = the pass' R sums
template <typename Launch>
int chunk_pass(eslam_ctx* ctx, uint32_t R, const GmmBufs& g, double* rec, Launch launch)
{
    hipError_t e = hipSuccess;
    if (!ctx->sharded) {
        e = launch(g.a);
    } else {
        e = hipMemsetAsync(g.mine, 0, g.maxch * R * sizeof(double), ctx->stream);
        if (e == hipSuccess) e = launch(g.mine);
        if (e != hipSuccess) return fail(ctx, ESLAM_ERR_HIP, hipGetErrorString(e));
        const int rc = gather_chunks(ctx, g.nch.data(), g.maxch, R, g.mine, g.all, g.a);
        if (rc) return rc;
    }
    if (e == hipSuccess) e = eslam_launch_gmm_tree(g.a, g.b, g.total, R, ctx->scratch_host, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ESLAM_ERR_HIP, hipGetErrorString(e));
    memcpy(rec, ctx->scratch_host.get(), R * sizeof(double));
    return ESLAM_OK;
}

// a pass of the mixture's fit; rec = its DM_GMM_REC(K) sums
int gmm_pass(eslam_ctx* ctx, int K, bool hard, const GmmPass& P, uint32_t J, const GmmBufs& g, double* rec)
{
    return chunk_pass(ctx, DM_GMM_REC(K), g, rec, [&](double* dst) {
        return eslam_launch_gmm_pass(K, hard, ctx->st[0], ctx->st[1], ctx->n, J, ctx->ctl, &P, dst, ctx->stream);
    });
}
}  // namespace

extern "C" int eslam_gpu_fit_pose_gmm(eslam_ctx* ctx, const eslam_gmm_params* params, eslam_gmm_component* out,
                                      eslam_gmm_info* info)
{
    if (!ctx || !params || !out) return ESLAM_ERR_INVALID_ARG;
    if (params->components < 1 || params->components > ESLAM_GMM_MAX_COMPONENTS)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "fit_pose_gmm: components must be in [1, 8]");
    if (!(params->tolerance >= 0.0)) return fail(ctx, ESLAM_ERR_INVALID_ARG, "fit_pose_gmm: tolerance must not be negative or NaN");
    if (!dm_isfinite(params->min_variance) || !(params->min_variance > 0.0))
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "fit_pose_gmm: min_variance must be finite and positive");
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    const int K = (int)params->components;
    const uint32_t R = DM_GMM_REC(K);
    static_assert(DM_GMM_MAX == ESLAM_GMM_MAX_COMPONENTS, "component limit");
    static_assert((kMaxRanks + 1) * kGmmWords * 8 <= 4096 && DM_GMM_REC(DM_GMM_MAX) * 8 <= 4096, "scratch_host holds a readback");
    if (ctx->sharded) {
        // the ranks' parameters, compared before anything depends on them
        uint64_t mine[3];
        mine[0] = (uint64_t)params->components | (uint64_t)params->max_iterations << 32;
        mine[1] = dm_bits(params->tolerance);
        mine[2] = dm_bits(params->min_variance);
        static_assert(sizeof(mine) <= kHostXBytes, "host_allgather's words");
        const int rc = same_on_every_rank(ctx, mine, 3, "fit_pose_gmm: the ranks' parameters differ");
        if (rc) return rc;
    }
    int rc = materialize(ctx);                       // the particles as they stand
    const uint32_t J = dm_chunk_rows_cfg(ctx->n_global, ctx->cfg.sum_chunk_rows);
    GmmBufs g;
    if (!rc) rc = grow(ctx, ctx->gmm, gmm_carve(ctx, R, J, nullptr, &g));
    // sharded: a rank whose gather or allocation failed must not leave the others in the passes'
    // collectives (a failure inside a pass is a HIP or transport error no rank recovers from)
    rc = agree(ctx, rc, "fit_pose_gmm");
    if (rc) return rc;
    gmm_carve(ctx, R, J, ctx->gmm.get(), &g);

    // pass B: order-free words, reduced over the ranks identically everywhere
    const int G = ctx->sharded ? ctx->comm.nranks : 1;
    HIPCHK(ctx, eslam_launch_gmm_bounds(ctx->st[0], ctx->st[1], ctx->n, ctx->ctl, g.part, g.words, ctx->stream));
    if (ctx->sharded) {
        rc = comm_allgather(ctx, g.words, g.words_all, kGmmWords * sizeof(uint64_t));
        if (rc) return rc;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->scratch_host, ctx->sharded ? g.words_all : g.words, (uint64_t)G * kGmmWords * sizeof(uint64_t),
                               hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t B[kGmmWords] = {};
    for (int r = 0; r < G; ++r) {
        const uint64_t* w = ctx->scratch_host.as<const uint64_t>() + (uint64_t)r * kGmmWords;
        for (int q = kGmmMaxW; q <= kGmmMaxY; ++q) B[q] = B[q] > w[q] ? B[q] : w[q];
        B[kGmmUsed] += w[kGmmUsed];
        B[kGmmSkipped] += w[kGmmSkipped];
    }

    const double nan_ = dm_from_bits(0x7ff8000000000000ull);
    dm_gmm_comp comp[DM_GMM_MAX];
    memset(comp, 0, sizeof(comp));
    memset(out, 0, sizeof(eslam_gmm_component) * K);
    eslam_gmm_info inf;
    memset(&inf, 0, sizeof(inf));
    inf.particles_used = B[kGmmUsed];
    inf.particles_skipped = B[kGmmSkipped];
    if (!B[kGmmUsed]) {                              // no fitted particle: everything zero
        if (info) *info = inf;
        return ESLAM_OK;
    }
    GmmPass P;
    memset(&P, 0, sizeof(P));
    const double xmin = gmm_unkey(~B[kGmmMinX]), xmax = gmm_unkey(B[kGmmMaxX]);
    const double ymin = gmm_unkey(~B[kGmmMinY]), ymax = gmm_unkey(B[kGmmMaxY]);
    P.E = dm_stat_exp(gmm_unkey(B[kGmmMaxW]));
    P.cx = 0.5 * xmin + 0.5 * xmax;
    P.cy = 0.5 * ymin + 0.5 * ymax;
    P.axis = (xmax - xmin) >= (ymax - ymin) ? 0 : 1;
    P.amin = P.axis ? ymin : xmin;
    P.h = ((P.axis ? ymax : xmax) - P.amin) / (double)K;

    // pass 0: the hard assignment; then the fused E+M passes
    double rec[DM_GMM_REC(DM_GMM_MAX)];
    rc = gmm_pass(ctx, K, true, P, J, g, rec);
    if (rc) return rc;
    for (int k = 0; k < K; ++k) comp[k].live = 1;
    int nlive = dm_gmm_mstep(rec, K, params->min_variance, comp);
    double L = nan_, Lprev = nan_;
    for (uint32_t t = 1; t <= params->max_iterations && nlive > 0; ++t) {
        memcpy(P.c, comp, sizeof(comp));
        rc = gmm_pass(ctx, K, false, P, J, g, rec);
        if (rc) return rc;
        L = rec[6 * K + 1] / rec[6 * K];
        nlive = dm_gmm_mstep(rec, K, params->min_variance, comp);
        inf.iterations = t;
        if (t >= 2 && dm_fabs(L - Lprev) <= params->tolerance) { inf.converged = 1; break; }
        Lprev = L;
    }
    for (int k = 0; k < K; ++k) {
        if (!comp[k].set) continue;
        out[k].weight = comp[k].weight;
        out[k].mean[0] = comp[k].mx + P.cx;
        out[k].mean[1] = comp[k].my + P.cy;
        out[k].cov[0] = comp[k].cxx;
        out[k].cov[1] = comp[k].cxy;
        out[k].cov[2] = comp[k].cyy;
    }
    inf.components_live = (uint32_t)nlive;
    for (int k = 0; k < K; ++k) inf.live_mask |= comp[k].live ? 1u << k : 0u;
    inf.log_likelihood = L;
    inf.centre[0] = P.cx;
    inf.centre[1] = P.cy;
    inf.weight_exp = P.E;
    if (info) *info = inf;
    return ESLAM_OK;
}

// ---------------------------------------------------------------------------------------
// the pose estimate with its 4 x 4 covariance over (x, y, z, yaw), summed on the device
// ---------------------------------------------------------------------------------------
extern "C" int eslam_gpu_pose_moments(eslam_ctx* ctx, const eslam_pose_gate* gate, eslam_pose_moments* out)
{
    if (!ctx || !out) return ESLAM_ERR_INVALID_ARG;
    MomPass P;
    memset(&P, 0, sizeof(P));
    if (gate && !dm_mom_gate_set(&P.g, gate->centre, gate->cov, gate->chi2))
        return fail(ctx, ESLAM_ERR_INVALID_ARG,
                    "pose_moments: the gate needs a finite centre, xx > 0, a finite determinant > 0 and a finite chi2 >= 0");
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    static_assert((kMaxRanks + 1) * kMomWords * 8 <= 4096 && DM_MOM_REC2 * 8 <= 4096, "scratch_host holds a readback");
    static_assert(kMomWords <= kGmmWords && kMomBoundsBlocks <= kGmmBoundsBlocks, "gmm_carve's pass B arrays hold the moments'");
    if (ctx->sharded) {
        // the ranks' gates, compared before anything depends on them: the six doubles' bits, all
        // ones without a gate (no accepted gate has them: its values are finite)
        uint64_t mine[6];
        memset(mine, 0xff, sizeof(mine));
        if (gate) memcpy(mine, gate, sizeof(mine));
        static_assert(sizeof(eslam_pose_gate) == sizeof(mine) && sizeof(mine) <= kHostXBytes, "host_allgather's words");
        const int rc = same_on_every_rank(ctx, mine, 6, "pose_moments: the ranks' gates differ");
        if (rc) return rc;
    }
    const int rc = materialize(ctx);                 // the particles as they stand
    return pose_moments_of(ctx, ctx->st[0], ctx->st[1], P, rc, out);
}

int eslam_host::pose_moments_of(eslam_ctx* ctx, DevState s0, DevState s1, MomPass& P, int rc, eslam_pose_moments* out)
{
    const uint32_t J = dm_chunk_rows_cfg(ctx->n_global, ctx->cfg.sum_chunk_rows);
    GmmBufs g;                                       // the fit's layout at the wider record
    if (!rc) rc = grow(ctx, ctx->moments, gmm_carve(ctx, DM_MOM_REC2, J, nullptr, &g));
    rc = agree(ctx, rc, "pose_moments");             // no rank is left alone in the collectives below
    if (rc) return rc;
    gmm_carve(ctx, DM_MOM_REC2, J, ctx->moments.get(), &g);

    // pass B: order-free words, reduced over the ranks identically everywhere
    const int G = ctx->sharded ? ctx->comm.nranks : 1;
    HIPCHK(ctx, eslam_launch_moments_bounds(s0, s1, ctx->n, ctx->ctl, &P, g.part, g.words, ctx->stream));
    if (ctx->sharded) {
        rc = comm_allgather(ctx, g.words, g.words_all, kMomWords * sizeof(uint64_t));
        if (rc) return rc;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->scratch_host, ctx->sharded ? g.words_all : g.words, (uint64_t)G * kMomWords * sizeof(uint64_t),
                               hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t B[kMomWords] = {};
    for (int r = 0; r < G; ++r) {
        const uint64_t* w = ctx->scratch_host.as<const uint64_t>() + (uint64_t)r * kMomWords;
        B[kMomMaxW] = B[kMomMaxW] > w[kMomMaxW] ? B[kMomMaxW] : w[kMomMaxW];
        for (int q = kMomCounted; q <= kMomSkipped; ++q) B[q] += w[q];
    }
    eslam_pose_moments m;
    memset(&m, 0, sizeof(m));
    m.particles_counted = B[kMomCounted];
    m.particles_gated_out = B[kMomGatedOut];
    m.particles_skipped = B[kMomSkipped];
    if (B[kMomCounted] + B[kMomGatedOut]) m.weight_exp = P.E = dm_stat_exp(gmm_unkey(B[kMomMaxW]));
    if (!B[kMomCounted]) {                           // no counted particle: the counts, every double zero
        *out = m;
        return ESLAM_OK;
    }
    auto pass = [&](int which, uint32_t R, double* rec) {
        return chunk_pass(ctx, R, g, rec, [&](double* dst) {
            return eslam_launch_moments_pass(which, s0, s1, ctx->n, J, ctx->ctl, &P, dst, ctx->stream);
        });
    };
    double rec[DM_MOM_REC2], q[4];
    rc = pass(1, DM_MOM_REC1, rec);
    if (rc) return rc;
    dm_mom_mean(rec, P.mean, q);
    rc = pass(2, DM_MOM_REC2, rec);
    if (rc) return rc;
    memcpy(m.mean, P.mean, sizeof(m.mean));
    dm_mom_cov(rec, m.cov);
    m.yaw_resultant = q[0];
    m.effective = q[1];
    m.weight_share = q[2];
    m.z_within = q[3];
    *out = m;
    return ESLAM_OK;
}

// ---------------------------------------------------------------------------------------
// KLD-sampling: the occupied bins of the pose lattice, counted on the device, and the particle
// count they ask for
// ---------------------------------------------------------------------------------------
extern "C" void eslam_kld_params_default(const eslam_config* cfg, eslam_kld_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->bin_xy = 0.1;
    p->theta_bins = 36;
    p->epsilon = 0.05;
    p->z_quantile = 2.3263478740408408;
    p->n_min = cfg && cfg->particle_count ? cfg->particle_count : 1;
}

namespace {
// what is wrong with the parameters, or null
const char* kld_refusal(const eslam_kld_params* p)
{
    if (!dm_isfinite(p->bin_xy) || !(p->bin_xy > 0.0)) return "kld: bin_xy must be finite and positive";
    if (p->theta_bins < 1 || p->theta_bins > 4096) return "kld: theta_bins must be in [1, 4096]";
    if (p->multinomial > 1) return "kld: multinomial must be 0 or 1";
    if (!dm_isfinite(p->epsilon) || !(p->epsilon > 0.0)) return "kld: epsilon must be finite and positive";
    if (!dm_isfinite(p->z_quantile) || !(p->z_quantile >= 0.0)) return "kld: z_quantile must be finite and not negative";
    if (p->n_min == 0) return "kld: n_min must be at least 1";
    if (p->n_max != 0 && p->n_max < p->n_min) return "kld: n_max must be 0 or at least n_min";
    if (!(p->min_change >= 0.0)) return "kld: min_change must not be negative or NaN";
    return nullptr;
}

uint64_t kld_mix(uint64_t a, uint64_t b)
{
    uint64_t h = (a ^ (a >> 31)) * 0x9e3779b97f4a7c15ull;
    h = ((h ^ (h >> 29)) + b) * 0xbf58476d1ce4e5b9ull;
    return h ^ (h >> 32);
}

// min / max / sum of record b into a
void kld_fold(int64_t* a, const int64_t* b)
{
    a[kKldIx0] = a[kKldIx0] < b[kKldIx0] ? a[kKldIx0] : b[kKldIx0];
    a[kKldIx1] = a[kKldIx1] > b[kKldIx1] ? a[kKldIx1] : b[kKldIx1];
    a[kKldIy0] = a[kKldIy0] < b[kKldIy0] ? a[kKldIy0] : b[kKldIy0];
    a[kKldIy1] = a[kKldIy1] > b[kKldIy1] ? a[kKldIy1] : b[kKldIy1];
    a[kKldCounted] += b[kKldCounted];
    a[kKldSkipped] += b[kKldSkipped];
}

// ctx->kld of at least the layout's bytes (the new block exists before the old one goes)
int kld_reserve(eslam_ctx* ctx, uint64_t words, uint64_t gather)
{
    KldScratch ks;
    Carver size(nullptr);
    carve_kld(size, words, gather, &ks);
    hipError_t he = hipSuccess;
    const int rc = ctx->kld.grow_keep(size.bytes(), 1, ctx->stream, &he);
    if (rc == ESLAM_ERR_HIP) return fail(ctx, rc, hipGetErrorString(he));
    if (rc) return fail(ctx, rc, "kld_count: no device memory for the bitmap");
    return ESLAM_OK;
}

// the count itself; params checked, info zeroed
int kld_count(eslam_ctx* ctx, const eslam_kld_params* p, eslam_kld_info* info)
{
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    const int G = ctx->sharded ? ctx->comm.nranks : 1;
    static_assert(kKldWords * 8 <= kHostXBytes, "host_allgather's words");
    if (ctx->sharded) {
        // the ranks' parameters, compared before anything depends on them.  Six words: what shapes
        // the collectives that follow (the lattice, the bitmap's limit) and epsilon as they are,
        // the other four values as two 64-bit mixes
        uint64_t mine[kKldWords];
        mine[0] = dm_bits(p->bin_xy);
        mine[1] = (uint64_t)p->theta_bins | (uint64_t)p->multinomial << 32;
        mine[2] = p->max_bins;
        mine[3] = dm_bits(p->epsilon);
        mine[4] = kld_mix(dm_bits(p->z_quantile), p->n_min);
        mine[5] = kld_mix(p->n_max, dm_bits(p->min_change));
        const int rc = same_on_every_rank(ctx, mine, kKldWords, "kld_count: the ranks' parameters differ");
        if (rc) return rc;
    }
    const double inv = 1.0 / p->bin_xy;
    // pass 1 over the particles as they stand.  A rank whose gather or allocation failed says so
    // in the sign of its count, so no rank is left in a collective
    int rc = materialize(ctx);
    if (!rc) rc = kld_reserve(ctx, 0, 0);
    int64_t rec[kKldWords] = {2147483647ll, -2147483648ll, 2147483647ll, -2147483648ll, 0, 0};
    KldScratch ks;
    if (!rc) {
        Carver place(ctx->kld.get());
        carve_kld(place, 0, 0, &ks);
        HIPCHK(ctx, eslam_launch_kld_bounds(ctx->st[0], ctx->st[1], ctx->n, ctx->ctl, inv, p->theta_bins, ks.part, ks.out, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->scratch_host, ks.out, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(rec, ctx->scratch_host.get(), sizeof(rec));
    }
    if (ctx->sharded) {
        const std::string msg = ctx->err;
        int64_t all[kKldWords * kMaxRanks];
        if (rc) rec[kKldCounted] = -1;
        const int crc = host_allgather(ctx, rec, all, sizeof(rec));
        if (rc) return fail(ctx, rc, msg.c_str());
        if (crc) return crc;
        int64_t tot[kKldWords] = {2147483647ll, -2147483648ll, 2147483647ll, -2147483648ll, 0, 0};
        for (int r = 0; r < G; ++r) {
            if (all[kKldWords * r + kKldCounted] < 0)
                return fail(ctx, ESLAM_ERR_COMM, ("kld_count: rank " + std::to_string(r) + " failed").c_str());
            kld_fold(tot, &all[kKldWords * r]);
        }
        memcpy(rec, tot, sizeof(rec));
    } else if (rc) {
        return rc;
    }
    info->particles_counted = (uint64_t)rec[kKldCounted];
    info->particles_skipped = (uint64_t)rec[kKldSkipped];
    info->bins[2] = p->theta_bins;
    uint64_t k = 0;
    if (rec[kKldCounted]) {
        const uint64_t nx = (uint64_t)(rec[kKldIx1] - rec[kKldIx0] + 1), ny = (uint64_t)(rec[kKldIy1] - rec[kKldIy0] + 1);
        info->origin[0] = rec[kKldIx0];
        info->origin[1] = rec[kKldIy0];
        info->bins[0] = nx;
        info->bins[1] = ny;
        uint64_t cells = 0, total = 0;
        const bool wide = __builtin_mul_overflow(nx, ny, &cells) || __builtin_mul_overflow(cells, (uint64_t)p->theta_bins, &total);
        if (wide || total > (p->max_bins ? p->max_bins : 1ull << 27))
            return fail(ctx, ESLAM_ERR_UNSUPPORTED, "kld_count: cloud too spread for the bin size (the box's bins exceed max_bins)");
        const uint64_t words = (total + 63) / 64;
        rc = agree(ctx, kld_reserve(ctx, words, ctx->sharded ? (uint64_t)G : 0), "kld_count");
        if (rc) return rc;
        Carver place(ctx->kld.get());
        carve_kld(place, words, ctx->sharded ? (uint64_t)G : 0, &ks);
        KldGrid g;
        memset(&g, 0, sizeof(g));
        g.inv = inv;
        g.theta_bins = p->theta_bins;
        g.ix0 = rec[kKldIx0];
        g.iy0 = rec[kKldIy0];
        g.nx = nx;
        HIPCHK(ctx, eslam_launch_kld_mark(ctx->st[0], ctx->st[1], ctx->n, ctx->ctl, &g, ks.bits, words, ctx->stream));
        if (ctx->sharded) {
            rc = comm_allgather(ctx, ks.bits, ks.all, words * sizeof(uint64_t));
            if (rc) return rc;
            HIPCHK(ctx, eslam_launch_kld_or(ks.all, (uint32_t)G, words, ks.bits, ctx->stream));
        }
        HIPCHK(ctx, eslam_launch_kld_popcount(ks.bits, words, ks.part, ks.out, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->scratch_host, ks.out, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        k = (uint64_t)ctx->scratch_host.as<const int64_t>()[kKldCounted];
    }
    info->bins_occupied = k;
    info->bound = dm_kld_bound(k, p->epsilon, p->z_quantile);
    // the largest count the resample that follows accepts (resample_to, resample_sharded)
    uint64_t limit = ctx->sharded ? (1ull << 30) - 64 : (1ull << 32) - 2;
    if (p->n_max && p->n_max < limit) limit = p->n_max;
    const uint64_t capacity = !particle_maps(ctx) ? 0 : ctx->sharded ? ctx->n_global : ctx->cap;
    info->samples = dm_kld_samples(info->bound, p->n_min, limit, capacity, ctx->n_global, p->min_change, &info->clamped);
    return ESLAM_OK;
}
}  // namespace

extern "C" int eslam_gpu_kld_count(eslam_ctx* ctx, const eslam_kld_params* params, eslam_kld_info* info)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!ctx || !params || !info) return ESLAM_ERR_INVALID_ARG;
    if (const char* why = kld_refusal(params)) return fail(ctx, ESLAM_ERR_INVALID_ARG, why);
    return kld_count(ctx, params, info);
}

extern "C" int eslam_gpu_resample_kld(eslam_ctx* ctx, const eslam_kld_params* params, eslam_kld_info* info, eslam_resample_info* rinfo)
{
    if (info) memset(info, 0, sizeof(*info));
    if (rinfo) memset(rinfo, 0, sizeof(*rinfo));
    if (!ctx || !params) return ESLAM_ERR_INVALID_ARG;
    if (const char* why = kld_refusal(params)) return fail(ctx, ESLAM_ERR_INVALID_ARG, why);
    // the maps of a sharded filter do not travel, and whether the count changes is known only
    // after the count's collectives: refused before any, unless the parameters fix the count
    const bool pinned = ctx->sharded && particle_maps(ctx);
    if (pinned && !(params->n_min == ctx->n_global && params->n_max == ctx->n_global))
        return fail(ctx, ESLAM_ERR_UNSUPPORTED,
                    "resample_kld: a sharded filter with per-particle maps keeps its count (n_min == n_max == the global count)");
    eslam_kld_info inf;
    memset(&inf, 0, sizeof(inf));
    const int rc = kld_count(ctx, params, &inf);
    if (info) *info = inf;
    if (rc) return rc;
    const bool multi = params->multinomial != 0;
    return ctx->sharded && !pinned ? resample_sharded(ctx, inf.samples, multi, rinfo) : resample_to(ctx, inf.samples, multi, rinfo);
}
