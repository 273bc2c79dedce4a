// eslam_host_trajectory.hip -- host side of libeslam_gpu: the trajectory log.  Its
// lifecycle, the record at the end of a step, the link's composition after a resample outside the
// step, and the two queries: a particle's lineage and the smoothed trajectory.  No kernels.
#include <hip/hip_runtime.h>

#include <string.h>

#include <string>
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

// ---------------------------------------------------------------------------------------
// the log of a sharded filter (DESIGN.md 5j "Sharded")
// ---------------------------------------------------------------------------------------
TrajTable traj_table(const eslam_ctx* ctx, const std::vector<uint64_t>& bounds)
{
    TrajTable T;
    memset(&T, 0, sizeof(T));
    T.G = (uint32_t)ctx->comm.nranks;
    T.me = (uint32_t)ctx->comm.rank;
    for (uint32_t r = 0; r <= T.G; ++r) T.b[r] = (uint32_t)bounds[r];
    return T;
}

// Items of an entry by global slot, the one exchange of the sharded log: out[p] becomes the item
// (node: a TrajItem, else a word) of slots[p] for the `count` positions in device memory, under
// the shard table `bounds` the entry (or the word array) was recorded under; src names this
// rank's part of it.  A slot outside the entry gives kTrajNone / a NaN item.  The slots this rank
// owns are served in place.  The others: bucketed by owner on the device, the request counts
// all_gathered, one all_to_all_v of the 4-byte requests, the owners' serve kernel, one
// all_to_all_v of the items, a scatter to the positions kept.  Where no rank asks another for
// anything the call ends after the all_gather.  Collective.  rc: what preparing the call returned
// on this rank; that, or the failure of this call's own allocation, travels in the counts (~0),
// so every rank returns instead of waiting: the failing rank its code, the others ESLAM_ERR_COMM.
int traj_fetch(eslam_ctx* ctx, int rc, bool node, const uint32_t* slots, uint64_t count, const std::vector<uint64_t>& bounds,
               TrajSrc src, void* out)
{
    TrajectoryLog& t = ctx->traj;
    const int G = ctx->comm.nranks, me = ctx->comm.rank;
    const TrajTable T = traj_table(ctx, bounds);
    src.first = T.b[me];
    const uint64_t item = node ? sizeof(TrajItem) : 4;
    if (G == 1) {                                    // every slot is this rank's: no exchange
        if (rc) return rc;
        HIPCHK(ctx, eslam_launch_traj_serve(node, slots, count, 1, &T, &src, out, ctx->stream));
        return ESLAM_OK;
    }
    uint32_t nblocks = 0;
    uint64_t per = 0;
    eslam_traj_bucket_shape(count, &nblocks, &per);
    TrajFetchOut xo;
    uint32_t tot[kTrajTotWords] = {};
    hipError_t he = hipSuccess;
    if (!rc) {
        Carver size(nullptr);
        carve_traj_fetch_out(size, count, nblocks, &xo);
        rc = t.xa.grow_keep(size.bytes(), 1, ctx->stream, &he);
        if (rc == ESLAM_ERR_HIP) return fail(ctx, rc, hipGetErrorString(he));
        if (rc) fail(ctx, rc, "trajectory: no device memory for the exchange's requests");
    }
    if (!rc) {
        Carver place(t.xa.get());
        carve_traj_fetch_out(place, count, nblocks, &xo);
        HIPCHK(ctx, eslam_launch_traj_serve(node, slots, count, 1, &T, &src, out, ctx->stream));
        HIPCHK(ctx, eslam_launch_traj_bucket(slots, count, &T, xo.cnt, xo.tot, xo.req, xo.pos, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(tot, xo.tot, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    // the request counts: row r of the gathered matrix is what rank r asks of each rank
    const std::string msg = ctx->err;
    uint64_t* h = ctx->mg_host;
    for (int d = 0; d < G; ++d) h[mg::kCounts + d] = rc ? ~0ull : (uint64_t)tot[d];
    HIPCHK(ctx, hipMemcpyAsync(ctx->mg + mg::kCounts, &h[mg::kCounts], 8ull * G, hipMemcpyHostToDevice, ctx->stream));
    const int crc = comm_allgather(ctx, ctx->mg + mg::kCounts, ctx->mg + mg::kCountsAll, 8ull * G);
    if (crc) return rc ? rc : crc;
    HIPCHK(ctx, hipMemcpyAsync(&h[mg::kCountsAll], ctx->mg + mg::kCountsAll, 8ull * G * G, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    bool peer_failed = false, any = false;
    uint64_t nin[kMaxRanks], tin = 0, tout = 0;
    for (int r = 0; r < G; ++r) {
        for (int d = 0; d < G; ++d) {
            const uint64_t v = h[mg::kCountsAll + r * G + d];
            peer_failed |= v == ~0ull;
            any |= v != 0;
        }
        nin[r] = h[mg::kCountsAll + r * G + me];
    }
    if (rc) return fail(ctx, rc, msg.c_str());
    if (peer_failed) return fail(ctx, ESLAM_ERR_COMM, "trajectory: the exchange failed on another rank");
    if (!any) return ESLAM_OK;
    for (int r = 0; r < G; ++r) {
        tin += nin[r];
        tout += tot[r];
    }
    // the memory for what comes in is sized only now: the ranks agree on it before they exchange
    TrajFetchIn xi;
    Carver size(nullptr);
    carve_traj_fetch_in(size, tin, tout, item, &xi);
    rc = t.xb.grow_keep(size.bytes(), 1, ctx->stream, &he);
    if (rc == ESLAM_ERR_HIP) fail(ctx, rc, hipGetErrorString(he));
    else if (rc) fail(ctx, rc, "trajectory: no device memory for the exchange's items");
    rc = agree(ctx, rc, "trajectory");
    if (rc) return rc;
    Carver place(t.xb.get());
    carve_traj_fetch_in(place, tin, tout, item, &xi);
    uint64_t sb[kMaxRanks], rb[kMaxRanks];
    for (int r = 0; r < G; ++r) {
        sb[r] = 4ull * tot[r];
        rb[r] = 4ull * nin[r];
    }
    rc = comm_alltoallv(ctx, xo.req, sb, xi.reqin, rb);
    if (rc) return rc;
    HIPCHK(ctx, eslam_launch_traj_serve(node, xi.reqin, tin, 0, &T, &src, xi.served, ctx->stream));
    for (int r = 0; r < G; ++r) {
        sb[r] = item * nin[r];
        rb[r] = item * tot[r];
    }
    rc = comm_alltoallv(ctx, xi.served, sb, xi.answers, rb);
    if (rc) return rc;
    HIPCHK(ctx, eslam_launch_traj_scatter(node, xi.answers, xo.pos, tout, out, ctx->stream));
    return ESLAM_OK;
}

// this rank's part of link[cur] as the exchange serves it (under t.link_table)
TrajSrc link_src(const TrajectoryLog& t)
{
    TrajSrc s;
    memset(&s, 0, sizeof(s));
    s.word = t.link[t.cur];
    s.count = (uint32_t)t.link_n;
    return s;
}

// ... and of ring entry `ring` (under t.table[ring]); bits: the smoothed sweep's bitmap or null
TrajSrc entry_src(const TrajectoryLog& t, uint32_t ring, uint64_t* bits)
{
    TrajSrc s;
    memset(&s, 0, sizeof(s));
    s.e = t.entry[ring];
    s.count = t.count[ring];
    s.bits = bits;
    return s;
}

void link_moved(eslam_ctx* ctx, bool identity)
{
    TrajectoryLog& t = ctx->traj;
    t.cur ^= 1u;
    t.link_n = ctx->n;
    t.link_table = ctx->gall;
    t.link_identity = identity;
}

// the record of a sharded filter.  While the link is the identity the parents are the sources
// themselves and nothing is exchanged; after a composition link[source] comes through traj_fetch
int record_sharded(eslam_ctx* ctx, bool updated)
{
    TrajectoryLog& t = ctx->traj;
    int rc = settle(ctx);                            // the update's deferred exchange, then its gather
    if (!rc) rc = materialize(ctx);
    if (rc) return rc;
    const uint32_t first = (uint32_t)ctx->gbase;
    const uint32_t* pre = nullptr;
    if (!t.link_identity) {
        TrajLinkScratch ls = {};
        Carver size(nullptr);
        carve_traj_link(size, ctx->n, &ls);
        const int mine = traj_scratch(ctx, size.bytes());
        if (!mine) {
            Carver place(t.scratch.get());
            carve_traj_link(place, ctx->n, &ls);
            HIPCHK(ctx, eslam_launch_traj_sources(ctx->ctl, updated ? 1 : 0, ctx->pt.anc, first, ctx->n, ls.src, ctx->stream));
        }
        rc = traj_fetch(ctx, mine, false, ls.src, ctx->n, t.link_table, link_src(t), ls.got);
        if (rc) return rc;
        pre = ls.got;
    }
    const uint32_t e = t.head;
    HIPCHK(ctx, eslam_launch_traj_record_sharded(ctx->st[0], ctx->st[1], ctx->ctl, ctx->n, updated ? 1 : 0, ctx->pt.anc, pre, first,
                                                 t.link[t.cur ^ 1u], &t.entry[e], ctx->stream));
    link_moved(ctx, true);
    t.count[e] = (uint32_t)ctx->n;
    t.gcount[e] = ctx->n_global;
    t.table[e] = ctx->gall;
    t.step[e] = t.next_step++;
    t.head = (e + 1u) % t.capacity;
    if (t.held < t.capacity) t.held++;
    return ESLAM_OK;
}

// The first collective of a sharded query: `nwords` words every rank must pass alike (its
// arguments) and this rank's status so far.  A failing rank keeps its code, the others return
// ESLAM_ERR_COMM; differing words are ESLAM_ERR_INVALID_ARG on every rank.
int query_agree(eslam_ctx* ctx, int mine, const uint64_t* words, uint32_t nwords, const char* what)
{
    const int G = ctx->comm.nranks;
    if (G == 1) return mine;
    constexpr uint32_t kW = kHostXBytes / 8;
    const std::string msg = ctx->err;
    uint64_t w[kW] = {(uint64_t)(int64_t)mine}, all[kW * kMaxRanks] = {};
    for (uint32_t q = 0; q < nwords && q + 1 < kW; ++q) w[q + 1] = words[q];
    const int crc = host_allgather(ctx, w, all, sizeof(w));
    if (mine) return fail(ctx, mine, msg.c_str());
    if (crc) return crc;
    for (int r = 0; r < G; ++r)
        if (all[kW * r])
            return fail(ctx, ESLAM_ERR_COMM, (std::string(what) + ": rank " + std::to_string(r) + " failed (" +
                                              std::to_string((int64_t)all[kW * r]) + ")").c_str());
    for (int r = 0; r < G; ++r)
        if (memcmp(all + kW * r, w, sizeof(w)) != 0)
            return fail(ctx, ESLAM_ERR_INVALID_ARG, (std::string(what) + ": the ranks passed different arguments").c_str());
    return ESLAM_OK;
}

// eslam_gpu_get_trajectories on a sharded filter.  The leaves are replicated: every rank walks
// all of them and receives the whole result.  The first fetch reads link[index] from the leaf's
// current owner; every level then fetches the slots' items (five values and the parent) from the
// entry's owners under the entry's own table.
int trajectories_sharded(eslam_ctx* ctx, const uint64_t* indices, uint64_t count, eslam_trajectory_pose* out, uint64_t capacity,
                         uint64_t* steps)
{
    TrajectoryLog& t = ctx->traj;
    const int G = ctx->comm.nranks;
    // what the arguments alone decide, before any collective
    if (count >= (1ull << 32)) return fail(ctx, ESLAM_ERR_INVALID_ARG, "get_trajectories: too many indices");
    for (uint64_t k = 0; k < count; ++k)
        if (indices[k] >= ctx->n_global)
            return fail(ctx, ESLAM_ERR_INVALID_ARG, "get_trajectories: an index is not below the global particle count");
    const uint32_t m = (uint32_t)(t.held < capacity ? t.held : capacity);
    if (m && count && !out) return ESLAM_ERR_INVALID_ARG;
    // the scratch, then the ranks' counts, capacities and status in one all_gather
    TrajTraceSharded s = {};
    Carver size(nullptr);
    carve_traj_trace_sharded(size, count, m, G, &s);
    int rc = check_poisoned(ctx);
    if (!rc) rc = traj_scratch(ctx, size.bytes());
    const uint64_t words[2] = {count, capacity};
    rc = query_agree(ctx, rc, words, 2, "get_trajectories");
    if (rc) return rc;
    if (const int rc_ = settle(ctx)) return rc_;
    if (!count) return ESLAM_OK;
    Carver place(t.scratch.get());
    carve_traj_trace_sharded(place, count, m, G, &s);
    std::vector<uint32_t> leaf(count);
    for (uint64_t k = 0; k < count; ++k) leaf[k] = (uint32_t)indices[k];
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(s.leaf, leaf.data(), count * 4, hipMemcpyHostToDevice));
    if (G > 1) {                                     // the lists' contents
        rc = comm_allgather(ctx, s.leaf, s.all, count * 4);
        if (rc) return rc;
        std::vector<uint32_t> all(count * G);
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(all.data(), s.all, all.size() * 4, hipMemcpyDeviceToHost));
        for (int r = 0; r < G; ++r)
            if (memcmp(all.data() + count * r, leaf.data(), count * 4) != 0)
                return fail(ctx, ESLAM_ERR_INVALID_ARG, "get_trajectories: the ranks passed different indices");
    }
    if (!m) return ESLAM_OK;
    rc = materialize(ctx);                           // like the other queries; the log's link already stands
    if (rc) return rc;
    rc = traj_fetch(ctx, ESLAM_OK, false, s.leaf, count, t.link_table, link_src(t), s.a);
    for (uint32_t j = 0; j < m && !rc; ++j) {        // newest first; s.a moves one entry back per level
        const uint32_t ring = t.at(j);
        rc = traj_fetch(ctx, ESLAM_OK, true, s.a, count, t.table[ring], entry_src(t, ring, nullptr), s.items);
        if (!rc) HIPCHK(ctx, eslam_launch_traj_trace_take(s.items, count, (uint32_t)t.gcount[ring], s.a, m, j, s.nodes, ctx->stream));
    }
    if (rc) return rc;
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
            o.particles = t.gcount[ring];
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

// eslam_gpu_trajectory_smoothed on a sharded filter: the sweep over this rank's leaves.  Per
// level the items come through traj_fetch, whose owners mark the slots they serve in a bitmap over
// their own part of the entry; the ranks' population counts add up to the distinct ancestors, and
// the scratch state goes through the sharded passes of pose_moments_of under the current weights.
int smoothed_sharded(eslam_ctx* ctx, eslam_trajectory_estimate* out, uint64_t capacity, uint64_t* entries)
{
    TrajectoryLog& t = ctx->traj;
    const int G = ctx->comm.nranks;
    const uint32_t m = (uint32_t)(t.held < capacity ? t.held : capacity);
    if (m && !out) return ESLAM_ERR_INVALID_ARG;
    const uint64_t n = ctx->n;
    TrajSmoothScratch s = {};
    TrajItem* items = nullptr;
    Carver size(nullptr);
    carve_traj_smooth(size, n, t.max_particles, &s);
    items = size.take<TrajItem>(n);
    int rc = check_poisoned(ctx);
    if (!rc) rc = traj_scratch(ctx, size.bytes());
    const uint64_t words[1] = {capacity};
    rc = query_agree(ctx, rc, words, 1, "trajectory_smoothed");
    if (rc) return rc;
    if (const int rc_ = settle(ctx)) return rc_;
    if (!m) return ESLAM_OK;
    rc = materialize(ctx);                           // the particles and weights as they stand
    if (!rc) rc = read_ctl(ctx);
    if (rc) return rc;
    Carver place(t.scratch.get());
    carve_traj_smooth(place, n, t.max_particles, &s);
    items = place.take<TrajItem>(n);
    DevState S;
    memset(&S, 0, sizeof(S));
    S.x = s.x; S.y = s.y; S.th = s.th; S.z = s.z; S.zs = s.zs; S.w = s.w;
    const DevState& cur = ctx->st[ctx->ctl_host->base ^ ctx->ctl_host->flip];
    HIPCHK(ctx, hipMemcpyAsync(s.w, cur.w, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s.a, t.link[t.cur], n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    for (uint32_t j = 0; j < m; ++j) {               // newest first; s.a moves one entry back per level
        const uint32_t ring = t.at(j);
        const uint64_t words_j = ((uint64_t)t.count[ring] + 63) / 64;
        eslam_trajectory_estimate& o = out[m - 1u - j];
        memset(&o, 0, sizeof(o));
        o.step = t.step[ring];
        HIPCHK(ctx, hipMemsetAsync(s.k.bits, 0, words_j * sizeof(uint64_t), ctx->stream));
        rc = traj_fetch(ctx, ESLAM_OK, true, s.a, n, t.table[ring], entry_src(t, ring, s.k.bits), items);
        if (rc) return rc;
        HIPCHK(ctx, eslam_launch_traj_level_take(items, n, s.a, S, ctx->stream));
        HIPCHK(ctx, eslam_launch_kld_popcount(s.k.bits, words_j, s.k.part, s.k.out, ctx->stream));
        MomPass P;
        memset(&P, 0, sizeof(P));
        rc = pose_moments_of(ctx, S, S, P, ESLAM_OK, &o.moments);
        if (rc) return rc;
        int64_t rec[kKldWords];
        HIPCHK(ctx, hipMemcpy(rec, s.k.out, sizeof(rec), hipMemcpyDeviceToHost));   // the passes have synchronised
        uint64_t marked[kMaxRanks] = {(uint64_t)rec[kKldCounted]};
        if (G > 1) {                                 // a word per rank: the owners' marked bits
            const uint64_t own = marked[0];
            rc = host_allgather(ctx, &own, marked, 8);
            if (rc) return rc;
        }
        for (int r = 0; r < G; ++r) o.distinct_ancestors += marked[r];
    }
    *entries = m;
    return ESLAM_OK;
}
}  // namespace

int eslam_host::trajectory_reset(eslam_ctx* ctx)
{
    TrajectoryLog& t = ctx->traj;
    t.head = t.held = 0;
    t.cur = 0;
    t.link_n = ctx->n;
    if (t.sharded) {
        t.link_table = ctx->gall;
        t.link_identity = true;
        HIPCHK(ctx, eslam_launch_traj_iota_from(t.link[0], t.link_n, (uint32_t)ctx->gbase, ctx->stream));
        return ESLAM_OK;
    }
    HIPCHK(ctx, eslam_launch_traj_iota(t.link[0], t.link_n, ctx->stream));
    return ESLAM_OK;
}

int eslam_host::trajectory_record(eslam_ctx* ctx, bool updated)
{
    TrajectoryLog& t = ctx->traj;
    if (ctx->n > t.max_particles) return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory: more particles than the log's max_particles");
    if (t.sharded) return record_sharded(ctx, updated);
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
    if (t.sharded) {
        // pt.anc: old global indices, slots of the layout link[cur] is indexed under (the old table)
        const int rc = traj_fetch(ctx, ESLAM_OK, false, ctx->pt.anc, ctx->n, t.link_table, link_src(t), t.link[t.cur ^ 1u]);
        if (rc) return rc;
        link_moved(ctx, false);
        return ESLAM_OK;
    }
    HIPCHK(ctx, eslam_launch_traj_compose(ctx->pt.anc, t.link[t.cur], t.link_n, t.link[t.cur ^ 1u], ctx->n, ctx->stream));
    t.cur ^= 1u;
    t.link_n = ctx->n;
    return ESLAM_OK;
}

namespace {
// the log's slots per entry, or what is wrong with the request
int enable_slots(eslam_ctx* ctx, uint64_t max_particles, uint64_t* slots)
{
    *slots = max_particles ? max_particles : (ctx->n ? ctx->cap : 0);
    if (*slots == 0) return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory_enable: max_particles 0 needs an initialised filter");
    if (*slots >= (1ull << 32) - 1 || *slots < ctx->n)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory_enable: max_particles must hold the current particles and be below 2^32 - 1");
    return ESLAM_OK;
}

// everything an enable allocates, into t and anc: a failure leaves the context as it was
int enable_alloc(eslam_ctx* ctx, uint32_t capacity_steps, uint64_t slots, TrajectoryLog& t, Dev<uint32_t>& anc)
{
    uint32_t* link[2];
    Carver size(nullptr);
    carve_traj_log(size, capacity_steps, slots, nullptr, link);
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
    return ESLAM_OK;
}

int enable_commit(eslam_ctx* ctx, TrajectoryLog& t, Dev<uint32_t>& anc)
{
    if (anc) ctx->pt.anc = std::move(anc);           // kept from now on, as with ESLAM_FLAG_RECORD_ANCESTORS
    ctx->traj = std::move(t);
    return trajectory_reset(ctx);
}
}  // namespace

extern "C" int eslam_gpu_trajectory_enable(eslam_ctx* ctx, uint32_t capacity_steps, uint64_t max_particles)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (ctx->sharded)
        return fail(ctx, ESLAM_ERR_UNSUPPORTED,
                    "trajectory_enable: on a sharded filter the log is enabled by eslam_gpu_trajectory_enable_sharded, a collective");
    if (capacity_steps == 0) return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory_enable: capacity_steps must be at least 1");
    uint64_t slots = 0;
    if (const int rc_ = enable_slots(ctx, max_particles, &slots)) return rc_;
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    // a gather pending from before the log runs now: the link starts as the identity over the
    // particles as they stand
    if (const int rc_ = materialize(ctx)) return rc_;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    TrajectoryLog t;
    Dev<uint32_t> anc;
    if (const int rc_ = enable_alloc(ctx, capacity_steps, slots, t, anc)) return rc_;
    return enable_commit(ctx, t, anc);
}

// The same on a sharded filter: a collective.  max_particles is this rank's.  One all_gather of
// (status, capacity_steps, slots) before anything changes: a rank that cannot enable returns its
// own code and the others ESLAM_ERR_COMM; ranks that disagree on capacity_steps all return
// ESLAM_ERR_INVALID_ARG.
extern "C" int eslam_gpu_trajectory_enable_sharded(eslam_ctx* ctx, uint32_t capacity_steps, uint64_t max_particles)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (!ctx->sharded) return eslam_gpu_trajectory_enable(ctx, capacity_steps, max_particles);
    if (capacity_steps == 0) return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory_enable: capacity_steps must be at least 1");
    const int G = ctx->comm.nranks;
    uint64_t slots = 0;
    int mine = settle(ctx);                          // in SPMD order every rank has the same exchange pending
    if (!mine) mine = enable_slots(ctx, max_particles, &slots);
    if (!mine) mine = check_poisoned(ctx);
    if (!mine) mine = materialize(ctx);
    if (!mine && hipStreamSynchronize(ctx->stream) != hipSuccess) mine = fail(ctx, ESLAM_ERR_HIP, "trajectory_enable: the stream failed");
    TrajectoryLog t;
    Dev<uint32_t> anc;
    if (!mine) mine = enable_alloc(ctx, capacity_steps, slots, t, anc);
    const std::string msg = ctx->err;
    static_assert(3 * 8 <= kHostXBytes, "host_allgather's buffer holds the enable's words");
    const uint64_t words[3] = {(uint64_t)(int64_t)mine, capacity_steps, slots};
    uint64_t all[3 * kMaxRanks] = {};
    const int crc = host_allgather(ctx, words, all, sizeof(words));
    if (mine) return fail(ctx, mine, msg.c_str());
    if (crc) return crc;
    for (int r = 0; r < G; ++r)
        if (all[3 * r])
            return fail(ctx, ESLAM_ERR_COMM, ("trajectory_enable: rank " + std::to_string(r) + " failed (" +
                                              std::to_string((int64_t)all[3 * r]) + ")").c_str());
    for (int r = 0; r < G; ++r)
        if (all[3 * r + 1] != capacity_steps)
            return fail(ctx, ESLAM_ERR_INVALID_ARG, "trajectory_enable: the ranks passed different capacity_steps");
    t.sharded = true;
    t.gcount.assign(capacity_steps, 0);
    t.table.assign(capacity_steps, std::vector<uint64_t>());
    for (int r = 0; r < G; ++r) t.max_all.push_back(all[3 * r + 2]);
    return enable_commit(ctx, t, anc);
}

// a resample of a sharded filter to the table nb: whether every rank's log has room for its new shard
bool eslam_host::trajectory_holds(const eslam_ctx* ctx, const uint64_t* nb)
{
    const TrajectoryLog& t = ctx->traj;
    if (!t.on || !t.sharded) return true;
    for (int r = 0; r < ctx->comm.nranks; ++r)
        if (nb[r + 1] - nb[r] > t.max_all[r]) return false;
    return true;
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
    // particles as they stand are the lineages' new start.  On a sharded filter a collective
    // in SPMD order (a deferred exchange is settled); every rank resets alike, nothing travels
    if (const int rc_ = settle(ctx)) return rc_;
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
        info->particles = t.sharded ? t.gcount[t.at(0)] : t.count[t.at(0)];
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
    if (t.sharded) return trajectories_sharded(ctx, indices, count, out, capacity, steps);
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
    if (t.sharded) return smoothed_sharded(ctx, out, capacity, entries);
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
