// eslam_host_comm.hip -- host side of libeslam_gpu: the multi-GPU plumbing.  The collectives the
// host side goes through (the user's callbacks, in device or host memory), eslam_gpu_set_comm, and
// the library's own RCCL transport (eslam_gpu_set_comm_rccl).  No kernels.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <string.h>

#include <string>

#include "eslam_ctx.h"

// ---------------------------------------------------------------------------------------
// multi-GPU plumbing: the three exchanges of an update go through the user's collectives
// ---------------------------------------------------------------------------------------
// all_gather of `bytes` per rank from device memory into device memory
int eslam_host::comm_allgather(eslam_ctx* ctx, const void* dsend, void* drecv, uint64_t bytes)
{
    const eslam_comm& c = ctx->comm;
    if (c.device_memory) {
        if (c.allgather(c.user, dsend, drecv, bytes, (void*)ctx->stream) != 0)
            return fail(ctx, ESLAM_ERR_COMM, "allgather callback failed");
        return ESLAM_OK;
    }
    int rc = grow(ctx, ctx->stage, bytes * (c.nranks + 1));
    if (rc) return rc;
    char* h = ctx->stage.as<char>();
    HIPCHK(ctx, hipMemcpyAsync(h, dsend, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (c.allgather(c.user, h, h + bytes, bytes, nullptr) != 0) return fail(ctx, ESLAM_ERR_COMM, "allgather callback failed");
    HIPCHK(ctx, hipMemcpyAsync(drecv, h + bytes, bytes * c.nranks, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // the staging buffer is reused
    return ESLAM_OK;
}

int eslam_host::comm_alltoallv(eslam_ctx* ctx, const void* dsend, const uint64_t* sb, void* drecv, const uint64_t* rb,
                               hipStream_t stream)
{
    const eslam_comm& c = ctx->comm;
    if (!stream) stream = ctx->stream;
    if (c.device_memory) {
        if (c.alltoallv(c.user, dsend, sb, drecv, rb, (void*)stream) != 0)
            return fail(ctx, ESLAM_ERR_COMM, "alltoallv callback failed");
        return ESLAM_OK;
    }
    uint64_t ts = 0, tr = 0;
    for (int r = 0; r < c.nranks; ++r) { ts += sb[r]; tr += rb[r]; }
    int rc = grow(ctx, ctx->stage, ts + tr + 64);
    if (rc) return rc;
    char* h = ctx->stage.as<char>();
    char* hr = h + ((ts + 63) & ~63ull);
    if (ts) HIPCHK(ctx, hipMemcpyAsync(h, dsend, ts, hipMemcpyDeviceToHost, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    if (c.alltoallv(c.user, h, sb, hr, rb, nullptr) != 0) return fail(ctx, ESLAM_ERR_COMM, "alltoallv callback failed");
    if (tr) HIPCHK(ctx, hipMemcpyAsync(drecv, hr, tr, hipMemcpyHostToDevice, stream));
    HIPCHK(ctx, hipStreamSynchronize(stream));
    return ESLAM_OK;
}

int eslam_host::host_allgather(eslam_ctx* ctx, const void* send, void* recv, uint64_t bytes)
{
    const eslam_comm& c = ctx->comm;
    if (!c.device_memory) {
        if (c.allgather(c.user, send, recv, bytes, nullptr) != 0) return fail(ctx, ESLAM_ERR_COMM, "allgather callback failed");
        return ESLAM_OK;
    }
    if (bytes > kHostXBytes) return fail(ctx, ESLAM_ERR_INVALID_ARG, "host_allgather: more words than set_comm sized the buffer for");
    char* d = ctx->hostx;
    HIPCHK(ctx, hipMemcpyAsync(d, send, bytes, hipMemcpyHostToDevice, ctx->stream));
    const int rc = comm_allgather(ctx, d, d + bytes, bytes);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(recv, d + bytes, bytes * c.nranks, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ESLAM_OK;
}

int eslam_host::same_on_every_rank(eslam_ctx* ctx, const uint64_t* mine, uint32_t nwords, const char* msg)
{
    uint64_t all[kHostXBytes / 8 * kMaxRanks] = {};
    if (nwords * 8ull > kHostXBytes) return fail(ctx, ESLAM_ERR_INVALID_ARG, "host_allgather: more words than set_comm sized the buffer for");
    const int rc = host_allgather(ctx, mine, all, nwords * 8ull);
    if (rc) return rc;
    for (int r = 0; r < ctx->comm.nranks; ++r)
        if (memcmp(all + (uint64_t)nwords * r, mine, nwords * 8ull) != 0) return fail(ctx, ESLAM_ERR_INVALID_ARG, msg);
    return ESLAM_OK;
}

int eslam_host::agree(eslam_ctx* ctx, int rc, const char* what)
{
    if (!ctx->sharded) return rc;
    const std::string msg = ctx->err;
    const int64_t mine = rc;
    int64_t all[kMaxRanks] = {};
    const int crc = host_allgather(ctx, &mine, all, 8);
    if (rc) {
        ctx->err = msg;
        return rc;
    }
    if (crc) return crc;
    for (int r = 0; r < ctx->comm.nranks; ++r)
        if (all[r])
            return fail(ctx, ESLAM_ERR_COMM,
                        (std::string(what) + ": rank " + std::to_string(r) + " failed (" + std::to_string(all[r]) + ")").c_str());
    return ESLAM_OK;
}

void eslam_host::chunk_shape(const uint64_t* gall, int G, uint32_t J, uint64_t* nch, uint64_t* maxch, uint64_t* total)
{
    const uint64_t csz = 64ull * J;
    *maxch = 1;
    *total = 0;
    for (int r = 0; r < G; ++r) {
        const uint64_t c = (gall[r + 1] - gall[r] + csz - 1) / csz;
        if (nch) nch[r] = c;
        *maxch = c > *maxch ? c : *maxch;
        *total += c;
    }
}

int eslam_host::gather_chunks(eslam_ctx* ctx, const uint64_t* nch, uint64_t maxch, uint32_t R, const double* mine, double* all,
                              double* a)
{
    const int rc = comm_allgather(ctx, mine, all, maxch * R * sizeof(double));
    if (rc) return rc;
    hipError_t e = hipSuccess;
    uint64_t off = 0;
    for (int r = 0; r < ctx->comm.nranks && e == hipSuccess; ++r) {
        if (nch[r]) e = hipMemcpyAsync(a + off * R, all + (uint64_t)r * maxch * R, nch[r] * R * sizeof(double),
                                       hipMemcpyDeviceToDevice, ctx->stream);
        off += nch[r];
    }
    if (e != hipSuccess) return fail(ctx, ESLAM_ERR_HIP, hipGetErrorString(e));
    return ESLAM_OK;
}

// sharded getCentroid: this rank's chunk records (padded to the largest shard), all ranks'
// (G x that), and the tree's two ping-pong levels over the global chunks; 5 doubles a record
uint64_t eslam_host::centroid_bytes(const uint64_t* gall, int G, uint32_t J)
{
    uint64_t maxch, total;
    chunk_shape(gall, G, J, nullptr, &maxch, &total);
    return (maxch + (uint64_t)G * maxch + 2 * (total ? total : 1)) * 5 * sizeof(double);
}

// A shard table takes effect in two parts, shared by eslam_gpu_set_comm and the resample of a
// sharded filter to another count.  reserve: everything sized by the table that may fail
// (getCentroid's buffer, allocated here so the per-step getCentroid of a Rock task allocates
// nothing), with the context's table still the old one.  apply: reserve, then the table itself:
// gall, n_global and gbase; the cached A^n_global follows n_global (fin_params).  Neither
// touches the particles.
int eslam_host::reserve_shard_table(eslam_ctx* ctx, int nranks, uint64_t n_global, const uint64_t* shard_gbase)
{
    const uint64_t need = centroid_bytes(shard_gbase, nranks, dm_chunk_rows_cfg(n_global, ctx->cfg.sum_chunk_rows));
    if (need <= ctx->cent.cap()) return ESLAM_OK;
    hipError_t he = hipSuccess;
    const int rc = ctx->cent.grow_keep(need, 1, ctx->stream, &he);
    if (rc == ESLAM_ERR_HIP) return fail(ctx, rc, hipGetErrorString(he));
    if (rc) return fail(ctx, rc, "no device memory for getCentroid's chunk records");
    return ESLAM_OK;
}

int eslam_host::apply_shard_table(eslam_ctx* ctx, int nranks, int rank, uint64_t n_global, const uint64_t* shard_gbase)
{
    if (const int rc = reserve_shard_table(ctx, nranks, n_global, shard_gbase)) return rc;
    ctx->gall.assign(shard_gbase, shard_gbase + nranks + 1);
    ctx->n_global = n_global;
    ctx->gbase = shard_gbase[rank];
    return ESLAM_OK;
}

extern "C" int eslam_gpu_set_comm(eslam_ctx* ctx, const eslam_comm* comm, uint64_t n_global, const uint64_t* shard_gbase)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (comm && ctx->traj.on)
        return fail(ctx, ESLAM_ERR_UNSUPPORTED, "eslam_gpu_set_comm: a filter with a trajectory log cannot be sharded (disable the log first)");
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    free_particles(ctx);
    if (ctx->statics_sharded) g_statics_sharded.fetch_sub(1);
    ctx->statics_sharded = false;
    if (!comm) {
        ctx->sharded = false;
        ctx->gall.clear();
        ctx->gbase = 0;
        ctx->n_global = 0;
        return ESLAM_OK;
    }
    if (!shard_gbase || !comm->allgather || !comm->alltoallv || comm->nranks < 1 || comm->nranks > kMaxRanks ||
        comm->rank < 0 || comm->rank >= comm->nranks)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "eslam_gpu_set_comm: bad communicator (1 <= nranks <= 16)");
    if (n_global == 0 || n_global > (1ull << 30) - 64)     // resample mark encoding (kMarkOwn)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "eslam_gpu_set_comm: n_global must be in [1, 2^30 - 64]");
    const uint64_t csz = 64ull * dm_chunk_rows_cfg(n_global, ctx->cfg.sum_chunk_rows);
    if (shard_gbase[0] != 0 || shard_gbase[comm->nranks] != n_global)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "eslam_gpu_set_comm: shard_gbase must run from 0 to n_global");
    for (int r = 0; r < comm->nranks; ++r) {
        if (shard_gbase[r + 1] <= shard_gbase[r])
            return fail(ctx, ESLAM_ERR_INVALID_ARG, "eslam_gpu_set_comm: every shard needs at least one particle");
        if (shard_gbase[r] % csz)
            return fail(ctx, ESLAM_ERR_INVALID_ARG, "eslam_gpu_set_comm: shard starts must be multiples of the summation chunk");
    }
    if (!ctx->mg) {
        HIPCHK(ctx, ctx->recs.alloc(sizeof(Shard) * kNShard * kMaxRanks));
        HIPCHK(ctx, ctx->mg.alloc(mg::kWords * 8));
        HIPCHK(ctx, ctx->mg_host.alloc(mg::kWords * 8));
        HIPCHK(ctx, hipMemset(ctx->recs, 0, sizeof(Shard) * kNShard * kMaxRanks));
        HIPCHK(ctx, hipMemset(ctx->mg, 0, mg::kWords * 8));
    }
    // host_allgather's buffer: its own words and every rank's, so no collective allocates
    if (!ctx->hostx) HIPCHK(ctx, ctx->hostx.alloc(kHostXBytes * (kMaxRanks + 1)));
    if (const int rc_ = reserve_shard_table(ctx, comm->nranks, n_global, shard_gbase)) return rc_;
    if ((ctx->cfg.flags & ESLAM_FLAG_PROCESS_STATICS) && comm->nranks > 1) {
        if (g_statics_sharded.fetch_add(1) != 0) {
            g_statics_sharded.fetch_sub(1);
            return fail(ctx, ESLAM_ERR_INVALID_ARG,
                        "eslam_gpu_set_comm: ESLAM_FLAG_PROCESS_STATICS allows one sharded context per process "
                        "(ranks in one process would share the respawn counter and rand())");
        }
        ctx->statics_sharded = true;
    }
    ctx->comm = *comm;
    ctx->sharded = true;
    return apply_shard_table(ctx, comm->nranks, comm->rank, n_global, shard_gbase);
}

// the canonical table: near-equal shards whose starts are multiples of the summation chunk
extern "C" int eslam_gpu_shard_bounds(uint64_t n_global, int32_t nranks, uint32_t sum_chunk_rows, uint64_t* bounds_out)
{
    if (!bounds_out || nranks < 1 || n_global == 0) return ESLAM_ERR_INVALID_ARG;
    const uint64_t csz = 64ull * dm_chunk_rows_cfg(n_global, sum_chunk_rows);
    const uint64_t chunks = (n_global + csz - 1) / csz, G = (uint64_t)nranks;
    if (chunks < G) return ESLAM_ERR_INVALID_ARG;      // fewer chunks than ranks: some shard would be empty
    for (uint64_t r = 0; r < G; ++r) {
        const uint64_t b = (chunks * r / G) * csz;
        bounds_out[r] = b < n_global ? b : n_global;
    }
    bounds_out[G] = n_global;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_get_shard_bounds(eslam_ctx* ctx, uint64_t* bounds_out, uint32_t capacity)
{
    if (!ctx || !bounds_out) return ESLAM_ERR_INVALID_ARG;
    if (!ctx->sharded) return fail(ctx, ESLAM_ERR_INVALID_ARG, "eslam_gpu_get_shard_bounds: the context is not sharded");
    if (capacity < ctx->gall.size())
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "eslam_gpu_get_shard_bounds: room for nranks + 1 entries is needed");
    memcpy(bounds_out, ctx->gall.data(), ctx->gall.size() * sizeof(uint64_t));
    return ESLAM_OK;
}

// ---------------------------------------------------------------------------------------
// RCCL transport (eslam_gpu_set_comm_rccl): the eslam_comm callbacks implemented in C++ on
// the context's stream, RCCL resolved at run time (the process's librccl.so.1 -- the one
// torch loaded, if any -- so one RCCL serves both)
// ---------------------------------------------------------------------------------------
namespace {
struct RcclApi {
    bool ok = false;
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
};

const RcclApi& rccl_api()
{
    static RcclApi api = [] {
        RcclApi a;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return a;
#define ESLAM_SYM(f, name) a.f = reinterpret_cast<decltype(a.f)>(dlsym(h, name))
        ESLAM_SYM(get_unique_id, "ncclGetUniqueId");
        ESLAM_SYM(comm_init_rank, "ncclCommInitRank");
        ESLAM_SYM(comm_destroy, "ncclCommDestroy");
        ESLAM_SYM(all_gather, "ncclAllGather");
        ESLAM_SYM(send, "ncclSend");
        ESLAM_SYM(recv, "ncclRecv");
        ESLAM_SYM(group_start, "ncclGroupStart");
        ESLAM_SYM(group_end, "ncclGroupEnd");
        ESLAM_SYM(error_string, "ncclGetErrorString");
#undef ESLAM_SYM
        a.ok = a.get_unique_id && a.comm_init_rank && a.comm_destroy && a.all_gather && a.send && a.recv &&
               a.group_start && a.group_end && a.error_string;
        return a;
    }();
    return api;
}

int rccl_allgather_cb(void* user, const void* send, void* recv, uint64_t bytes, void* stream)
{
    eslam_ctx* ctx = static_cast<eslam_ctx*>(user);
    const RcclApi& a = rccl_api();
    return a.all_gather(send, recv, bytes, ncclUint8, static_cast<ncclComm_t>(ctx->rccl), static_cast<hipStream_t>(stream)) ==
                   ncclSuccess ? 0 : 1;
}

int rccl_alltoallv_cb(void* user, const void* send, const uint64_t* send_bytes, void* recv, const uint64_t* recv_bytes,
                      void* stream)
{
    eslam_ctx* ctx = static_cast<eslam_ctx*>(user);
    const RcclApi& a = rccl_api();
    const ncclComm_t comm = static_cast<ncclComm_t>(ctx->rccl);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t so = 0, ro = 0;
    if (a.group_start() != ncclSuccess) return 1;
    int bad = 0;
    for (int r = 0; r < ctx->comm.nranks; ++r) {
        if (send_bytes[r]) bad |= a.send(static_cast<const char*>(send) + so, send_bytes[r], ncclUint8, r, comm, st) != ncclSuccess;
        if (recv_bytes[r]) bad |= a.recv(static_cast<char*>(recv) + ro, recv_bytes[r], ncclUint8, r, comm, st) != ncclSuccess;
        so += send_bytes[r];
        ro += recv_bytes[r];
    }
    bad |= a.group_end() != ncclSuccess;
    return bad;
}

}  // namespace

void eslam_host::rccl_release(eslam_ctx* ctx)
{
    if (ctx->rccl) rccl_api().comm_destroy(static_cast<ncclComm_t>(ctx->rccl));
    ctx->rccl = nullptr;
}

extern "C" int eslam_gpu_rccl_unique_id(uint8_t id[ESLAM_RCCL_ID_BYTES])
{
    if (!id) return ESLAM_ERR_INVALID_ARG;
    const RcclApi& a = rccl_api();
    if (!a.ok) return ESLAM_ERR_UNSUPPORTED;
    ncclUniqueId u;
    if (a.get_unique_id(&u) != ncclSuccess) return ESLAM_ERR_COMM;
    static_assert(sizeof(u) == ESLAM_RCCL_ID_BYTES, "ncclUniqueId size");
    memcpy(id, &u, sizeof(u));
    return ESLAM_OK;
}

extern "C" int eslam_gpu_set_comm_rccl(eslam_ctx* ctx, int32_t nranks, int32_t rank, const uint8_t id[ESLAM_RCCL_ID_BYTES],
                                       uint64_t n_global, const uint64_t* shard_gbase)
{
    if (!ctx || !id) return ESLAM_ERR_INVALID_ARG;
    if (ctx->traj.on)
        return fail(ctx, ESLAM_ERR_UNSUPPORTED, "eslam_gpu_set_comm_rccl: a filter with a trajectory log cannot be sharded (disable the log first)");
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    const RcclApi& a = rccl_api();
    if (!a.ok) return fail(ctx, ESLAM_ERR_UNSUPPORTED, "eslam_gpu_set_comm_rccl: librccl.so.1 not found");
    if (nranks < 1 || nranks > kMaxRanks || rank < 0 || rank >= nranks)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "eslam_gpu_set_comm_rccl: bad communicator (1 <= nranks <= 16)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    rccl_release(ctx);
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = a.comm_init_rank(&comm, nranks, u, rank);
    if (r != ncclSuccess)
        return fail(ctx, ESLAM_ERR_COMM, (std::string("ncclCommInitRank: ") + a.error_string(r)).c_str());
    ctx->rccl = comm;
    eslam_comm c;
    memset(&c, 0, sizeof(c));
    c.user = ctx;
    c.rank = rank;
    c.nranks = nranks;
    c.device_memory = 1;
    c.allgather = rccl_allgather_cb;
    c.alltoallv = rccl_alltoallv_cb;
    const int rc = eslam_gpu_set_comm(ctx, &c, n_global, shard_gbase);
    if (rc) rccl_release(ctx);
    return rc;
}
