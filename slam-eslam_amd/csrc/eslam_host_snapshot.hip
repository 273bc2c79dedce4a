// eslam_host_snapshot.hip -- host side of libeslam_gpu: eslam_gpu_save / eslam_gpu_load and their
// stream and positional forms (the blob's layout, the plan, the writer and the reader).  No kernels:
// those are in eslam_snapshot.hip.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "eslam_ctx.h"
#include "eslam_scratch.h"

// ---------------------------------------------------------------------------------------
// snapshots: eslam_gpu_save / eslam_gpu_load (kernels in eslam_snapshot.hip)
// ---------------------------------------------------------------------------------------
namespace {

const char kSnapMagic[8] = {'E', 'S', 'L', 'A', 'M', 'S', 'N', 'P'};
enum { kSecGrid = 0, kSecHash, kSecParticles, kSecScalars, kSecMaps, kSecCount };   // bit k of SnapHeader::sections
struct SnapSection {
    uint64_t off, size;
};
struct SnapHeader {
    char magic[8];
    uint32_t version, sections;
    uint64_t bytes;
    uint64_t n;
    uint32_t particle_maps, local_map_trail;
    uint32_t hx, hy;                         // the window's half-widths (0 without per-particle maps)
    double max_sensor_range;
    uint32_t width, height;
    double scale_x, scale_y, offset_x, offset_y;
    double g2l[12];
    uint64_t n_patches;
    uint32_t has_height, hash_bins;
    uint64_t hash_n;
    uint64_t tables, pages;
    uint32_t wx, wy;
    uint32_t row_words, pad;
    SnapSection sec[kSecCount];
    uint64_t reserved;
};
static_assert(sizeof(SnapHeader) == 336, "snapshot header");
struct SnapScalars {
    eslam_rng_state rng;
    uint64_t pad;
    int32_t wexp;
    uint32_t minstd;
    double max_weight;
    uint64_t update_count;
    double inv_n;
};
static_assert(sizeof(eslam_rng_state) == 280 && sizeof(SnapScalars) == 320, "snapshot scalars");

inline uint64_t pad16(uint64_t b) { return (b + 15) & ~(uint64_t)15; }
inline uint32_t snap_row_words(uint32_t W, uint32_t V) { return (4u + W + 3u * V + 3u) & ~3u; }
constexpr uint64_t kPageBytes = DM_LM_PAGE_CELLS * sizeof(float2);

// the sections' offsets and sizes that the header's counts imply (the one layout a blob may have)
void snap_layout(const SnapHeader& h, SnapSection sec[kSecCount], uint64_t* bytes)
{
    uint64_t at = sizeof(SnapHeader);
    const uint64_t ncell = (uint64_t)h.width * h.height, np = h.n_patches, n = h.n;
    uint64_t size[kSecCount];
    size[kSecGrid] = pad16((ncell + 1) * 4) + pad16(np * 8) + (h.has_height ? pad16(np * 4) : 0);
    size[kSecHash] = 4 * pad16(h.hash_n * 8) + pad16(h.hash_n * 4) + pad16((uint64_t)h.hash_bins * h.hash_bins * 4);
    size[kSecParticles] = 7 * pad16(n * 8) + pad16(n);
    size[kSecScalars] = sizeof(SnapScalars);
    size[kSecMaps] = pad16(n * 4) + pad16(h.tables * h.row_words * 4) + pad16(h.pages * 4) + h.pages * kPageBytes;
    for (int k = 0; k < kSecCount; ++k) {
        sec[k] = SnapSection{0, 0};
        if (!(h.sections & (1u << k))) continue;
        sec[k] = SnapSection{at, size[k]};
        at += size[k];
    }
    *bytes = at;
}

enum PieceKind { PK_HOST = 0, PK_DEV, PK_SID, PK_TABLES, PK_OWNER, PK_PAGES };
// one array of the blob, or the part of it this rank writes: count units of unit bytes at blob
// offset off (then tail zeros, up to 16 bytes, where the part ends the array)
struct Piece {
    int kind;
    const void* src;                         // PK_HOST: host memory; PK_DEV: device memory
    uint64_t count, unit;
    uint64_t off = 0, tail = 0;
};
// the blob as positional writes and reads (the stream forms ignore the offset: their order is the blob's)
typedef std::function<int(uint64_t off, const void* data, uint64_t bytes)> SnapSink;
typedef std::function<int(uint64_t off, void* data, uint64_t bytes)> SnapSource;

struct SnapPlan {
    SnapHeader h;
    SnapScalars sc;
    std::vector<Piece> pieces;
    SnapCensus cen;
    const uint32_t* sid;
    std::vector<uint32_t> bsizes;            // the pose hash's bucket sizes
    uint64_t T = 0, P = 0;                   // this rank's live tables and pages (h.tables, h.pages: the filter's)
    uint32_t tbase = 0, pbase = 0;           // those of the ranks below (a sharded filter)
};

const char* const kSnapStreamSharded =
    "snapshot: a sharded filter is one file written and read by offset (eslam_gpu_save_at / eslam_gpu_load_at); "
    "a sequential stream cannot carry a part of it";

int snap_staging(eslam_ctx* ctx, uint64_t bytes)
{
    for (int k = 0; k < 2; ++k)
        HIPCHK(ctx, ctx->snap_ev[k].create(false));
    if (bytes <= ctx->snap_cap) return ESLAM_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 2; ++k) {
        ctx->snap_host[k].reset();
        ctx->snap_dev[k].reset();
    }
    ctx->snap_cap = 0;
    for (int k = 0; k < 2; ++k) {
        if (ctx->snap_host[k].alloc(bytes) != hipSuccess || ctx->snap_dev[k].alloc(bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "snapshot: no memory for the staging buffers (lower chunk_bytes)");
        }
    }
    ctx->snap_cap = bytes;
    return ESLAM_OK;
}

// the staging size for pieces of at most `largest` bytes with units of at most `unit` bytes
uint64_t snap_stage_bytes(uint64_t chunk, uint64_t largest, uint64_t unit)
{
    uint64_t b = chunk < largest ? chunk : largest;
    b = b < unit ? unit : b;
    return pad16(b < 4096 ? 4096 : b) + 16;  // a part's last chunk carries the whole array's padding
}

uint64_t snap_tiles(uint64_t items) { return (items + kCompactTileItems - 1) / kCompactTileItems; }

int snap_read_count(eslam_ctx* ctx, const uint32_t* dev, uint64_t* out)
{
    uint32_t* h = ctx->scratch_host.as<uint32_t>();
    HIPCHK(ctx, hipMemcpyAsync(h, dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *out = *h;
    return ESLAM_OK;
}

// the census of the per-particle maps: the live tables and pages, ranked (pl.cen), and their counts
int snap_census(eslam_ctx* ctx, SnapPlan& pl)
{
    const LocalMaps& lm = ctx->lm;
    SnapCensus& c = pl.cen;
    Carver size(nullptr);
    carve_census(size, lm.ntables, ctx->cap, lm.npages, &c);
    // kept until the maps are dropped (free_local_maps)
    if (!ctx->lmb.census && ctx->lmb.census.alloc(size.bytes()) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "snapshot: no device memory for the census");
    }
    Carver place(ctx->lmb.census.get());
    carve_census(place, lm.ntables, ctx->cap, lm.npages, &c);
    const uint64_t n = ctx->n, ttiles = snap_tiles(n);
    int rc = grow(ctx, ctx->lmb.counts, (ttiles + 1) * 4);
    if (rc) return rc;
    c.counts = ctx->lmb.counts;
    HIPCHK(ctx, eslam_launch_snap_census_tables(&lm, &c, pl.sid, n, ctx->stream));
    uint64_t T = 0, P = 0;
    rc = snap_read_count(ctx, c.counts + ttiles, &T);
    if (rc) return rc;
    const uint64_t ptiles = snap_tiles(T * (lm.wx * lm.wy + lm.V));
    if (ptiles >= 0xffffffffull) return fail(ctx, ESLAM_ERR_UNSUPPORTED, "snapshot: the page census has 2^32 tiles or more");
    rc = grow(ctx, ctx->lmb.counts, (ptiles + 1) * 4);
    if (rc) return rc;
    c.counts = ctx->lmb.counts;
    HIPCHK(ctx, eslam_launch_snap_census_pages(&lm, &c, T, ctx->stream));
    rc = snap_read_count(ctx, c.counts + ptiles, &P);
    if (rc) return rc;
    pl.T = pl.h.tables = T;
    pl.P = pl.h.pages = P;
    return ESLAM_OK;
}

// settle, run a pending gather, take the census: the header, the scalars and the pieces of a save
// this rank's part of the plan: everything but the counts of the other ranks
int snap_plan_local(eslam_ctx* ctx, SnapPlan& pl);
// the pieces this rank writes, in the blob's order
int snap_plan_pieces(eslam_ctx* ctx, SnapPlan& pl);

// On a sharded filter a collective: one all_gather of every rank's {code, tables, pages,
// n_patches, update_count, minstd}.  A rank whose own part failed takes part in it, so either
// every rank has a plan or every rank returns an error (its own, or ESLAM_ERR_COMM).
int snap_plan(eslam_ctx* ctx, SnapPlan& pl)
{
    if (const int rc_ = settle(ctx)) return rc_;
    int rc = snap_plan_local(ctx, pl);
    if (ctx->sharded) {
        const std::string msg = ctx->err;
        const int G = ctx->comm.nranks, me = ctx->comm.rank;
        const uint64_t mine[6] = {(uint64_t)(int64_t)rc, pl.T, pl.P, pl.h.n_patches, pl.sc.update_count, pl.sc.minstd};
        std::vector<uint64_t> all(6 * (size_t)G, 0);
        static_assert(sizeof(mine) <= kHostXBytes, "host_allgather's buffer");
        const int crc = host_allgather(ctx, mine, all.data(), sizeof(mine));
        if (rc) {
            ctx->err = msg;
            return rc;
        }
        if (crc) return crc;
        uint64_t T = 0, P = 0;
        for (int r = 0; r < G; ++r) {
            const uint64_t* q = &all[6 * (size_t)r];
            if (q[0]) return fail(ctx, ESLAM_ERR_COMM, ("snapshot: rank " + std::to_string(r) + " failed").c_str());
            if (q[3] != mine[3] || q[4] != mine[4] || q[5] != mine[5])
                return fail(ctx, ESLAM_ERR_COMM, "snapshot: the ranks' grids, update counts or generators differ (not one filter)");
            if (r == me) {
                pl.tbase = (uint32_t)T;
                pl.pbase = (uint32_t)P;
            }
            T += q[1];
            P += q[2];
        }
        if (T > ctx->n_global) return fail(ctx, ESLAM_ERR_COMM, "snapshot: the ranks hold more tables than the filter has particles");
        if (P >= 0xffffffffull) return fail(ctx, ESLAM_ERR_UNSUPPORTED, "snapshot: 2^32 - 1 live pages or more");
        pl.h.n = ctx->n_global;
        pl.h.tables = T;
        pl.h.pages = P;
        snap_layout(pl.h, pl.h.sec, &pl.h.bytes);
    }
    return snap_plan_pieces(ctx, pl);
}

int snap_plan_local(eslam_ctx* ctx, SnapPlan& pl)
{
    memset(&pl.h, 0, sizeof(pl.h));
    memset(&pl.sc, 0, sizeof(pl.sc));
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    if (!ctx->has_map) return fail(ctx, ESLAM_ERR_NO_ENVIRONMENT, "No environment attached.");
    int rc = materialize(ctx);
    if (!rc) rc = read_ctl(ctx);
    if (rc) return rc;
    const Ctl& ctl = *ctx->ctl_host;
    const DevState& s = ctx->st[ctl.base ^ ctl.flip];
    SnapHeader& h = pl.h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, kSnapMagic, 8);
    h.version = ESLAM_SNAPSHOT_VERSION;
    h.n = ctx->n;
    h.particle_maps = particle_maps(ctx) ? 1u : 0u;
    h.local_map_trail = ctx->cfg.local_map_trail;
    h.max_sensor_range = ctx->cfg.max_sensor_range;
    h.width = ctx->map.width;
    h.height = ctx->map.height_cells;
    h.scale_x = ctx->map_scale[0];
    h.scale_y = ctx->map_scale[1];
    h.offset_x = ctx->map.offset_x;
    h.offset_y = ctx->map.offset_y;
    memcpy(h.g2l, ctx->map.g2l, sizeof(h.g2l));
    h.n_patches = ctx->map_np;
    h.has_height = ctx->grid.height ? 1u : 0u;
    h.sections = (1u << kSecGrid) | (1u << kSecParticles) | (1u << kSecScalars);
    if (h.particle_maps) {
        h.hx = dm_lm_half(ctx->cfg.max_sensor_range, ctx->map_scale[0]);
        h.hy = dm_lm_half(ctx->cfg.max_sensor_range, ctx->map_scale[1]);
    }
    if (ctx->has_hash) {
        h.sections |= 1u << kSecHash;
        h.hash_n = ctx->hash_n;
        h.hash_bins = (uint32_t)ctx->cfg.hash_slope_bins;
        pl.bsizes.resize(ctx->hash_bstart.size() - 1);
        for (size_t b = 0; b + 1 < ctx->hash_bstart.size(); ++b) pl.bsizes[b] = ctx->hash_bstart[b + 1] - ctx->hash_bstart[b];
    }
    pl.sid = s.sid;
    if (ctx->lm_ready && ctx->n) {
        h.sections |= 1u << kSecMaps;
        h.wx = ctx->lm.wx;
        h.wy = ctx->lm.wy;
        h.row_words = snap_row_words(ctx->lm.wx * ctx->lm.wy, ctx->lm.V);
        rc = snap_census(ctx, pl);
        if (rc) return rc;
    }
    snap_layout(h, h.sec, &h.bytes);
    // the scalars: eslam_gpu_get_rng_state's, and what the next update reads of the control block
    SnapScalars& sc = pl.sc;
    memset(&sc, 0, sizeof(sc));
    sc.rng.minstd_x = ctl.minstd;
    sc.rng.project_count = ctx->proj_event;
    sc.rng.init_count = ctx->init_event;
    sc.rng.hash_count = *ctx->hash_ev;
    sc.rng.max_weight = ctl.max_weight;
    memcpy(sc.rng.ud_pose, ctx->ud_pose, sizeof(ctx->ud_pose));
    memcpy(sc.rng.libc_rand, ctx->libcp->r, sizeof(sc.rng.libc_rand));
    sc.rng.libc_rand_pos = ctx->libcp->i;
    sc.wexp = ctl.wexp;
    sc.minstd = ctl.minstd;
    sc.max_weight = ctl.max_weight;
    sc.update_count = ctl.update_count;
    sc.inv_n = ctl.inv_n;
    return ESLAM_OK;
}

// Every array of the blob is split by owner ("Sharded filters"): rank 0 writes
// what every rank holds alike (header, grid, hash, scalars); the particle arrays go by shard;
// tables and pages by the ranks' counts (rank-major order is the canonical order).  The zeros
// behind an array go with the rank that holds its last element.  Unsharded: everything.
int snap_plan_pieces(eslam_ctx* ctx, SnapPlan& pl)
{
    const SnapHeader& h = pl.h;
    const Ctl& ctl = *ctx->ctl_host;
    const DevState& s = ctx->st[ctl.base ^ ctl.flip];
    std::vector<Piece>& p = pl.pieces;
    const bool lead = !ctx->sharded || ctx->comm.rank == 0;
    uint64_t at = 0, mine = 0;
    // the array of `total` units at the blob's cursor: this rank writes [first, first + count)
    auto add = [&](int kind, const void* src, uint64_t total, uint64_t unit, uint64_t first, uint64_t count) {
        Piece q{kind, src, count, unit};
        q.off = at + first * unit;
        q.tail = (count && first + count == total) ? pad16(total * unit) - total * unit : 0;
        at += pad16(total * unit);
        mine += count * unit + q.tail;
        if (count) p.push_back(q);
    };
    auto whole = [&](int kind, const void* src, uint64_t total, uint64_t unit) { add(kind, src, total, unit, 0, lead ? total : 0); };
    const uint64_t ncell = (uint64_t)h.width * h.height, n = h.n, gb = ctx->sharded ? ctx->gbase : 0, nl = ctx->n;
    whole(PK_HOST, &pl.h, sizeof(SnapHeader), 1);
    whole(PK_DEV, ctx->grid.cells, ncell + 1, 4);
    whole(PK_DEV, ctx->grid.patch, h.n_patches, 8);
    if (h.has_height) whole(PK_DEV, ctx->grid.height, h.n_patches, 4);
    if (ctx->has_hash) {
        for (int f = 0; f < 4; ++f) whole(PK_DEV, hash_field(ctx, f), h.hash_n, 8);
        whole(PK_HOST, ctx->hash_bucket.data(), h.hash_n * 4, 1);
        whole(PK_HOST, pl.bsizes.data(), pl.bsizes.size() * 4, 1);
    }
    const double* f7[7] = {s.x, s.y, s.th, s.z, s.zs, s.w, s.mprob};
    for (int f = 0; f < 7; ++f) add(PK_DEV, f7[f], n, 8, gb, nl);
    add(PK_DEV, s.flags, n, 1, gb, nl);
    whole(PK_HOST, &pl.sc, sizeof(SnapScalars), 1);
    if (h.sections & (1u << kSecMaps)) {
        add(PK_SID, nullptr, n, 4, gb, nl);
        add(PK_TABLES, nullptr, h.tables, (uint64_t)h.row_words * 4, pl.tbase, pl.T);
        add(PK_OWNER, nullptr, h.pages, 4, pl.pbase, pl.P);
        add(PK_PAGES, nullptr, h.pages, kPageBytes, pl.pbase, pl.P);
    }
    if (at != h.bytes || (!ctx->sharded && mine != h.bytes)) return fail(ctx, ESLAM_ERR_HIP, "snapshot: the pieces do not add up to the layout");
    return ESLAM_OK;
}

// chunks a piece splits into: whole units, at most chunk bytes (one unit when a unit is longer);
// the piece's padding rides on its last chunk
uint64_t snap_units_per_chunk(const Piece& q, uint64_t chunk)
{
    const uint64_t u = chunk / q.unit;       // chunk is a multiple of 16: the padded last chunk fits too
    return u ? u : 1;
}

uint64_t snap_chunk_count(const std::vector<Piece>& p, uint64_t chunk)
{
    uint64_t c = 0;
    for (const Piece& q : p) {
        if (!q.count) continue;
        const uint64_t per = snap_units_per_chunk(q, chunk);
        c += (q.count + per - 1) / per;
    }
    return c;
}

void snap_fill_info(const SnapHeader& h, uint64_t chunks, eslam_snapshot_info* info)
{
    if (!info) return;
    memset(info, 0, sizeof(*info));
    info->bytes = h.bytes;
    info->particles = h.n;
    info->tables = h.tables;
    info->pages = h.pages;
    info->grid_patches = h.n_patches;
    info->hash_poses = h.hash_n;
    info->chunks = chunks;
    info->version = h.version;
    info->sections = h.sections;
}

struct SnapChunk {
    size_t piece;
    uint64_t k0, cnt;
    bool last;                               // the piece's last chunk: its padding follows
};

int snap_write_pieces(eslam_ctx* ctx, SnapPlan& pl, const SnapSink& w, uint64_t chunk, uint64_t* chunks_out);

// positional: the sink takes every chunk with its offset (a sharded filter: this rank's chunks,
// and the call is a collective); else the chunks come in the blob's order
int snap_save(eslam_ctx* ctx, const SnapSink& w, bool positional, uint64_t chunk_bytes, eslam_snapshot_info* info, uint64_t capacity)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!ctx || !w) return ESLAM_ERR_INVALID_ARG;
    if (ctx->sharded && !positional) return fail(ctx, ESLAM_ERR_UNSUPPORTED, kSnapStreamSharded);
    if (chunk_bytes && chunk_bytes < 4096) return fail(ctx, ESLAM_ERR_INVALID_ARG, "snapshot: chunk_bytes is 0 or at least 4096");
    const uint64_t chunk = (chunk_bytes ? chunk_bytes : kSnapDefaultChunk) & ~(uint64_t)15;
    SnapPlan pl;
    int rc = snap_plan(ctx, pl);             // sharded: every rank has a plan, or every rank returns here
    if (rc) return rc;
    uint64_t chunks = 0;
    if (capacity < pl.h.bytes)
        rc = fail(ctx, ESLAM_ERR_INVALID_ARG, "snapshot: the buffer is smaller than the snapshot (eslam_gpu_snapshot_size)");
    else
        rc = snap_write_pieces(ctx, pl, w, chunk, &chunks);
    rc = agree(ctx, rc, "snapshot");
    if (rc) return rc;
    snap_fill_info(pl.h, chunks, info);
    return ESLAM_OK;
}

int snap_write_pieces(eslam_ctx* ctx, SnapPlan& pl, const SnapSink& w, uint64_t chunk, uint64_t* chunks_out)
{
    int rc = ESLAM_OK;
    uint64_t largest = 0, unit = 16;
    for (const Piece& q : pl.pieces) {
        largest = std::max(largest, pad16(q.count * q.unit + q.tail));
        unit = std::max(unit, pad16(q.unit));
    }
    rc = snap_staging(ctx, snap_stage_bytes(chunk, largest, unit));
    if (rc) return rc;
    const std::vector<Piece>& P = pl.pieces;
    // the next chunk after (piece, k0 + cnt); piece == P.size(): none
    auto next = [&](const SnapChunk& c) {
        SnapChunk d = c;
        d.k0 = c.k0 + c.cnt;
        while (d.piece < P.size() && d.k0 >= P[d.piece].count) {
            ++d.piece;
            d.k0 = 0;
        }
        if (d.piece < P.size()) {
            const uint64_t per = snap_units_per_chunk(P[d.piece], chunk), left = P[d.piece].count - d.k0;
            d.cnt = left < per ? left : per;
            d.last = d.cnt == left;
        }
        return d;
    };
    // chunk c into its slot: packed or copied on the stream into the pinned buffer, the slot's event after it
    auto issue = [&](const SnapChunk& c, uint32_t slot) -> int {
        const Piece& q = P[c.piece];
        const uint64_t bytes = c.cnt * q.unit, off = c.k0 * q.unit;
        char* host = ctx->snap_host[slot].as<char>();
        if (q.kind == PK_HOST) {
            memcpy(host, (const char*)q.src + off, bytes);
        } else if (q.kind == PK_DEV) {
            HIPCHK(ctx, hipMemcpyAsync(host, (const char*)q.src + off, bytes, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            HIPCHK(ctx, eslam_launch_snap_pack(q.kind - PK_SID, &ctx->lm, &pl.cen, pl.sid, pl.T, pl.tbase, pl.pbase, c.k0, c.cnt,
                                               pl.h.row_words, ctx->snap_dev[slot], ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(host, ctx->snap_dev[slot], bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(ctx, hipEventRecord(ctx->snap_ev[slot], ctx->stream));
        return ESLAM_OK;
    };
    SnapChunk cur = next(SnapChunk{0, 0, 0, false});
    uint32_t slot = 0;
    uint64_t chunks = 0;
    if (cur.piece < P.size()) rc = issue(cur, slot);
    while (!rc && cur.piece < P.size()) {
        // the device packs chunk c + 1 while the host writes chunk c
        const SnapChunk nxt = next(cur);
        if (nxt.piece < P.size()) rc = issue(nxt, slot ^ 1u);
        if (rc) break;
        HIPCHK(ctx, hipEventSynchronize(ctx->snap_ev[slot]));
        const Piece& q = P[cur.piece];
        uint64_t bytes = cur.cnt * q.unit;
        if (cur.last && q.tail) {            // zeros up to the array's next 16-byte boundary
            memset(ctx->snap_host[slot].as<char>() + bytes, 0, q.tail);
            bytes += q.tail;
        }
        if (w(q.off + cur.k0 * q.unit, ctx->snap_host[slot], bytes) != 0) {
            rc = fail(ctx, ESLAM_ERR_COMM, "snapshot: the write callback failed");
            break;
        }
        ++chunks;
        cur = nxt;
        slot ^= 1u;
    }
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);    // a copy into the pinned buffers may be in flight
        return rc;
    }
    *chunks_out = chunks;
    return ESLAM_OK;
}

// ---- load -------------------------------------------------------------------------------
struct SnapReader {
    eslam_ctx* ctx;
    SnapSource r;
    uint64_t chunk;
    uint32_t slot = 0;
    uint64_t chunks = 0;
    uint64_t at = 0;                         // the blob offset of the next array
    uint64_t dst0 = 0;                       // PK_TABLES / PK_OWNER: the pool entry of unit `first`
    const SnapSubset* sub = nullptr;         // PK_OWNER: owners renamed through the subset
};
typedef std::function<int(const void* data, uint64_t k0, uint64_t cnt)> SnapCheck;

int snap_bad(eslam_ctx* ctx, const char* msg) { return fail(ctx, ESLAM_ERR_INVALID_ARG, msg); }

// one array of the blob through the staging buffers: every chunk is read into a pinned slot,
// checked on the host (check; may be empty), and then copied to dst (PK_HOST: host memory,
// may be null; PK_DEV: device memory) or unpacked into pool entries [k0, k0 + cnt)
int snap_read_part(SnapReader& rd, int kind, void* dst, uint64_t count, uint64_t unit, uint32_t rw, const SnapCheck& check,
                   uint64_t off, uint64_t tail);

// the whole array at the cursor
int snap_read(SnapReader& rd, int kind, void* dst, uint64_t count, uint64_t unit, uint32_t rw, const SnapCheck& check)
{
    const uint64_t all = count * unit, off = rd.at;
    rd.at += pad16(all);
    rd.dst0 = 0;
    return snap_read_part(rd, kind, dst, count, unit, rw, check, off, pad16(all) - all);
}

// units [first, first + count) of the array of `total` units at the cursor, which then moves past the array
int snap_read_slice(SnapReader& rd, int kind, void* dst, uint64_t total, uint64_t first, uint64_t count, uint64_t unit,
                    const SnapCheck& check)
{
    const uint64_t off = rd.at + first * unit;
    rd.at += pad16(total * unit);
    rd.dst0 = 0;
    return snap_read_part(rd, kind, dst, count, unit, 0, check, off, 0);
}

int snap_read_part(SnapReader& rd, int kind, void* dst, uint64_t count, uint64_t unit, uint32_t rw, const SnapCheck& check,
                   uint64_t off, uint64_t tail)
{
    eslam_ctx* ctx = rd.ctx;
    uint64_t per = rd.chunk / unit;
    per = per ? per : 1;
    for (uint64_t k0 = 0; k0 < count; k0 += per) {
        const uint64_t cnt = count - k0 < per ? count - k0 : per, bytes = cnt * unit;
        const bool last = k0 + cnt == count;
        const uint32_t slot = rd.slot;
        rd.slot ^= 1u;
        HIPCHK(ctx, hipEventSynchronize(ctx->snap_ev[slot]));     // the slot's previous chunk has left it
        char* host = ctx->snap_host[slot].as<char>();
        if (rd.r(off + k0 * unit, host, bytes + (last ? tail : 0)) != 0) return fail(ctx, ESLAM_ERR_COMM, "snapshot: the read callback failed");
        ++rd.chunks;
        if (check) {
            const int rc = check(host, k0, cnt);
            if (rc) return rc;
        }
        if (kind == PK_HOST) {
            if (dst) memcpy((char*)dst + k0 * unit, host, bytes);
            continue;
        }
        if (kind == PK_DEV) {
            HIPCHK(ctx, hipMemcpyAsync((char*)dst + k0 * unit, host, bytes, hipMemcpyHostToDevice, ctx->stream));
        } else {
            HIPCHK(ctx, hipMemcpyAsync(ctx->snap_dev[slot], host, bytes, hipMemcpyHostToDevice, ctx->stream));
            if (kind == PK_OWNER && rd.sub)
                HIPCHK(ctx, eslam_launch_snap_unpack_owner_subset(&ctx->lm, rd.dst0 + k0, cnt, rd.sub, ctx->snap_dev[slot], ctx->stream));
            else
                HIPCHK(ctx, eslam_launch_snap_unpack(kind - PK_SID, &ctx->lm, rd.dst0 + k0, cnt, rw, ctx->snap_dev[slot], ctx->stream));
        }
        HIPCHK(ctx, hipEventRecord(ctx->snap_ev[slot], ctx->stream));
    }
    return ESLAM_OK;
}

int snap_check_header(eslam_ctx* ctx, const SnapHeader& h, uint64_t known_bytes)
{
    if (memcmp(h.magic, kSnapMagic, 8) != 0) return snap_bad(ctx, "snapshot: bad magic");
    if (h.version != ESLAM_SNAPSHOT_VERSION) return snap_bad(ctx, "snapshot: unknown version");
    const uint32_t need = (1u << kSecGrid) | (1u << kSecParticles) | (1u << kSecScalars);
    if ((h.sections & need) != need || (h.sections >> kSecCount)) return snap_bad(ctx, "snapshot: section mask");
    if (h.particle_maps > 1u || (h.particle_maps != 0u) != particle_maps(ctx))
        return snap_bad(ctx, "snapshot: ESLAM_FLAG_PARTICLE_MAPS differs from the context's");
    if (h.local_map_trail != ctx->cfg.local_map_trail) return snap_bad(ctx, "snapshot: local_map_trail differs from the context's");
    if (h.n >= (1ull << 32) - 1 || h.tables > h.n || h.pages >= 0xffffffffull) return snap_bad(ctx, "snapshot: counts out of range");
    if (!h.width || !h.height || (uint64_t)h.width * h.height >= 0xffffffffull || h.n_patches > 0xffffffffull || h.has_height > 1u)
        return snap_bad(ctx, "snapshot: grid size");
    if (!(h.scale_x > 0.0) || !(h.scale_y > 0.0) || !dm_isfinite(h.scale_x) || !dm_isfinite(h.scale_y))
        return snap_bad(ctx, "snapshot: grid scale");
    const bool hash = (h.sections >> kSecHash) & 1u, maps = (h.sections >> kSecMaps) & 1u;
    if (hash ? (h.hash_bins == 0 || h.hash_bins > 4096 || h.hash_bins != (uint32_t)ctx->cfg.hash_slope_bins || h.hash_n >= (1ull << 32))
             : (h.hash_bins != 0 || h.hash_n != 0))
        return snap_bad(ctx, "snapshot: pose hash size (hash_slope_bins differs from the context's?)");
    if (h.particle_maps) {
        const double r = ctx->cfg.max_sensor_range;
        if (!(r == r) || r < 0.0 || r > 1e6) return snap_bad(ctx, "max_sensor_range must be finite and >= 0");
        if (h.hx != dm_lm_half(r, h.scale_x) || h.hy != dm_lm_half(r, h.scale_y))
            return snap_bad(ctx, "snapshot: max_sensor_range (the window's half-widths) differs from the context's");
        if (h.local_map_trail > 4096) return snap_bad(ctx, "local_map_trail: at most 4096 tiles");
    } else if (h.hx || h.hy) {
        return snap_bad(ctx, "snapshot: window without per-particle maps");
    }
    if (maps != (h.particle_maps && h.n > 0)) return snap_bad(ctx, "snapshot: per-particle map section");
    if (maps) {
        if (h.wx != 2 * h.hx + 1 || h.wy != 2 * h.hy + 1 || h.row_words != snap_row_words(h.wx * h.wy, h.local_map_trail))
            return snap_bad(ctx, "snapshot: table row size");
    } else if (h.tables || h.pages || h.wx || h.wy || h.row_words) {
        return snap_bad(ctx, "snapshot: tables without a map section");
    }
    SnapSection sec[kSecCount];
    uint64_t bytes = 0;
    snap_layout(h, sec, &bytes);
    for (int k = 0; k < kSecCount; ++k)
        if (sec[k].off != h.sec[k].off || sec[k].size != h.sec[k].size)
            return snap_bad(ctx, "snapshot: a section's offset or size does not match the header's counts");
    if (bytes != h.bytes || (known_bytes && known_bytes != h.bytes)) return snap_bad(ctx, "snapshot: size does not match the header (truncated?)");
    if (ctx->sharded && h.n != ctx->n_global)
        return snap_bad(ctx, "snapshot: its particle count is not the sharded context's n_global");
    if (maps && !ctx->sharded) {             // a sharded load checks its own part's pages, once it has counted them
        const uint64_t per = ctx->cfg.local_map_pages ? ctx->cfg.local_map_pages : kDefaultMapPages;
        if (h.pages > (h.n ? h.n : 1) * per)
            return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "snapshot: more live pages than the context's pool holds (raise eslam_config.local_map_pages)");
    }
    return ESLAM_OK;
}

// the host's check of a chunk of table rows: every id before a kernel reads it
SnapCheck snap_rows_check(eslam_ctx* ctx, uint32_t rw, uint32_t W, uint32_t V, uint64_t P)
{
    return [=](const void* d, uint64_t, uint64_t cnt) {
        const uint32_t* v = (const uint32_t*)d;
        for (uint64_t k = 0; k < cnt; ++k) {
            const uint32_t* r = v + k * rw;
            if (r[2] > 1u || r[3] > V) return snap_bad(ctx, "snapshot: a table's shadow flag or trail mark is out of range");
            for (uint32_t s = 0; s < W; ++s)
                if (r[4 + s] != DM_LM_NONE && r[4 + s] >= P)
                    return snap_bad(ctx, "snapshot: a window slot names a page past the snapshot's pages");
            for (uint32_t e = 0; e < V; ++e) {
                const uint32_t pg = r[4 + W + 3 * e + 2];
                if (pg != DM_LM_NONE && pg >= P) return snap_bad(ctx, "snapshot: a trail entry names a page past the snapshot's pages");
            }
        }
        return (int)ESLAM_OK;
    };
}

// the header, read and checked: no collective yet, and every rank of a sharded filter decides alike
int snap_load_header(eslam_ctx* ctx, SnapReader& rd, SnapHeader& h, uint64_t known_bytes)
{
    if (known_bytes && known_bytes < sizeof(SnapHeader)) return snap_bad(ctx, "snapshot: shorter than its header");
    if (rd.r(0, &h, sizeof(h)) != 0) return fail(ctx, ESLAM_ERR_COMM, "snapshot: the read callback failed");
    ++rd.chunks;
    rd.at = sizeof(h);
    return snap_check_header(ctx, h, known_bytes);
}

int snap_load_maps_subset(eslam_ctx* ctx, SnapReader& rd, const SnapHeader& h, uint64_t* pages_loaded);

// everything behind the header.  A sharded filter reads the shared parts in full, its shard
// [gbase, gbase + nl) of the particle arrays, and of the maps what its particles name.
int snap_load_body(eslam_ctx* ctx, SnapReader& rd, SnapHeader& h)
{
    int rc = ESLAM_OK;
    const uint64_t ncell = (uint64_t)h.width * h.height, np = h.n_patches, n = h.n;
    const uint64_t gb = ctx->sharded ? ctx->gbase : 0, nl = ctx->sharded ? ctx->gall[ctx->comm.rank + 1] - ctx->gbase : n;
    const bool hash = (h.sections >> kSecHash) & 1u, maps = (h.sections >> kSecMaps) & 1u;
    uint64_t largest = std::max(std::max((ncell + 1) * 4, np * 8), std::max(n * 8, h.hash_n * 8));
    largest = std::max(largest, std::max(h.tables * h.row_words * 4, h.pages * kPageBytes));
    rc = snap_staging(ctx, snap_stage_bytes(rd.chunk, pad16(largest), pad16(std::max<uint64_t>(kPageBytes, (uint64_t)h.row_words * 4))));
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    free_particles(ctx);                     // whatever the context held goes first
    const SnapCheck none;
    // ---- the shared grid: through eslam_gpu_set_map (occ and cell_tab rebuilt as there)
    {
        std::vector<uint32_t> cells(ncell + 1);
        std::vector<float2> patch(np);
        std::vector<float> mean(np ? np : 1), stdev(np ? np : 1), height;
        uint32_t prev = 0;
        rc = snap_read(rd, PK_HOST, cells.data(), ncell + 1, 4, 0, [&](const void* d, uint64_t k0, uint64_t cnt) {
            const uint32_t* c = (const uint32_t*)d;
            for (uint64_t k = 0; k < cnt; ++k) {
                if (c[k] < prev || c[k] > np || (k0 + k == 0 && c[k] != 0)) return snap_bad(ctx, "snapshot: the grid's cell_start is not a prefix sum");
                prev = c[k];
            }
            return (int)ESLAM_OK;
        });
        if (!rc && prev != np) rc = snap_bad(ctx, "snapshot: cell_start[width*height] != n_patches");
        if (!rc) rc = snap_read(rd, PK_HOST, patch.data(), np, 8, 0, none);
        if (!rc && h.has_height) {
            height.resize(np ? np : 1);
            rc = snap_read(rd, PK_HOST, height.data(), np, 4, 0, none);
        }
        if (rc) return rc;
        for (uint64_t k = 0; k < np; ++k) {
            mean[k] = patch[k].x;
            stdev[k] = patch[k].y;
        }
        eslam_mls_grid g;
        memset(&g, 0, sizeof(g));
        g.width = h.width;
        g.height = h.height;
        g.scale_x = h.scale_x;
        g.scale_y = h.scale_y;
        g.offset_x = h.offset_x;
        g.offset_y = h.offset_y;
        memcpy(g.global2local, h.g2l, sizeof(h.g2l));
        g.cell_start = cells.data();
        g.n_patches = np;
        g.patch_mean = mean.data();
        g.patch_stdev = stdev.data();
        g.patch_height = h.has_height ? height.data() : nullptr;
        rc = eslam_gpu_set_map(ctx, &g);
        if (rc) return rc;
    }
    // ---- the pose hash: restored, not recomputed
    if (hash) {
        const uint64_t hn = h.hash_n, cap = hn ? hn : 1;
        const uint32_t nb = h.hash_bins * h.hash_bins;
        ctx->d_hash.reset();
        ctx->d_hash_blist.reset();
        ctx->hash_n = 0;
        if (ctx->d_hash.alloc(sizeof(double) * 4 * cap) != hipSuccess || ctx->d_hash_blist.alloc(sizeof(uint32_t) * cap) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "hash pose buffers");
        }
        for (int f = 0; f < 4 && !rc; ++f) rc = snap_read(rd, PK_DEV, ctx->d_hash + (uint64_t)f * cap, hn, 8, 0, none);
        std::vector<int32_t> bucket(hn);
        std::vector<uint32_t> sizes(nb), bstart(nb + 1, 0u);
        if (!rc) rc = snap_read(rd, PK_HOST, bucket.data(), hn, 4, 0, [&](const void* d, uint64_t, uint64_t cnt) {
            const int32_t* b = (const int32_t*)d;
            for (uint64_t k = 0; k < cnt; ++k)
                if (b[k] < 0 || (uint32_t)b[k] >= nb) return snap_bad(ctx, "snapshot: a hash pose's bucket is out of range");
            return (int)ESLAM_OK;
        });
        if (!rc) rc = snap_read(rd, PK_HOST, sizes.data(), nb, 4, 0, none);
        if (rc) return rc;
        for (uint64_t i = 0; i < hn; ++i) bstart[bucket[i] + 1]++;
        for (uint32_t b = 0; b < nb; ++b) {
            if (bstart[b + 1] != sizes[b]) return snap_bad(ctx, "snapshot: the hash's bucket sizes do not match its buckets");
            bstart[b + 1] += bstart[b];
        }
        std::vector<uint32_t> blist(cap), fill(bstart.begin(), bstart.end() - 1);
        for (uint64_t i = 0; i < hn; ++i) blist[fill[bucket[i]]++] = (uint32_t)i;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (hn) HIPCHK(ctx, hipMemcpy(ctx->d_hash_blist, blist.data(), sizeof(uint32_t) * hn, hipMemcpyHostToDevice));
        ctx->hash_bucket.swap(bucket);
        ctx->hash_bstart.swap(bstart);
        ctx->hash_n = hn;
        ctx->has_hash = true;
    }
    // ---- the particles (the eight arrays of the current buffer, into buffer 0)
    rc = alloc_particles(ctx, nl);
    if (rc) return rc;
    if (maps && !ctx->lm_ready) return fail(ctx, ESLAM_ERR_HIP, "snapshot: per-particle maps not allocated");
    {
        const DevState& s = ctx->st[0];
        double* f7[7] = {s.x, s.y, s.th, s.z, s.zs, s.w, s.mprob};
        if (ctx->sharded) {
            for (int f = 0; f < 7 && !rc; ++f) rc = snap_read_slice(rd, PK_DEV, f7[f], n, gb, nl, 8, none);
            if (!rc) rc = snap_read_slice(rd, PK_DEV, s.flags, n, gb, nl, 1, none);
        } else {
            for (int f = 0; f < 7 && !rc; ++f) rc = snap_read(rd, PK_DEV, f7[f], n, 8, 0, none);
            if (!rc) rc = snap_read(rd, PK_DEV, s.flags, n, 1, 0, none);
        }
        if (rc) return rc;
    }
    // ---- the scalars
    SnapScalars sc;
    rc = snap_read(rd, PK_HOST, &sc, sizeof(sc), 1, 0, none);
    if (!rc) rc = reset_ctl_for_new_particles(ctx, sc.wexp);
    if (rc) return rc;
    {
        Ctl& ctl = *ctx->ctl_host;           // as reset_ctl_for_new_particles read it
        ctl.minstd = sc.minstd;
        ctl.max_weight = sc.max_weight;
        ctl.update_count = sc.update_count;
        ctl.inv_n = sc.inv_n;
        if (maps) {
            ctl.pg_cursor = 0;
            ctl.pg_nfree = ctx->lm.npages - h.pages;
            ctl.pg_total = 0;
            ctl.pg_gc = 0;
        }
        ctx->proj_event = sc.rng.project_count;
        ctx->init_event = sc.rng.init_count;
        *ctx->hash_ev = sc.rng.hash_count;
        memcpy(ctx->ud_pose, sc.rng.ud_pose, sizeof(ctx->ud_pose));
        memcpy(ctx->libcp->r, sc.rng.libc_rand, sizeof(sc.rng.libc_rand));
        ctx->libcp->i = sc.rng.libc_rand_pos % 34u;
        rc = write_ctl(ctx);
        if (rc) return rc;
        ctx->dbg_valid = false;
    }
    // ---- the per-particle maps of a sharded filter: this rank's subset, then the page counters
    if (maps && ctx->sharded) {
        uint64_t ploc = 0;
        rc = snap_load_maps_subset(ctx, rd, h, &ploc);
        if (!rc) rc = read_ctl(ctx);
        if (rc) return rc;
        ctx->ctl_host->pg_nfree = ctx->lm.npages - ploc;
        rc = write_ctl(ctx);
        if (rc) return rc;
    }
    // ---- the per-particle maps: table k into pool entry k, page k into pool entry k
    if (maps && !ctx->sharded) {
        const uint64_t T = h.tables, P = h.pages;
        const uint32_t rw = h.row_words, W = h.wx * h.wy, V = h.local_map_trail;
        rc = snap_read(rd, PK_DEV, ctx->st[0].sid, n, 4, 0, [&](const void* d, uint64_t, uint64_t cnt) {
            const uint32_t* v = (const uint32_t*)d;
            for (uint64_t k = 0; k < cnt; ++k)
                if (v[k] >= T) return snap_bad(ctx, "snapshot: a particle names a table past the snapshot's tables");
            return (int)ESLAM_OK;
        });
        if (!rc) rc = snap_read(rd, PK_TABLES, nullptr, T, (uint64_t)rw * 4, rw, snap_rows_check(ctx, rw, W, V, P));
        if (!rc) rc = snap_read(rd, PK_OWNER, nullptr, P, 4, 0, [&](const void* d, uint64_t, uint64_t cnt) {
            const uint32_t* v = (const uint32_t*)d;
            for (uint64_t k = 0; k < cnt; ++k)
                if (v[k] != DM_LM_NONE && v[k] >= T) return snap_bad(ctx, "snapshot: a page's owner is past the snapshot's tables");
            return (int)ESLAM_OK;
        });
        if (!rc) rc = snap_read(rd, PK_DEV, ctx->lm.page, P, kPageBytes, 0, none);
        if (rc) return rc;
        HIPCHK(ctx, eslam_launch_snap_finish(&ctx->lm, T, P, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ESLAM_OK;
}

// f(a, b, local) for every run [a, b) of set bits below `limit`, ascending; local: the set bits below a
template <typename F>
int snap_for_runs(const std::vector<uint32_t>& bits, uint64_t limit, F f)
{
    uint64_t i = 0, local = 0;
    auto bit = [&](uint64_t k) { return (bits[k >> 5] >> (k & 31)) & 1u; };
    while (i < limit) {
        if (!(i & 31) && bits[i >> 5] == 0u) {
            i += 32;
            continue;
        }
        if (!bit(i)) {
            ++i;
            continue;
        }
        uint64_t b = i + 1;
        while (b < limit) {
            if (!(b & 31) && bits[b >> 5] == 0xffffffffu) b += 32;
            else if (bit(b)) ++b;
            else break;
        }
        if (b > limit) b = limit;
        if (const int rc = f(i, b, local)) return rc;
        local += b - i;
        i = b;
    }
    return ESLAM_OK;
}

// The per-particle maps of a sharded load ("Sharded filters"): the tables this
// rank's particles name, in the snapshot's order, into pool tables 0, 1, ...; the pages those
// tables name into pool pages 0, 1, ...  Two bitmaps over the snapshot's ids, ranked by
// popcount on the device; the host walks their runs of set bits and reads each run's rows,
// owner words and pages.  With every bit set this is the one-GPU load: entry k into pool entry k.
int snap_load_maps_subset(eslam_ctx* ctx, SnapReader& rd, const SnapHeader& h, uint64_t* pages_loaded)
{
    const uint64_t T = h.tables, P = h.pages, n = h.n, gb = ctx->gbase, nl = ctx->n;
    const uint32_t rw = h.row_words, W = h.wx * h.wy, V = h.local_map_trail;
    const uint64_t tw = (T + 31) / 32, pw = (P + 31) / 32;
    const uint64_t off_sid = rd.at, off_tab = off_sid + pad16(n * 4), off_own = off_tab + pad16(T * rw * 4), off_pg = off_own + pad16(P * 4);
    const SnapCheck none;
    Dev<uint32_t> scratch;                   // dropped with the call
    const uint64_t words = tw + (tw + 1) + pw + (pw + 1);
    if (scratch.alloc(words * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "snapshot: no device memory for the subset's bitmaps");
    }
    HIPCHK(ctx, hipMemsetAsync(scratch, 0, words * 4, ctx->stream));
    SnapSubset sub;
    sub.tbits = scratch;
    sub.tpre = sub.tbits + tw;
    sub.pbits = sub.tpre + tw + 1;
    sub.ppre = sub.pbits + pw;
    sub.tables = T;
    sub.pages = P;
    // the scratch goes only once the stream is idle, whichever way the call ends
    struct Idle {
        hipStream_t s;
        ~Idle() { (void)hipStreamSynchronize(s); }
    } idle{ctx->stream};
    // ---- tables: the bits of this shard's names, their ranks, the names rewritten
    uint32_t* sid = ctx->st[0].sid;
    int rc = snap_read_slice(rd, PK_DEV, sid, n, gb, nl, 4, [&](const void* d, uint64_t, uint64_t cnt) {
        const uint32_t* v = (const uint32_t*)d;
        for (uint64_t k = 0; k < cnt; ++k)
            if (v[k] >= T) return snap_bad(ctx, "snapshot: a particle names a table past the snapshot's tables");
        return (int)ESLAM_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, eslam_launch_snap_mark_ids(sid, nl, sub.tbits, T, ctx->stream));
    HIPCHK(ctx, eslam_launch_snap_rank_bits(sub.tbits, tw, sub.tpre, ctx->stream));
    HIPCHK(ctx, eslam_launch_snap_rank_sid(sid, nl, &sub, ctx->stream));
    std::vector<uint32_t> tbits(tw + 1), pbits(pw + 1);
    uint32_t tloc = 0, ploc = 0;
    HIPCHK(ctx, hipMemcpyAsync(tbits.data(), sub.tbits, tw * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&tloc, sub.tpre + tw, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (tloc > ctx->lm.ntables || tloc > nl) return fail(ctx, ESLAM_ERR_HIP, "snapshot: more tables named than particles");
    // ---- rows: each run of named tables into pool tables local(run start)..., page ids still the snapshot's
    const SnapCheck rows = snap_rows_check(ctx, rw, W, V, P);
    rc = snap_for_runs(tbits, T, [&](uint64_t a, uint64_t b, uint64_t local) {
        rd.dst0 = local;
        return snap_read_part(rd, PK_TABLES, nullptr, b - a, (uint64_t)rw * 4, rw, rows, off_tab + a * rw * 4, 0);
    });
    if (rc) return rc;
    // ---- pages: the bits of what those rows name, their ranks; this rank's pool must hold them
    HIPCHK(ctx, eslam_launch_snap_mark_rows(&ctx->lm, tloc, sub.pbits, P, ctx->stream));
    HIPCHK(ctx, eslam_launch_snap_rank_bits(sub.pbits, pw, sub.ppre, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(pbits.data(), sub.pbits, pw * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&ploc, sub.ppre + pw, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ploc > ctx->lm.npages)
        return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY,
                    "snapshot: more live pages than this rank's pool holds (raise eslam_config.local_map_pages)");
    HIPCHK(ctx, eslam_launch_snap_renumber_tables(&ctx->lm, tloc, &sub, ctx->stream));
    rd.sub = &sub;
    rc = snap_for_runs(pbits, P, [&](uint64_t a, uint64_t b, uint64_t local) {
        rd.dst0 = local;
        return snap_read_part(rd, PK_OWNER, nullptr, b - a, 4, 0, [&](const void* d, uint64_t, uint64_t cnt) {
            const uint32_t* v = (const uint32_t*)d;
            for (uint64_t k = 0; k < cnt; ++k)
                if (v[k] != DM_LM_NONE && v[k] >= T) return snap_bad(ctx, "snapshot: a page's owner is past the snapshot's tables");
            return (int)ESLAM_OK;
        }, off_own + a * 4, 0);
    });
    rd.sub = nullptr;
    rd.dst0 = 0;
    if (rc) return rc;
    // consecutive set bits are consecutive local ids: a run of pages is one plain copy
    rc = snap_for_runs(pbits, P, [&](uint64_t a, uint64_t b, uint64_t local) {
        return snap_read_part(rd, PK_DEV, (char*)ctx->lm.page + local * kPageBytes, b - a, kPageBytes, 0, none, off_pg + a * kPageBytes, 0);
    });
    if (rc) return rc;
    HIPCHK(ctx, eslam_launch_snap_finish(&ctx->lm, tloc, ploc, ctx->stream));
    rd.at = off_pg + P * kPageBytes;
    *pages_loaded = ploc;
    return ESLAM_OK;
}

// positional: the source is read by offset (a sharded filter: a collective, and each rank reads
// its part only); else in the blob's order, every byte once
int snap_load(eslam_ctx* ctx, const SnapSource& r, bool positional, uint64_t chunk_bytes, eslam_snapshot_info* info, uint64_t known_bytes)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!ctx || !r) return ESLAM_ERR_INVALID_ARG;
    if (ctx->sharded && !positional) return fail(ctx, ESLAM_ERR_UNSUPPORTED, kSnapStreamSharded);
    if (chunk_bytes && chunk_bytes < 4096) return fail(ctx, ESLAM_ERR_INVALID_ARG, "snapshot: chunk_bytes is 0 or at least 4096");
    SnapReader rd;
    rd.ctx = ctx;
    rd.r = r;
    rd.chunk = (chunk_bytes ? chunk_bytes : kSnapDefaultChunk) & ~(uint64_t)15;
    SnapHeader h;
    memset(&h, 0, sizeof(h));
    int rc = ESLAM_OK;
    if (ctx->sharded) {
        // the header decides alike on every rank, before the first collective
        rc = snap_load_header(ctx, rd, h, known_bytes);
        if (rc) {
            const std::string msg = ctx->err;
            (void)hipStreamSynchronize(ctx->stream);
            free_particles(ctx);
            ctx->err = msg;
            return rc;
        }
        rc = settle(ctx);
    } else {
        rc = settle(ctx);
        if (rc) return rc;
        rc = snap_load_header(ctx, rd, h, known_bytes);
    }
    if (!rc) rc = snap_load_body(ctx, rd, h);
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    rc = agree(ctx, rc, "snapshot");                // sharded: no rank goes on with a filter another rank could not load
    if (rc) {
        // the context reads as "no particles"; set_map + init_* or another load starts it over
        const std::string msg = ctx->err;
        (void)hipStreamSynchronize(ctx->stream);
        free_particles(ctx);
        ctx->err = msg;
        return rc;
    }
    snap_fill_info(h, rd.chunks, info);
    return ESLAM_OK;
}

struct SnapMem {
    char* p;
    uint64_t left;
};
int snap_mem_write(void* user, const void* data, uint64_t bytes)
{
    SnapMem* m = (SnapMem*)user;
    if (bytes > m->left) return 1;
    memcpy(m->p, data, bytes);
    m->p += bytes;
    m->left -= bytes;
    return 0;
}
int snap_mem_read(void* user, void* data, uint64_t bytes)
{
    SnapMem* m = (SnapMem*)user;
    if (bytes > m->left) return 1;
    memcpy(data, m->p, bytes);
    m->p += bytes;
    m->left -= bytes;
    return 0;
}

SnapSink snap_stream_sink(eslam_write_fn w, void* user)
{
    if (!w) return SnapSink();
    return [w, user](uint64_t, const void* data, uint64_t bytes) { return w(user, data, bytes); };
}
SnapSource snap_stream_source(eslam_read_fn r, void* user)
{
    if (!r) return SnapSource();
    return [r, user](uint64_t, void* data, uint64_t bytes) { return r(user, data, bytes); };
}

}  // namespace

// a collective on a sharded filter
extern "C" int eslam_gpu_snapshot_size(eslam_ctx* ctx, eslam_snapshot_info* info)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!ctx || !info) return ESLAM_ERR_INVALID_ARG;
    SnapPlan pl;
    const int rc = snap_plan(ctx, pl);
    if (rc) return rc;
    snap_fill_info(pl.h, snap_chunk_count(pl.pieces, kSnapDefaultChunk), info);
    return ESLAM_OK;
}

extern "C" int eslam_gpu_save_stream(eslam_ctx* ctx, eslam_write_fn w, void* user, uint64_t chunk_bytes, eslam_snapshot_info* info)
{
    return snap_save(ctx, snap_stream_sink(w, user), false, chunk_bytes, info, ~0ull);
}

extern "C" int eslam_gpu_load_stream(eslam_ctx* ctx, eslam_read_fn r, void* user, uint64_t chunk_bytes, eslam_snapshot_info* info)
{
    return snap_load(ctx, snap_stream_source(r, user), false, chunk_bytes, info, 0);
}

extern "C" int eslam_gpu_save_at(eslam_ctx* ctx, eslam_pwrite_fn w, void* user, uint64_t chunk_bytes, eslam_snapshot_info* info)
{
    SnapSink sink;
    if (w) sink = [w, user](uint64_t off, const void* data, uint64_t bytes) { return w(user, off, data, bytes); };
    return snap_save(ctx, sink, true, chunk_bytes, info, ~0ull);
}

extern "C" int eslam_gpu_load_at(eslam_ctx* ctx, eslam_pread_fn r, void* user, uint64_t known_bytes, uint64_t chunk_bytes,
                                 eslam_snapshot_info* info)
{
    SnapSource src;
    if (r) src = [r, user](uint64_t off, void* data, uint64_t bytes) { return r(user, off, data, bytes); };
    return snap_load(ctx, src, true, chunk_bytes, info, known_bytes);
}

extern "C" int eslam_gpu_save(eslam_ctx* ctx, void* buf, uint64_t capacity, uint64_t chunk_bytes, eslam_snapshot_info* info)
{
    if (!buf) return ESLAM_ERR_INVALID_ARG;
    SnapMem m{(char*)buf, capacity};
    return snap_save(ctx, snap_stream_sink(snap_mem_write, &m), false, chunk_bytes, info, capacity);
}

// on a sharded filter every rank holds the whole blob and reads its part of it
extern "C" int eslam_gpu_load(eslam_ctx* ctx, const void* buf, uint64_t bytes, uint64_t chunk_bytes, eslam_snapshot_info* info)
{
    if (!buf) return ESLAM_ERR_INVALID_ARG;
    if (ctx && ctx->sharded) {
        const char* p = (const char*)buf;
        const SnapSource src = [p, bytes](uint64_t off, void* data, uint64_t b) {
            if (off > bytes || b > bytes - off) return 1;
            memcpy(data, p + off, b);
            return 0;
        };
        return snap_load(ctx, src, true, chunk_bytes, info, bytes ? bytes : 1);
    }
    SnapMem m{(char*)const_cast<void*>(buf), bytes};
    return snap_load(ctx, snap_stream_source(snap_mem_read, &m), false, chunk_bytes, info, bytes ? bytes : 1);
}

