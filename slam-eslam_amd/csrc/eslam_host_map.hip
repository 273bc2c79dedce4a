// eslam_host_map.hip -- host side of libeslam_gpu: the maps.  The per-particle maps' update and
// match, the shared map's update (one GPU and sharded), map_size and get_map, a particle's map as
// a grid (export and adoption), and the scan build from laser scans and depth images.  No kernels.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "eslam_ctx.h"
#include "eslam_scratch.h"

// timing mode (EventRing): event k (0..4) of the current map update (start, gather, copy on write,
// plan, merge); event k (0: start, 1: end) of the current map match
static void mrec(eslam_ctx* ctx, int k) { ctx->mring.record(ctx->timing, k, ctx->stream); }
static void xrec(eslam_ctx* ctx, int k) { ctx->xring.record(ctx->timing, k, ctx->stream); }

// ---------------------------------------------------------------------------------------
// per-particle local maps
// ---------------------------------------------------------------------------------------
extern "C" int eslam_gpu_map_update(eslam_ctx* ctx, const eslam_scan_patch* patches, uint32_t count)
{
    if (!ctx || (!patches && count)) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (!particle_maps(ctx)) return fail(ctx, ESLAM_ERR_INVALID_ARG, "map_update needs per-particle maps (ESLAM_FLAG_PARTICLE_MAPS)");
    if (!ctx->has_map) return fail(ctx, ESLAM_ERR_NO_ENVIRONMENT, "No environment attached.");
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    if (!ctx->lm_ready) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "per-particle maps not allocated");
    for (uint32_t k = 0; k < count; ++k)
        if (!dm_isfinite(patches[k].position[0]) || !dm_isfinite(patches[k].position[1]) ||
            !dm_isfinite(patches[k].position[2]) || !dm_isfinite(patches[k].stdev))
            return fail(ctx, ESLAM_ERR_INVALID_ARG, "map_update: scan patches must be finite");
    mrec(ctx, 0);
    // one GPU: a pending resample gather runs inside the merge (MergeParams::fuse: the store
    // classes and the merge read the particles through the marks), so the update reads and
    // writes the particle state once.  Sharded: the gather may hand this rank particles whose
    // stores are still in received payloads, which get local stores first (materialize).
    const bool fuse = !ctx->sharded;
    const GatherView gv = gather_view(ctx);
    if (!fuse) {
        const int rc = materialize(ctx);
        if (rc) return rc;
    }
    mrec(ctx, 1);
    // the scan on the device: this update's slot is free once the update before last is done
    const uint32_t slot = ctx->scan_slot ^= 1u;
    if (!ctx->scan_ev[slot]) HIPCHK(ctx, ctx->scan_ev[slot].create(false));
    else HIPCHK(ctx, hipEventSynchronize(ctx->scan_ev[slot]));
    const uint64_t sbytes = (uint64_t)(count ? count : 1) * sizeof(ScanPatch);
    int rc = grow(ctx, ctx->scan_host[slot], sbytes);
    if (!rc) rc = grow(ctx, ctx->scan_dev[slot], sbytes);
    // a scan of more than kScanPartSmall patches merges in parts of kScanPartLarge
    const uint32_t part = count <= kScanPartSmall ? kScanPartSmall : kScanPartLarge;
    if (!rc && part == kScanPartLarge) rc = grow(ctx, ctx->lmb.codes, ctx->cap * 2 * kScanPartLarge);
    if (rc) return rc;
    ScanPatch* sh = ctx->scan_host[slot];
    for (uint32_t k = 0; k < count; ++k)
        sh[k] = ScanPatch{patches[k].position[0], patches[k].position[1], patches[k].position[2], patches[k].stdev};
    if (count) HIPCHK(ctx, hipMemcpyAsync(ctx->scan_dev[slot], sh, sbytes, hipMemcpyHostToDevice, ctx->stream));
    // the parts in order: every cell sees its patches in the scan's order; the parts' counters
    // add up (map_stores_changed counts a map once per part that changed it)
    for (uint32_t c0 = 0; c0 == 0 || c0 < count; c0 += part) {
        const uint32_t cm = count - c0 < part ? count - c0 : part;
        const SidRef sr{ctx->st[0].sid, ctx->st[1].sid, ctx->ctl};
        const CowScratch cs = cow_layout(ctx->pt.cow, ctx->cap);
        HIPCHK(ctx, eslam_launch_store_refs(sr, ctx->n, store_pool(ctx->cap), &cs, fuse ? &gv : nullptr, ctx->lm.tgen,
                                            ctx->stream));
        if (!c0) mrec(ctx, 2);
        MergeParams mp = merge_params(ctx, cs);
        mp.is_id = ctx->map.g2l_identity;
        mp.gv = gv;                           // (the first part runs a pending gather; the device knows)
        mp.gbase = ctx->gbase;
        mp.fuse = fuse ? 1u : 0u;
        mp.aux = (ctx->cfg.flags & ESLAM_FLAG_NO_AUX_GATHER) ? 0u : 1u;
        mp.acc = c0 ? 1u : 0u;
        mp.m = cm;
        mp.sp = ctx->scan_dev[slot] + c0;
        mp.codes = ctx->lmb.codes;
        HIPCHK(ctx, eslam_launch_map_plan(ctx->st[0], ctx->st[1], ctx->ctl, &ctx->map, &ctx->lm, &mp, ctx->lmb.pgc, ctx->stream));
        if (!c0) mrec(ctx, 3);
        HIPCHK(ctx, eslam_launch_map_merge(ctx->st[0], ctx->st[1], ctx->ctl, &ctx->map, &ctx->lm, &mp, ctx->stream));
        if (fuse) {
            HIPCHK(ctx, eslam_launch_commit(ctx->ctl, ctx->stream));     // the gather's buffer flip, if one ran
        }
    }
    HIPCHK(ctx, hipEventRecord(ctx->scan_ev[slot], ctx->stream));
    mrec(ctx, 4);
    return ESLAM_OK;
}

// processMap(scanMap, match = true, ...)  src/EmbodiedSlamFilter.cpp:214-221 (k_map_match)
extern "C" int eslam_gpu_map_match(eslam_ctx* ctx, const eslam_scan_patch* patches, uint32_t count)
{
    if (!ctx || (!patches && count)) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (!ctx->has_map) return fail(ctx, ESLAM_ERR_NO_ENVIRONMENT, "No environment attached.");
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    if (particle_maps(ctx) && !ctx->lm_ready) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "per-particle maps not allocated");
    for (uint32_t k = 0; k < count; ++k)
        if (!dm_isfinite(patches[k].position[0]) || !dm_isfinite(patches[k].position[1]) ||
            !dm_isfinite(patches[k].position[2]) || !dm_isfinite(patches[k].stdev))
            return fail(ctx, ESLAM_ERR_INVALID_ARG, "map_match: scan patches must be finite");
    xrec(ctx, 0);
    int rc = materialize(ctx);                // the weights of the particles as they stand
    if (rc) return rc;
    std::vector<ScanPatch> s;
    for (uint32_t k = 0; k < count; k += kMatchSampling)
        s.push_back(ScanPatch{patches[k].position[0], patches[k].position[1], patches[k].position[2], patches[k].stdev});
    MatchParams mp;
    mp.n = ctx->n;
    mp.m = (uint32_t)s.size();
    mp.is_id = ctx->map.g2l_identity;
    mp.sp = nullptr;
    const bool inline_sp = s.size() <= (size_t)kMaxScanPatches;   // the kernel arguments carry them
    if (inline_sp) {
        for (size_t k = 0; k < s.size(); ++k) mp.spi[k] = s[k];
    } else {
        rc = grow(ctx, ctx->lmb.match_sp, s.size() * sizeof(ScanPatch));
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->lmb.match_sp, s.data(), s.size() * sizeof(ScanPatch), hipMemcpyHostToDevice, ctx->stream));
        mp.sp = ctx->lmb.match_sp;
    }
    HIPCHK(ctx, eslam_launch_map_match(ctx->st[0], ctx->st[1], ctx->ctl, &ctx->map, store_of(ctx), &mp, ctx->stream));
    xrec(ctx, 1);
    // a scan of more than 640 patches: the host's copy of the sampled ones goes away on return
    if (!inline_sp) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ESLAM_OK;
}

extern "C" int eslam_gpu_set_particle_maps(eslam_ctx* ctx, int on)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    const bool cur = particle_maps(ctx);
    if ((on != 0) == cur) return ESLAM_OK;
    if (ctx->n) return fail(ctx, ESLAM_ERR_INVALID_ARG, "the map mode is chosen before the particles are initialised");
    if (on) ctx->cfg.flags |= ESLAM_FLAG_PARTICLE_MAPS;
    else ctx->cfg.flags &= ~ESLAM_FLAG_PARTICLE_MAPS;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_get_particle_map(eslam_ctx* ctx, uint64_t index, uint32_t* cells, float* mean, float* stdev,
                                          uint32_t capacity, uint32_t* count)
{
    if (!ctx || !count) return ESLAM_ERR_INVALID_ARG;
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (!particle_maps(ctx)) return fail(ctx, ESLAM_ERR_INVALID_ARG, "no per-particle maps (ESLAM_FLAG_PARTICLE_MAPS)");
    if (index >= ctx->n) return fail(ctx, ESLAM_ERR_INVALID_ARG, "particle index out of range");
    int rc = materialize(ctx);
    if (!rc) rc = read_ctl(ctx);
    if (rc) return rc;
    *count = 0;
    if (!ctx->lm_ready) return ESLAM_OK;
    const LocalMaps& lm = ctx->lm;
    const uint32_t* sid = ctx->st[ctx->ctl_host->base ^ ctx->ctl_host->flip].sid;
    uint32_t X = 0;
    HIPCHK(ctx, hipMemcpy(&X, sid + index, 4, hipMemcpyDeviceToHost));
    int2 c;
    std::vector<uint32_t> sl(lm.S);
    HIPCHK(ctx, hipMemcpy(&c, lm.ctr + X, sizeof(int2), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(sl.data(), lm.slot + (uint64_t)X * lm.S, lm.S * 4, hipMemcpyDeviceToHost));
    // the window's tiles in slot order, then the trail's in entry order, each tile's cells row
    // by row (the oracle's or_get_particle_map)
    uint32_t k = 0;
    float2 cell[DM_LM_PAGE_CELLS];
    const uint32_t W = lm.wx * lm.wy, toff = lm.S - 4u * lm.V;
    const uint32_t hw = sl[toff - 1u] == DM_LM_NONE ? 0u : sl[toff - 1u];   // the trail's used entries
    for (uint32_t s = 0; s < W + hw; ++s) {
            const bool tr = s >= W;
            const uint32_t pg = tr ? sl[toff + 4u * (s - W) + 2u] : sl[s];
            if (pg == DM_LM_NONE) continue;
            const int64_t a = tr ? (int64_t)(int32_t)sl[toff + 4u * (s - W)] : dm_lm_tile_of(s % lm.wx, c.x, lm.hx, lm.wx);
            const int64_t b = tr ? (int64_t)(int32_t)sl[toff + 4u * (s - W) + 1u] : dm_lm_tile_of(s / lm.wx, c.y, lm.hy, lm.wy);
            HIPCHK(ctx, hipMemcpy(cell, lm.page + (uint64_t)pg * DM_LM_PAGE_CELLS, sizeof(cell), hipMemcpyDeviceToHost));
            for (uint32_t j = 0; j < DM_LM_PAGE_CELLS; ++j) {
                if (!dm_lm_holds(cell[j].y)) continue;
                if (k < capacity) {
                    const uint64_t m = (uint64_t)(8 * a) + (j & 7u), n = (uint64_t)(8 * b) + (j >> 3);
                    if (cells) cells[k] = (uint32_t)(n * ctx->map.width + m);
                    if (mean) mean[k] = cell[j].x;
                    if (stdev) stdev[k] = cell[j].y;
                }
                ++k;
            }
    }
    *count = k;
    return ESLAM_OK;
}

// ---------------------------------------------------------------------------------------
// the shared map: processMap's merge into the one grid (eslam_shared_map.hip)
// ---------------------------------------------------------------------------------------
// a second set of the grid's arrays with room for `cap` patches; false (nothing held) when
// the device has no room
static bool sm_alloc_grid(GridBufs* g, uint64_t ncell, uint64_t cap, bool heights)
{
    *g = GridBufs{};
    const uint64_t c = cap ? cap : 1;
    bool ok = g->cells.alloc((ncell + 1) * 4) == hipSuccess && g->patch.alloc(c * sizeof(float2)) == hipSuccess &&
              g->occ.alloc(((ncell + 31) / 32) * 4) == hipSuccess && g->cell_tab.alloc(ncell * sizeof(uint4)) == hipSuccess;
    if (ok && heights) ok = g->height.alloc(c * 4) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        *g = GridBufs{};
    }
    return ok;
}

// the run scratch for `rec` records and `ncell` cells, carved from one allocation the context keeps
static int sm_scratch(eslam_ctx* ctx, uint64_t rec, uint64_t ncell, uint64_t scan_patches, SmScratch* s, ScanPatch** sp)
{
    const size_t sort_bytes = eslam_sm_sort_bytes(rec);
    Carver size(nullptr);
    carve_sm(size, rec, ncell, scan_patches, sort_bytes, s, sp);
    const uint64_t total = size.bytes();
    if (total > ctx->sm_mem.cap()) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->sm_mem.alloc(total) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "shared_map_update: no device memory for the run scratch (lower max_records)");
        }
    }
    Carver place(ctx->sm_mem.get());
    carve_sm(place, rec, ncell, scan_patches, sort_bytes, s, sp);
    return ESLAM_OK;
}

// ---- the merge on a sharded filter (eslam_gpu_shared_map_update_sharded): every rank merges
// every run into its own copy of the grid, from the run's poses gathered in global order
constexpr uint64_t kSmPoseBytes = kSmPoseWords * 8;

// the pose records of the run's particles [i0, i0 + np) (global), in global order, into `recv`:
// every rank stages its part of the run once per rank and the all_to_all_v hands every rank
// every part, in rank order -- the shards are consecutive, so that is the run's order
static int sm_exchange(eslam_ctx* ctx, uint64_t i0, uint64_t np, double* send, double* recv)
{
    const int G = ctx->comm.nranks, me = ctx->comm.rank;
    uint64_t sb[kMaxRanks], rb[kMaxRanks], first = 0, mine = 0;
    for (int r = 0; r < G; ++r) {
        const uint64_t a = i0 > ctx->gall[r] ? i0 : ctx->gall[r];
        const uint64_t b = i0 + np < ctx->gall[r + 1] ? i0 + np : ctx->gall[r + 1];
        const uint64_t c = b > a ? b - a : 0;
        rb[r] = c * kSmPoseBytes;
        if (r == me) {
            first = c ? a - ctx->gbase : 0;
            mine = c;
        }
    }
    for (int r = 0; r < G; ++r) sb[r] = mine * kSmPoseBytes;
    if (mine) HIPCHK(ctx, eslam_launch_sm_stage(ctx->st[0], ctx->st[1], ctx->ctl, first, mine, (uint32_t)G, send, ctx->stream));
    return comm_alltoallv(ctx, send, sb, recv, rb);
}

static uint64_t sm_patch_hash(const eslam_scan_patch* patches, uint32_t count)
{
    uint64_t h = 0xcbf29ce484222325ull;                        // FNV-1a over the patches' bytes
    const unsigned char* p = reinterpret_cast<const unsigned char*>(patches);
    for (uint64_t k = 0; k < (uint64_t)count * sizeof(eslam_scan_patch); ++k) h = (h ^ p[k]) * 0x100000001b3ull;
    return h;
}

// both entry points.  collective: eslam_gpu_shared_map_update_sharded; on a sharded filter
// (sh) the runs cover the global index range and read gathered poses.
static int sm_update(eslam_ctx* ctx, const eslam_scan_patch* patches, uint32_t count, uint64_t max_records,
                     eslam_shared_merge_info* info, bool collective)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!ctx || (!patches && count)) return ESLAM_ERR_INVALID_ARG;
    if (particle_maps(ctx))
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "shared_map_update: the filter has per-particle maps (eslam_gpu_map_update merges into those)");
    for (uint32_t k = 0; k < count; ++k)
        if (!dm_isfinite(patches[k].position[0]) || !dm_isfinite(patches[k].position[1]) ||
            !dm_isfinite(patches[k].position[2]) || !dm_isfinite(patches[k].stdev))
            return fail(ctx, ESLAM_ERR_INVALID_ARG, "shared_map_update: scan patches must be finite");
    if (!ctx->has_map) return fail(ctx, ESLAM_ERR_NO_ENVIRONMENT, "No environment attached.");
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (ctx->sharded && !collective)
        return fail(ctx, ESLAM_ERR_UNSUPPORTED,
                    "shared_map_update: a sharded filter keeps a copy of the grid per rank; the merge in global particle "
                    "order is the collective eslam_gpu_shared_map_update_sharded");
    const bool sh = ctx->sharded;
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    const uint64_t ncell = (uint64_t)ctx->map.width * ctx->map.height_cells;
    if (sh) {
        // every check above ran before the first collective; then the ranks must have been given
        // the same call, or their grids would differ from here on
        if (count && ncell >= 0xffffffffull)
            return fail(ctx, ESLAM_ERR_UNSUPPORTED, "shared_map_update: the grid has 2^32 - 1 cells or more");
        if (const int rc_ = settle(ctx)) return rc_;           // a deferred sharded exchange first
        const uint64_t mine[3] = {count, max_records, sm_patch_hash(patches, count)};
        static_assert(sizeof(mine) <= kHostXBytes, "host_allgather's buffer");
        if (const int rc_ = same_on_every_rank(ctx, mine, 3,
                                               "shared_map_update_sharded: the ranks passed different scans or max_records; every "
                                               "rank must make the same call"))
            return rc_;
    }
    if (info) info->n_patches = ctx->map_np;
    if (!count) return ESLAM_OK;
    if (ncell >= 0xffffffffull) return fail(ctx, ESLAM_ERR_UNSUPPORTED, "shared_map_update: the grid has 2^32 - 1 cells or more");
    // a run: whole particles, at most max_records records, at least one particle
    const uint64_t P = count, n = sh ? ctx->n_global : ctx->n;
    uint64_t lim = max_records ? max_records : kSmDefaultRecords;
    if (lim > (1ull << 31)) lim = 1ull << 31;                  // record indices are 32-bit
    uint64_t per = lim / P;
    per = per < 1 ? 1 : (per > n ? n : per);
    SmScratch sc;
    ScanPatch* d_sp = nullptr;
    double *x_send = nullptr, *x_recv = nullptr;               // a sharded run's pose records, out and in
    auto setup = [&]() -> int {
        int rc = sm_scratch(ctx, per * P, ncell, P, &sc, &d_sp);
        if (!rc && sh) {
            // the staged copies (one per rank) and the gathered run
            const uint64_t G = ctx->comm.nranks, out = (G * per * kSmPoseBytes + 255) & ~255ull;
            hipError_t he_ = hipSuccess;
            rc = ctx->sm_x.grow_keep(out + per * kSmPoseBytes, 1, ctx->stream, &he_);
            if (rc == ESLAM_ERR_OUT_OF_MEMORY)
                return fail(ctx, rc, "shared_map_update_sharded: no device memory for the exchange (lower max_records)");
            if (rc) HIPCHK(ctx, he_);
            x_send = reinterpret_cast<double*>(ctx->sm_x.as<char>());
            x_recv = reinterpret_cast<double*>(ctx->sm_x.as<char>() + out);
        }
        if (!rc) rc = materialize(ctx);                       // the particles as they stand
        if (rc) return rc;
        static_assert(sizeof(ScanPatch) == sizeof(eslam_scan_patch), "scan patch layout");
        HIPCHK(ctx, hipMemcpyAsync(d_sp, patches, P * sizeof(ScanPatch), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(sc.cnt, 0, kSmCounters * 8, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(sc.touched, 0, ncell * 4, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));       // `patches` is the caller's
        return ESLAM_OK;
    };
    int rc = setup();
    if (sh) rc = agree(ctx, rc, "shared_map_update_sharded");   // an allocation can fail on one rank only
    if (rc) return rc;
    GridBufs spare;
    uint64_t spare_cap = 0;
    uint64_t cnt[kSmCounters] = {};
    uint64_t done = 0, runs = 0, placed_all = 0;
    hipError_t he = hipSuccess;
    // what k_sm_place / k_sm_apply read the poses from: the particles, or (SmRun::gath) the gathered run
    DevState gathered = {};
    gathered.x = x_recv;
    const DevState a0 = sh ? gathered : ctx->st[0], a1 = sh ? gathered : ctx->st[1];
    for (uint64_t i0 = 0; i0 < n && !rc; i0 += per) {
        const uint64_t np = n - i0 < per ? n - i0 : per;
        SmRun run = {};
        run.i0 = sh ? 0 : i0;
        run.P = count;
        run.R = np * P;
        run.ncell = (uint32_t)ncell;
        run.is_id = ctx->map.g2l_identity;
        run.sp = d_sp;
        run.gath = sh ? 1u : 0u;
        if (sh && (rc = sm_exchange(ctx, i0, np, x_send, x_recv)) != ESLAM_OK) break;
        uint64_t placed = 0;
        // the new arrays exist before anything of the grid changes: a run that finds no room
        // leaves the grid as the runs before it made it
        do {
            if ((he = eslam_launch_sm_place(a0, a1, ctx->ctl, &ctx->map, &run, &sc, ctx->stream)) != hipSuccess) break;
            if ((he = hipMemcpyAsync(&placed, sc.cnt + kSmRunPlaced, 8, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) break;
            if ((he = hipStreamSynchronize(ctx->stream)) != hipSuccess) break;
            if (!placed) break;
            const uint64_t need = ctx->map_np + placed;
            if (need > 0xffffffffull) {
                rc = fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "shared_map_update: the grid would pass 2^32 - 1 patches");
                break;
            }
            if (!spare.cells || spare_cap < need) {
                uint64_t want = need + need / 4;
                want = want > 0xffffffffull ? 0xffffffffull : want;
                const bool h = ctx->grid.height != nullptr;
                spare_cap = sm_alloc_grid(&spare, ncell, want, h) ? want : sm_alloc_grid(&spare, ncell, need, h) ? need : 0;
                if (!spare_cap) rc = fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "shared_map_update: no device memory for the merged grid");
            }
        } while (0);
        if (sh) {
            // the ranks agree before any of them changes its grid (the apply fuses in place): after
            // a failure every rank holds the grid of the same completed runs
            if (he != hipSuccess) {
                ctx->err = std::string("shared_map_update: ") + hipGetErrorString(he);
                he = hipSuccess;
                rc = ESLAM_ERR_HIP;
            }
            rc = agree(ctx, rc, "shared_map_update_sharded");
        }
        if (he != hipSuccess || rc) break;
        if (placed) {
            const SmGrid cur = ctx->grid.view(), next = spare.view();
            if ((he = eslam_launch_sm_merge(a0, a1, ctx->ctl, &run, &cur, &next, &sc, ctx->stream)) != hipSuccess) break;
            uint32_t total = 0;
            if ((he = hipMemcpyAsync(&total, next.cell_start + ncell, 4, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) break;
            if ((he = hipStreamSynchronize(ctx->stream)) != hipSuccess) break;
            // the swap: every later launch takes the grid from ctx->map (K1's window staging, the
            // match, the hash build and get_map read these pointers at their call)
            std::swap(ctx->grid, spare);                          // the next run rebuilds into the old arrays
            std::swap(ctx->map_np_cap, spare_cap);
            ctx->map_np = total;
            ctx->map.cell_start = ctx->grid.cells; ctx->map.patch = ctx->grid.patch; ctx->map.height = ctx->grid.height;
            ctx->map.occ = ctx->grid.occ; ctx->map.cell_tab = ctx->grid.cell_tab;
        }
        placed_all += placed;
        done = i0 + np;
        ++runs;
    }
    if (he == hipSuccess) he = hipMemcpy(cnt, sc.cnt, sizeof(cnt), hipMemcpyDeviceToHost);
    spare = GridBufs{};                                          // (hipFree waits for the device)
    if (info) {
        info->particles_done = done;
        info->patches_placed = placed_all;
        info->patches_off_grid = done * P - placed_all;
        info->cells_touched = cnt[kSmTouched];
        info->fused = cnt[kSmFused];
        info->absorbed = cnt[kSmAbsorbed];
        info->inserted = cnt[kSmInserted];
        info->n_patches = ctx->map_np;
        info->runs = runs;
    }
    if (he != hipSuccess) {
        ctx->err = std::string("shared_map_update: ") + hipGetErrorString(he);
        return ESLAM_ERR_HIP;
    }
    return rc;
}

extern "C" int eslam_gpu_shared_map_update(eslam_ctx* ctx, const eslam_scan_patch* patches, uint32_t count, uint64_t max_records,
                                           eslam_shared_merge_info* info)
{
    return sm_update(ctx, patches, count, max_records, info, false);
}

extern "C" int eslam_gpu_shared_map_update_sharded(eslam_ctx* ctx, const eslam_scan_patch* patches, uint32_t count,
                                                   uint64_t max_records, eslam_shared_merge_info* info)
{
    return sm_update(ctx, patches, count, max_records, info, true);
}

extern "C" int eslam_gpu_map_size(eslam_ctx* ctx, uint32_t* width, uint32_t* height, uint64_t* n_patches, int* has_height)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (!ctx->has_map) return fail(ctx, ESLAM_ERR_NO_ENVIRONMENT, "No environment attached.");
    if (width) *width = ctx->map.width;
    if (height) *height = ctx->map.height_cells;
    if (n_patches) *n_patches = ctx->map_np;
    if (has_height) *has_height = ctx->grid.height ? 1 : 0;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_get_map(eslam_ctx* ctx, uint32_t* cell_start, float* mean, float* stdev, float* patch_height,
                                 uint64_t patch_capacity)
{
    if (!ctx || !cell_start || ((!mean || !stdev) && patch_capacity)) return ESLAM_ERR_INVALID_ARG;
    if (!ctx->has_map) return fail(ctx, ESLAM_ERR_NO_ENVIRONMENT, "No environment attached.");
    const uint64_t np = ctx->map_np, ncell = (uint64_t)ctx->map.width * ctx->map.height_cells;
    if (patch_capacity < np) return fail(ctx, ESLAM_ERR_INVALID_ARG, "get_map: patch_capacity is below the grid's patch count (eslam_gpu_map_size)");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(cell_start, ctx->grid.cells, (ncell + 1) * 4, hipMemcpyDeviceToHost));
    if (!np) return ESLAM_OK;
    std::vector<float2> patch(np);
    HIPCHK(ctx, hipMemcpy(patch.data(), ctx->grid.patch, np * sizeof(float2), hipMemcpyDeviceToHost));
    for (uint64_t k = 0; k < np; ++k) {
        mean[k] = patch[k].x;
        stdev[k] = patch[k].y;
    }
    if (patch_height) {
        if (ctx->grid.height) HIPCHK(ctx, hipMemcpy(patch_height, ctx->grid.height, np * 4, hipMemcpyDeviceToHost));
        else memset(patch_height, 0, np * 4);
    }
    return ESLAM_OK;
}

// ---------------------------------------------------------------------------------------
// a particle's whole map as one grid (kernels in eslam_particle_grid.hip)
// ---------------------------------------------------------------------------------------
// The checks of the three entry points, then the directory of particle index's table and the
// composed counts (in *s): *total = the composed grid's patches.
static int pgrid_count(eslam_ctx* ctx, uint64_t index, PgScratch* s, uint64_t* total)
{
    if (const int rc_ = settle(ctx)) return rc_;    // a deferred sharded exchange first
    if (!particle_maps(ctx)) return fail(ctx, ESLAM_ERR_INVALID_ARG, "no per-particle maps (ESLAM_FLAG_PARTICLE_MAPS)");
    if (!ctx->has_map) return fail(ctx, ESLAM_ERR_NO_ENVIRONMENT, "No environment attached.");
    if (!ctx->n) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "no particles");
    if (index >= ctx->n) return fail(ctx, ESLAM_ERR_INVALID_ARG, "particle index out of range");
    if (const int rc_ = check_poisoned(ctx)) return rc_;
    const uint64_t ncell = (uint64_t)ctx->map.width * ctx->map.height_cells;
    if (ncell >= 0xffffffffull) return fail(ctx, ESLAM_ERR_UNSUPPORTED, "particle_grid: the grid has 2^32 - 1 cells or more");
    int rc = materialize(ctx);
    if (!rc) rc = read_ctl(ctx);
    if (rc) return rc;
    if (!ctx->lm_ready) return fail(ctx, ESLAM_ERR_NOT_INITIALISED, "per-particle maps are not set up");
    const size_t bytes = eslam_pgrid_work_bytes(ctx->map.width, ctx->map.height_cells, nullptr, nullptr);
    if (bytes > ctx->pg_mem.cap() && ctx->pg_mem.alloc(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "particle_grid: no device memory for the scratch");
    }
    (void)eslam_pgrid_work_bytes(ctx->map.width, ctx->map.height_cells, ctx->pg_mem.get(), s);
    const uint32_t* sid = ctx->st[ctx->ctl_host->base ^ ctx->ctl_host->flip].sid;
    HIPCHK(ctx, eslam_launch_pgrid_count(&ctx->lm, sid + index, &ctx->map, s, ctx->stream));
    uint64_t own = 0;
    HIPCHK(ctx, hipMemcpyAsync(&own, s->own, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *total = ctx->map_np + own;
    if (*total > 0xffffffffull) return fail(ctx, ESLAM_ERR_INVALID_ARG, "particle_grid: the composed grid would pass 2^32 - 1 patches");
    return ESLAM_OK;
}

// ... and the composed grid itself in ctx->pg_out, a second set of the grid's arrays that stays
// with the context for the next export (allocating them cost more than composing into them);
// a count above `capacity` (the caller's arrays) is refused first
static int pgrid_compose(eslam_ctx* ctx, uint64_t index, uint64_t* total, uint64_t capacity)
{
    PgScratch s;
    if (const int rc_ = pgrid_count(ctx, index, &s, total)) return rc_;
    if (capacity < *total)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "get_particle_grid: patch_capacity is below the composed patch count (eslam_gpu_particle_grid_size)");
    const uint64_t ncell = (uint64_t)ctx->map.width * ctx->map.height_cells;
    const bool h = ctx->grid.height != nullptr;
    if (!ctx->pg_out.cells || ctx->pg_out_cells != ncell || ctx->pg_out_cap < *total || (ctx->pg_out.height != nullptr) != h) {
        // room for the window and the trail full of patches, so other particles' exports fit too
        uint64_t want = ctx->map_np + ((uint64_t)ctx->lm.wx * ctx->lm.wy + ctx->lm.V) * DM_LM_PAGE_CELLS;
        want = want < *total ? *total : (want > 0xffffffffull ? 0xffffffffull : want);
        ctx->pg_out_cells = ncell;
        ctx->pg_out_cap = sm_alloc_grid(&ctx->pg_out, ncell, want, h) ? want : sm_alloc_grid(&ctx->pg_out, ncell, *total, h) ? *total : 0;
        if (!ctx->pg_out.cells) {
            ctx->pg_out_cap = ctx->pg_out_cells = 0;
            return fail(ctx, ESLAM_ERR_OUT_OF_MEMORY, "particle_grid: no device memory for the composed grid");
        }
    }
    const SmGrid cur = ctx->grid.view(), nw = ctx->pg_out.view();
    HIPCHK(ctx, eslam_launch_pgrid_fill(&ctx->lm, &ctx->map, &s, &cur, &nw, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ESLAM_OK;
}

extern "C" int eslam_gpu_particle_grid_size(eslam_ctx* ctx, uint64_t index, uint64_t* n_patches)
{
    if (!ctx || !n_patches) return ESLAM_ERR_INVALID_ARG;
    PgScratch s;
    return pgrid_count(ctx, index, &s, n_patches);
}

extern "C" int eslam_gpu_get_particle_grid(eslam_ctx* ctx, uint64_t index, uint32_t* cell_start, float* mean, float* stdev,
                                           float* patch_height, uint64_t patch_capacity)
{
    if (!ctx || !cell_start || !mean || !stdev) return ESLAM_ERR_INVALID_ARG;
    uint64_t np = 0;
    if (const int rc_ = pgrid_compose(ctx, index, &np, patch_capacity)) return rc_;
    const GridBufs& out = ctx->pg_out;
    const uint64_t ncell = (uint64_t)ctx->map.width * ctx->map.height_cells;
    HIPCHK(ctx, hipMemcpy(cell_start, out.cells, (ncell + 1) * 4, hipMemcpyDeviceToHost));
    if (!np) return ESLAM_OK;
    std::vector<float2> patch(np);
    HIPCHK(ctx, hipMemcpy(patch.data(), out.patch, np * sizeof(float2), hipMemcpyDeviceToHost));
    for (uint64_t k = 0; k < np; ++k) {
        mean[k] = patch[k].x;
        stdev[k] = patch[k].y;
    }
    if (patch_height) {
        if (out.height) HIPCHK(ctx, hipMemcpy(patch_height, out.height, np * 4, hipMemcpyDeviceToHost));
        else memset(patch_height, 0, np * 4);
    }
    return ESLAM_OK;
}

extern "C" int eslam_gpu_adopt_particle_map(eslam_ctx* ctx, uint64_t index)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    // refused before any collective (settle is one)
    if (ctx->sharded)
        return fail(ctx, ESLAM_ERR_UNSUPPORTED,
                    "adopt_particle_map: a sharded filter keeps a copy of the grid per rank; export the map on the owning "
                    "rank (eslam_gpu_get_particle_grid) and give it to every rank by eslam_gpu_set_map");
    // the new arrays exist before anything changes
    uint64_t np = 0;
    if (const int rc_ = pgrid_compose(ctx, index, &np, ~0ull)) return rc_;
    // as eslam_gpu_set_map: the grid's arrays, the view every later launch reads, no pose hash,
    // and every particle's map starts over, empty (they name cells of the previous grid)
    ctx->grid = std::move(ctx->pg_out);                          // (hipFree waits for the device)
    ctx->pg_out = GridBufs{};
    const uint64_t cap = ctx->pg_out_cap;
    ctx->pg_out_cap = ctx->pg_out_cells = 0;
    ctx->map.cell_start = ctx->grid.cells; ctx->map.patch = ctx->grid.patch; ctx->map.height = ctx->grid.height;
    ctx->map.occ = ctx->grid.occ; ctx->map.cell_tab = ctx->grid.cell_tab;
    ctx->map.has_height = ctx->grid.height ? 1u : 0u;
    ctx->map_np = np;
    ctx->map_np_cap = cap ? cap : 1;
    ctx->has_hash = false;
    return local_maps_reset(ctx);
}

// ---------------------------------------------------------------------------------------
// the scan MLS from a sensor reading (kernels in eslam_scan.hip)
// ---------------------------------------------------------------------------------------
extern "C" int eslam_scan_params_default(const eslam_config* cfg, eslam_scan_params* p)
{
    if (!p) return ESLAM_ERR_INVALID_ARG;
    memset(p, 0, sizeof(*p));
    p->sensor2body[0] = p->sensor2body[5] = p->sensor2body[10] = 1.0;
    p->orientation[0] = 1.0;
    p->sensor_rot_sigma[0] = 5.0 / 180.0 * M_PI;       // scanAngleSigma  src/EmbodiedSlamFilter.cpp:281, 323
    p->body_rot_sigma[0] = p->body_rot_sigma[1] = 3.0 / 180.0 * M_PI;   // pitchRollSigma  :290, 332
    p->min_sigma = 1e-3;                               // :124
    p->resolution = 0.05;                              // Configuration::gridResolution
    p->patch_thickness = 0.1;                          // Configuration::gridPatchThickness
    p->max_sensor_range = cfg ? cfg->max_sensor_range : 3.0;
    return ESLAM_OK;
}

// the frame of a build from the caller's parameters (reach: see dm_scan_frame_init)
static int scan_frame(eslam_ctx* ctx, const eslam_scan_params* p, double ray, dm_scan_frame* f)
{
    bool fin = true;
    for (int i = 0; i < 12; ++i) fin = fin && dm_isfinite(p->sensor2body[i]);
    for (int i = 0; i < 4; ++i) fin = fin && dm_isfinite(p->orientation[i]);
    for (int i = 0; i < 3; ++i) fin = fin && dm_isfinite(p->sensor_rot_sigma[i]) && dm_isfinite(p->body_rot_sigma[i]);
    fin = fin && dm_isfinite(p->min_sigma) && dm_isfinite(p->resolution) && dm_isfinite(p->patch_thickness) &&
          dm_isfinite(p->max_sensor_range) && dm_isfinite(ray);
    if (!fin) return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan: transforms, sigmas and sizes must be finite");
    if (!(p->min_sigma > 0.0)) return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan: min_sigma must be positive");
    if (!(p->resolution > 0.0) || !(p->patch_thickness > 0.0) || !(p->max_sensor_range > 0.0))
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan: resolution, patch_thickness and max_sensor_range must be positive");
    // R_w = removeYaw(orientation), as fill_step_params compensates the feet
    double yc[4], Rw[9];
    remove_yaw(p->orientation, yc);
    q_to_mat(yc, Rw);
    if (!dm_scan_frame_init(f, p->sensor2body, Rw, p->sensor_rot_sigma, p->body_rot_sigma, p->min_sigma, p->resolution,
                            p->patch_thickness, p->max_sensor_range, p->max_sensor_range * ray))
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan: the scan grid would pass 2^32 - 1 cells (resolution too fine for the range)");
    return ESLAM_OK;
}

// a buffer of at least `bytes`: the new one exists before the old one goes, so a failed
// allocation leaves the context with what it had
template <typename B>
static int scan_grow(eslam_ctx* ctx, B& buf, uint64_t bytes, uint64_t unit, const char* what)
{
    hipError_t he = hipSuccess;
    const int rc = buf.grow_keep(bytes, unit, ctx->stream, &he);
    if (rc == ESLAM_ERR_OUT_OF_MEMORY) return fail(ctx, rc, what);
    HIPCHK(ctx, he);
    return ESLAM_OK;
}

static int scan_build(eslam_ctx* ctx, const dm_scan_frame* f, ScanReading* rd, const void* host_raw, eslam_scan_info* info)
{
    const uint64_t n = rd->n;
    ctx->scan_count = 0;
    if (info) info->points = n;
    if (!n) return ESLAM_OK;
    const uint64_t need = eslam_scan_work_bytes(n, nullptr, nullptr);
    if (const int rc_ = scan_grow(ctx, ctx->scan_mem, need, 1, "scan: no device memory for the build's scratch"))
        return rc_;
    ScanWork w;
    (void)eslam_scan_work_bytes(n, ctx->scan_mem, &w);
    HIPCHK(ctx, hipMemcpyAsync(w.raw, host_raw, n * 4, hipMemcpyHostToDevice, ctx->stream));
    rd->raw = w.raw;
    HIPCHK(ctx, eslam_launch_scan_order(f, rd, &w, ctx->stream));
    uint64_t cnt[kScanCounters] = {};
    uint32_t nheads = 0, total = 0;
    HIPCHK(ctx, hipMemcpyAsync(cnt, w.cnt, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&nheads, w.b + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // `host_raw` is the caller's
    const uint64_t binned = n - cnt[kScanInvalid] - cnt[kScanOutOfRange];
    if (info) {
        info->points_valid = binned;
        info->points_invalid = cnt[kScanInvalid];
        info->points_out_of_range = cnt[kScanOutOfRange];
        info->cells = nheads;
    }
    if (!nheads) return ESLAM_OK;
    HIPCHK(ctx, eslam_launch_scan_count(f, &w, nheads, (uint32_t)binned, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&total, w.a + nheads, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (const int rc_ = scan_grow(ctx, ctx->scan_out, (uint64_t)total * sizeof(eslam_scan_patch),
                                  sizeof(eslam_scan_patch), "scan: no device memory for the patches"))
        return rc_;
    HIPCHK(ctx, eslam_launch_scan_emit(f, &w, nheads, (uint32_t)binned, ctx->scan_out, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->scan_count = total;
    if (info) info->patches = total;
    return ESLAM_OK;
}

extern "C" int eslam_gpu_scan_from_laser(eslam_ctx* ctx, const eslam_laser_scan* scan, const eslam_scan_params* params,
                                         eslam_scan_info* info)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (!scan || !params || (scan->n && !scan->ranges)) return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan_from_laser: null argument");
    if (!dm_isfinite(scan->start_angle) || !dm_isfinite(scan->angular_resolution))
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan_from_laser: the angles must be finite");
    if (scan->n > kScanMaxPoints) return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan_from_laser: more than 2^30 beams");
    dm_scan_frame f;
    if (const int rc_ = scan_frame(ctx, params, 1.0, &f)) return rc_;
    ScanReading rd = {};
    rd.depth = 0;
    rd.n = scan->n;
    rd.start_angle = scan->start_angle;
    rd.angular_resolution = scan->angular_resolution;
    rd.min_range = scan->min_range;
    rd.max_range = scan->max_range;
    rd.width = 1;
    return scan_build(ctx, &f, &rd, scan->ranges, info);
}

extern "C" int eslam_gpu_scan_from_depth(eslam_ctx* ctx, const eslam_depth_image* image, const eslam_scan_params* params,
                                         eslam_scan_info* info)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (!image || !params || !image->data) return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan_from_depth: null argument");
    if (!image->width || !image->height) return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan_from_depth: a zero-size image");
    if ((uint64_t)image->width * image->height > kScanMaxPoints)
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan_from_depth: more than 2^30 pixels");
    if (!dm_isfinite(image->scale_x) || !dm_isfinite(image->scale_y) || !dm_isfinite(image->center_x) ||
        !dm_isfinite(image->center_y))
        return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan_from_depth: the image's scales and centres must be finite");
    dm_scan_frame f;
    const double ray = dm_scan_depth_ray(image->width, image->height, image->scale_x, image->scale_y, image->center_x,
                                         image->center_y);
    if (const int rc_ = scan_frame(ctx, params, ray, &f)) return rc_;
    ScanReading rd = {};
    rd.depth = 1;
    rd.n = image->width * image->height;
    rd.width = image->width;
    rd.sx = image->scale_x; rd.sy = image->scale_y; rd.cx = image->center_x; rd.cy = image->center_y;
    return scan_build(ctx, &f, &rd, image->data, info);
}

extern "C" int eslam_gpu_scan_patches(eslam_ctx* ctx, eslam_scan_patch* out, uint64_t capacity, uint64_t* count)
{
    if (!ctx) return ESLAM_ERR_INVALID_ARG;
    if (!count || (!out && capacity)) return fail(ctx, ESLAM_ERR_INVALID_ARG, "scan_patches: null argument");
    *count = ctx->scan_count;
    const uint64_t m = capacity < ctx->scan_count ? capacity : ctx->scan_count;
    if (m) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(out, ctx->scan_out, m * sizeof(eslam_scan_patch), hipMemcpyDeviceToHost));
    }
    return ESLAM_OK;
}
