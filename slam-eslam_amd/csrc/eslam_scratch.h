// eslam_scratch.h -- host-only: the layouts of the scratch blocks that are carved from one device
// allocation each.  A layout is a function of a Carver (eslam_buf.h) that names every array once,
// in the block's order; its caller runs it over a null base for the block's size and over the
// block for the pointers.  Plain functions of sizes, so tests/cpp/test_buf.cpp checks them
// without a device.
#pragma once

#include "eslam_internal.h"
#include "eslam_buf.h"

namespace eslam_host {

using eslam_buf::Carver;

// eslam_gpu_shared_map_update's run scratch: `rec` records, `ncell` cells, the sort's
// `sort_bytes` (eslam_sm_sort_bytes) and the scan's patches
inline void carve_sm(Carver& c, uint64_t rec, uint64_t ncell, uint64_t scan_patches, size_t sort_bytes, eslam_dev::SmScratch* s,
                     eslam_dev::ScanPatch** sp)
{
    s->keys = c.take<uint32_t>(rec + 1);
    s->vals = c.take<uint32_t>(rec);
    s->keys_out = c.take<uint32_t>(rec);
    s->order = c.take<uint32_t>(rec);
    s->app = c.take<float2>(rec);
    s->add = c.take<uint32_t>(ncell);
    s->segpos = c.take<uint32_t>(ncell);
    s->touched = c.take<uint32_t>(ncell);
    s->cnt = c.take<uint64_t>(eslam_dev::kSmCounters);
    s->sort_tmp = c.take_bytes(sort_bytes);
    s->sort_tmp_bytes = sort_bytes;
    *sp = c.take<eslam_dev::ScanPatch>(scan_patches);
}

// a resample of n particles (tn tiles) to `samples` (ts tiles): the cumulative sum, its coarse
// level, the counter's line, the draws' ancestors, the compacted ancestors (the multinomial draw
// only; otherwise the draws' own) and the compaction's counts
struct ResampleScratch {
    uint64_t *C, *coarse, *counter;
    uint32_t *anc, *anc_kept, *kept;
};
inline void carve_resample(Carver& c, uint64_t n, uint64_t tn, uint64_t samples, uint64_t ts, bool multi, ResampleScratch* s)
{
    s->C = c.take<uint64_t>(n);
    s->coarse = c.take<uint64_t>(tn);
    s->counter = c.take<uint64_t>(1);
    s->anc = c.take<uint32_t>(samples);
    s->anc_kept = multi ? c.take<uint32_t>(samples) : s->anc;
    s->kept = c.take<uint32_t>(ts + 1);
}

// the same on a sharded filter, per rank: C and its coarse level over the rank's own n particles,
// the call's counters (kRsWords), and, for the multinomial draw only, the kept draws of every
// tile of global draws (far below one 32-bit word per global draw); no word per draw otherwise
struct ResampleShardScratch {
    uint64_t *C, *coarse, *counter;
    uint32_t* kept;
};
inline void carve_resample_sharded(Carver& c, uint64_t n, uint64_t tn, uint64_t ts, bool multi, ResampleShardScratch* s)
{
    s->C = c.take<uint64_t>(n);
    s->coarse = c.take<uint64_t>(tn);
    s->counter = c.take<uint64_t>(eslam_dev::kRsWords);
    s->kept = multi ? c.take<uint32_t>(ts + 1) : nullptr;
}

// a snapshot's census over `ntables` pool tables, `cap` particles and `npages` pool pages
// (SnapCensus::counts is a buffer of its own)
inline void carve_census(Carver& c, uint64_t ntables, uint64_t cap, uint64_t npages, eslam_dev::SnapCensus* s)
{
    s->first = c.take<uint32_t>(ntables);
    s->trank = c.take<uint32_t>(ntables);
    s->tlist = c.take<uint32_t>(cap);
    s->firstref = c.take<uint64_t>(npages);
    s->prank = c.take<uint32_t>(npages);
    s->plist = c.take<uint32_t>(npages);
}

// a scan build of n points with the radix sort's `sort_bytes`
inline void carve_scan(Carver& c, uint64_t n, size_t sort_bytes, eslam_dev::ScanWork* s)
{
    s->a = c.take<uint32_t>(n + 1);
    s->b = c.take<uint32_t>(n + 1);
    s->c = c.take<uint32_t>(n + 1);
    s->d = c.take<uint32_t>(n + 1);
    s->e = c.take<uint32_t>(n + 1);
    s->raw = c.take<uint32_t>(n + 1);
    s->pz = c.take<double>(n ? n : 1);
    s->var = c.take<double>(n ? n : 1);
    s->sz = c.take<double>(n ? n : 1);
    s->sv = c.take<double>(n ? n : 1);
    s->cnt = c.take<uint64_t>(eslam_dev::kScanCounters);
    s->sort_tmp = c.take_bytes(sort_bytes);
    s->sort_tmp_bytes = sort_bytes;
}

// a KLD bin count over a bitmap of `words` 64-bit words: a pass' folded record, the blocks'
// records, the bitmap and, on a filter sharded over `gather` ranks (0: not sharded), theirs
inline void carve_kld(Carver& c, uint64_t words, uint64_t gather, eslam_dev::KldScratch* s)
{
    s->out = c.take<int64_t>(eslam_dev::kKldWords);
    s->part = c.take<int64_t>((uint64_t)eslam_dev::kKldBlocks * eslam_dev::kKldWords);
    s->bits = c.take<uint64_t>(words);
    s->all = c.take<uint64_t>(gather * words);
}

// the trajectory log's block (eslam_gpu_trajectory_enable): `steps` ring entries of `slots`
// particles each, then the two link buffers
inline void carve_traj_log(Carver& c, uint64_t steps, uint64_t slots, eslam_dev::TrajEntry* entry, uint32_t* link[2])
{
    for (uint64_t k = 0; k < steps; ++k) {
        eslam_dev::TrajEntry e;
        e.x = c.take<double>(slots);
        e.y = c.take<double>(slots);
        e.z = c.take<double>(slots);
        e.yaw = c.take<double>(slots);
        e.zs = c.take<double>(slots);
        e.parent = c.take<uint32_t>(slots);
        if (entry) entry[k] = e;
    }
    for (int b = 0; b < 2; ++b) link[b] = c.take<uint32_t>(slots);
}

// a trace of `count` lineages through `steps` entries: the entries, the leaves, the nodes
struct TrajTraceScratch {
    eslam_dev::TrajLevel* lv;
    uint32_t* leaf;
    eslam_dev::TrajNode* nodes;
};
inline void carve_traj_trace(Carver& c, uint64_t count, uint64_t steps, TrajTraceScratch* s)
{
    s->lv = c.take<eslam_dev::TrajLevel>(steps);
    s->leaf = c.take<uint32_t>(count);
    s->nodes = c.take<eslam_dev::TrajNode>(count * steps);
}

// the smoothed sweep over n leaves through entries of at most `slots` particles: the scratch
// state's six columns, the leaves' ancestors, and a KLD count's record, block records and bitmap
struct TrajSmoothScratch {
    double *x, *y, *th, *z, *zs, *w;
    uint32_t* a;
    eslam_dev::KldScratch k;
};
inline void carve_traj_smooth(Carver& c, uint64_t n, uint64_t slots, TrajSmoothScratch* s)
{
    double** f[6] = {&s->x, &s->y, &s->th, &s->z, &s->zs, &s->w};
    for (int j = 0; j < 6; ++j) *f[j] = c.take<double>(n);
    s->a = c.take<uint32_t>(n);
    carve_kld(c, (slots + 63) / 64, 0, &s->k);
}

// The log of a sharded filter.  The exchange's scratch by the requests a rank makes (`count`
// positions bucketed by `nblocks` blocks): the packed requests, their positions, the blocks'
// counts and the totals ...
struct TrajFetchOut {
    uint32_t *req, *pos, *cnt, *tot;
};
inline void carve_traj_fetch_out(Carver& c, uint64_t count, uint64_t nblocks, TrajFetchOut* s)
{
    s->req = c.take<uint32_t>(count);
    s->pos = c.take<uint32_t>(count);
    s->cnt = c.take<uint32_t>(nblocks * eslam_dev::kMaxRanks);
    s->tot = c.take<uint32_t>(eslam_dev::kTrajTotWords);
}
// ... and by the `tin` requests received and the `tout` answers awaited, of `item` bytes each
struct TrajFetchIn {
    uint32_t* reqin;
    void *served, *answers;
};
inline void carve_traj_fetch_in(Carver& c, uint64_t tin, uint64_t tout, uint64_t item, TrajFetchIn* s)
{
    s->reqin = c.take<uint32_t>(tin);
    s->served = c.take_bytes(tin * item);
    s->answers = c.take_bytes(tout * item);
}
// a sharded trace of `count` leaves through `steps` entries: the leaves, their slots in the level
// at hand, the level's items, the nodes; `all`: every rank's leaves, compared before the walk
struct TrajTraceSharded {
    uint32_t *leaf, *a, *all;
    eslam_dev::TrajItem* items;
    eslam_dev::TrajNode* nodes;
};
inline void carve_traj_trace_sharded(Carver& c, uint64_t count, uint64_t steps, uint64_t nranks, TrajTraceSharded* s)
{
    s->leaf = c.take<uint32_t>(count);
    s->a = c.take<uint32_t>(count);
    s->all = c.take<uint32_t>(count * nranks);
    s->items = c.take<eslam_dev::TrajItem>(count);
    s->nodes = c.take<eslam_dev::TrajNode>(count * steps);
}
// a record or a composition through a link that is not the identity: the n particles' sources
// and the words fetched for them
struct TrajLinkScratch {
    uint32_t *src, *got;
};
inline void carve_traj_link(Carver& c, uint64_t n, TrajLinkScratch* s)
{
    s->src = c.take<uint32_t>(n);
    s->got = c.take<uint32_t>(n);
}

// a particle-grid composition on tx x ty tiles with `blocks` blocks of cells
inline void carve_pgrid(Carver& c, uint64_t tx, uint64_t ty, uint64_t blocks, eslam_dev::PgScratch* s)
{
    s->dir = c.take<uint32_t>(tx * ty);
    s->bsum = c.take<uint32_t>(blocks + 1);
    s->own = c.take<uint64_t>(1);
    s->tx = (uint32_t)tx;
    s->ty = (uint32_t)ty;
}

}  // namespace eslam_host
