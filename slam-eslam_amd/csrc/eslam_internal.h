// eslam_internal.h -- shared between the HIP kernels and the host side of libeslam_gpu.
//
// Device memory layout (per context, one GPU):
//   state[2]   SoA fp64 x, y, theta, zpos, zsigma, weight, mprob + uint8 flags
//              (flags = n_contact_points | floating << 7); double-buffered for resample
//   marks      uint32 per particle: resample segment starts (particle index + 1)
//   row_first  uint32 per 64 outputs: source covering the row's first output
//   tile_sum   uint64 per scan tile: exact fixed-point weight total (K3a), read by K3b
//   shards     NSHARD x Shard: exact fixed-point statistics of the weighting kernel
//   ctl        Ctl: per-step scalars decided on the device (no host round trip per step)
//   jump       minstd jump-ahead tables A^(i), A^(i*2^11), A^(i*2^22)
#pragma once
#include <stdint.h>
#include "../../include/eslam_gpu.h"
#include "../../include/eslam_detmath.h"

namespace eslam_dev {

constexpr int kBlock = 256;              // threads per block (4 waves of 64)
constexpr int kWaves = kBlock / 64;
constexpr int kScanItems = 8;            // particles per thread in the scan kernel
constexpr int kScanTile = kBlock * kScanItems;   // 2048 particles per scan tile
constexpr int kGatherTile = kScanTile;           // outputs per resample-gather block
constexpr int kRow = 64;                         // outputs per row_first entry (one wave row)
constexpr int kNShard = 16;              // statistics shards (blockIdx % kNShard)
constexpr int kJumpBits = 11;
constexpr int kStatsLds = 2048;          // bytes of the statistics scratch at the LDS base
#ifndef ESLAM_WINDOW_LDS                 // experiment builds may shrink it
#define ESLAM_WINDOW_LDS 29696
#endif
// bytes of the MLS window after the statistics (1856 cells).  gfx950 allocates LDS in 1280-byte
// granules (inferred, r04i): K1 blocks of 32 736 B ran four per CU (each took 33 280 of the
// 160 KB), blocks of 31 776 B (32 000 allocated) run five: K1 180 -> 167 us at 4M
constexpr int kWindowLds = ESLAM_WINDOW_LDS;
#ifndef ESLAM_K1_BM_LDS                  // experiment builds may leave the tables in global memory
#define ESLAM_K1_BM_LDS 1
#endif
// K1 stages the two Box-Muller tables (dm_bm_log_tab 4 KB, dm_bm_sc_tab32 2 KB) in the last
// kBmLds bytes of the window's LDS when the staged window leaves them free (the bench's cloud
// needs about a third of the window), and reads them from global memory otherwise: no byte of
// LDS more, and the same table values either way
constexpr int kBmLds = 6144;
static_assert(kBmLds <= kWindowLds, "the tables lie inside the window's LDS");
#ifndef ESLAM_K1_ATTR                    // experiment builds may set an occupancy attribute on K1
#define ESLAM_K1_ATTR
#endif

#if defined(__HIPCC__)
// A^e for e < 2^32 from the context's three jump tables: A^(i), A^(i*2^11), A^(i*2^22)
__device__ __forceinline__ uint32_t jump_pow(const uint32_t* __restrict__ jt, uint64_t e)
{
    uint32_t a = jt[e & 2047u];
    uint32_t b = jt[2048u + ((e >> 11) & 2047u)];
    uint32_t c = jt[4096u + ((e >> 22) & 1023u)];
    return dm_mulmod31(dm_mulmod31(a, b), c);
}
#endif

// one statistics shard: exact sums as 4 limbs of 32-bit columns (uint64 each)
struct alignas(128) Shard {
    uint64_t A[DM_NBUCKETS][4];          // sum over chunks of  w_A * mprob        (per bucket)
    uint64_t B[DM_NBUCKETS][4];          // sum over chunks of (w_A * mprob)^2     (per bucket)
    uint64_t SW[4];                      // sum of m^(1/n) over accepted particles
    uint64_t D, TP;                      // data_particles, total_points
    uint64_t maxm;                       // bits of max accepted m (non-negative double)
    uint64_t flags;                      // bit q: accumulator q NaN, bit 16+q: infinite
    uint64_t err;                        // bit 0: zero measurement variance
    uint64_t bbox[4];                    // max of ~key(min x), key(max x), ~key(min y), key(max y)
    uint64_t pad[3];
};
static_assert(sizeof(Shard) % 128 == 0, "shard alignment");

// per-step device-side control block
struct alignas(128) Ctl {
    // committed buffer index and pending flip (latest state = base ^ flip)
    uint32_t base, flip;
    uint32_t resample;                   // decided by finalize for this update
    uint32_t uniform;                    // sumWeights <= 0 branch
    uint32_t mode;                       // finalize mode (see FinMode)
    uint32_t special;                    // 1: S NaN, 2: S inf
    uint32_t gather;                     // a resample gather is pending (marks -> state[base^1])
    uint32_t aborted;                    // the update hit the zero-measurement-variance error (phase B,
                                         // normalisation and resample skipped, as the reference's throw)
    int32_t scan_shift;                  // fixed-point shift of the resample cumulative sum
    int32_t wexp;                        // weight exponent bound for the next weighting
    double S, Q, eff, fw, max_weight;
    double f[DM_NBUCKETS];
    double inv_n;
    uint32_t minstd;                     // ParticleFilter::rand_gen state
    uint32_t minstd_start;               // state at the start of the current resample
    uint64_t tile_counter;               // dynamic tile id of the scan kernel
    uint64_t overruns;
    uint64_t data_particles, total_points;
    uint64_t update_count;
    uint64_t err;
    uint64_t bbox[4];                    // particle bounding box of the last weighting (keys)
    uint32_t k3_base;                    // the buffer the last weighting kernel wrote (base ^ flip at
                                         // its start): the fused K3 reads it while block 0 commits
    uint64_t map_dropped;                // scan patches the last map merge could not store (full stores)
    uint64_t map_changed;                // stores the last map merge changed
    uint64_t map_copied;                 // shared stores the last map merge wrote to a free store
    uint64_t map_covered;                // scan patches the last map merge saw on cells the shared grid covers
    uint64_t map_written;                // cell writes (inserts and fuses) of the last map merge
    uint64_t map_taken;                  // pages the last map merge took from the free list
    uint64_t map_evicted;                // tiles the last map update's full trails forgot
    uint64_t pg_cursor;                  // per-particle maps: next unused entry of LocalMaps::frees
    uint64_t pg_nfree;                   //   entries in LocalMaps::frees (the last collection)
    uint64_t pg_total;                   //   pages the current map update may take (its plan)
    uint32_t pg_gc;                      //   the current map update collects first
    uint32_t pg_pad;
    uint64_t fin_epoch;                  // fused finalize: the epoch of the launch whose finalize wrote
                                         // this block (checked in every block's copy of it)
};

enum FinMode : uint32_t {
    FIN_UPDATE = 0,       // updateWeights statistics -> phase B factors, normalise, maybe resample
    FIN_NORMALIZE = 1,    // standalone normalizeWeights (weights as they are)
    FIN_RESAMPLE = 2,     // standalone resample (no normalisation)
    FIN_SUM = 3,          // getWeightsSum only
};

struct DevState {
    double* x; double* y; double* th; double* z; double* zs; double* w; double* mprob;
    uint8_t* flags;
    uint32_t* sid;                       // per-particle maps only: the particle's map store
};

// Per-particle local maps (useSharedMap = false, ESLAM_FLAG_PARTICLE_MAPS): the
// shared grid plus, per particle, a window of (2 hx + 1) x (2 hy + 1) tiles of 8 x 8 cells
// around the particle (eslam_detmath.h DM_LM_*: the window reaches maxSensorRange and moves
// with the particle at every map update) and a trail of up to V tiles the window has left.
//   table  what a particle names (DevState::sid): the window centre and a row of S words: the
//          window's slots (wx * wy; the slot of tile (a, b) being (a mod wx) + wx (b mod wy),
//          each a page id or DM_LM_NONE), DM_LM_NONE words up to a multiple of 4 whose last two
//          are bookkeeping, no page ids (the shadow flag, then the trail's high-water mark:
//          dm_lm_row_words always leaves room for both), then the trail's V entries
//          {a, b, page, -} (page DM_LM_NONE: empty; lm_trail_* below).  Whoever walks a row's
//          pages reads the wx * wy slots and the trail's used entries, nothing in between.
//          The resample copies the name, so copies share a table; a map update that changes
//          a table another particle also names writes the result to a free table the particle
//          then names (copy on write: a shared table is never written).
//   page   the 64 cells {mean, stdev} of one tile (stdev >= 0: the cell holds a patch).  Pages
//          are shared by tables the same way; a page is written in place only by the table
//          that owns it at the table's current generation (LocalMaps::owner == gen << 32 |
//          table), and a table's generation moves on whenever it is shared, so every page it
//          had is then frozen and copied on the next write.  Free pages come from a list the
//          map update's collection rebuilds (mark the pages live tables name, compact the
//          rest) when the list runs short.
// K1 reads the first 64 bytes (LocalMaps up to my) with one scalar load per lookup.
struct LocalMaps {
    int2* ctr;                           // per table: window centre tile (DM_LM_UNSET: an empty table)
    uint32_t* slot;                      // per table: S page ids
    float2* page;                        // per page: 64 cells {mean, stdev}, row-major (m & 7) + 8 (n & 7)
    uint32_t S, wx, wy, hx;              // S: words per table row (dm_lm_row_words(wx wy, V))
    uint32_t hy, V;                      // V: trail entries per table (the last 4 V words of a row)
    uint64_t mx, my;                     // lm_magic(wx), lm_magic(wy)
    // --- the map update and the collection only
    uint32_t bx, by;                     // multiples of wx, wy >= 2^29 (non-negative residues)
    uint32_t* tgen;                      // per table: generation (bumped when a map update finds it shared)
    uint64_t* owner;                     // per page: gen << 32 | the table that may write it in place
    uint32_t* frees;                     // the free pages, in page order, from the last collection
    uint8_t* mark;                       // per page: a live table names it (the collection's marks)
    uint64_t npages, ntables;
};
static_assert(sizeof(int2) == 8, "centre");
constexpr int kMaxRanks = 16;

// sharded filters: a particle that a resample received from another rank names no local table
// yet; its sid is kSidRecord | the record index, and the copy on write that follows the gather
// gives it a free table (and pages) filled from the record's payload (the migrated map)
constexpr uint32_t kSidRecord = 0x80000000u;
// a migrated map: the header per record (its table's centre and page count), then the pages
// of all records in the records' order, each with its slot
struct alignas(8) MapPayHdr {
    int2 ctr;
    uint32_t npg;
    uint32_t share;                      // bit 0: the previous record (same source, same destination)
                                         // carries this record's map (npg 0): they name one table;
                                         // bit 1: the map holds copies of shared-grid cells (kLmShadow)
};
// the first record of each destination's range of a sharded send (PlanParams::send_off): a
// record there always carries its map
struct PaySeg {
    uint64_t off[kMaxRanks + 1];
    int32_t n;
    int32_t pad;
};
struct alignas(8) MapPayPage {
    uint32_t slot;                       // a window slot, or kPayTrail | trail entry e of tile (a, b)
    int32_t a, b;
    uint32_t pad;
    float2 cell[DM_LM_PAGE_CELLS];
};
static_assert(sizeof(MapPayPage) == 528, "payload page");
constexpr uint32_t kPayTrail = 0x80000000u;
// a table row's word lm_trail_off - 2 (the first of the two bookkeeping words every row
// reserves after its window's slots, dm_lm_row_words): kLmShadow when the map holds its own
// copy of a cell the shared grid covers (lookups then ask the particle's cells first)
constexpr uint32_t kLmShadow = 1u;
// the tables' pool holds 2 x cap tables: at most n <= cap are named by a particle, so at least
// cap are free whenever a map update starts, and particle i may take the i-th free one (copy
// on write with a fixed, deterministic allocation of tables and no allocation counter)
inline uint64_t store_pool(uint64_t cap) { return 2 * cap; }
// a ceil(2^35 / w) multiplier: (a * m) >> 35 = floor(a / w), exactly, for a < 2^30 and
// 3 <= w <= 31 (a * m < 2^64; the rounding error a * (m w - 2^35) / (w 2^35) < 1 / w)
constexpr uint32_t kLmMagicShift = 35;
inline uint64_t lm_magic(uint32_t w) { return ((1ull << kLmMagicShift) + w - 1) / w; }
constexpr uint32_t kDefaultMapPages = 16;       // pages per particle when the config says 0

// K1 reads the first 64 bytes (the lookup header) with one scalar load per lookup
struct MapView {
    const uint32_t* cell_start;
    const float2* patch;                 // (mean, stdev) per patch
    double inv_scale_x, inv_scale_y, offset_x, offset_y;
    uint32_t width, height_cells;
    uint32_t g2l_identity;               // global2local is exactly the identity
    uint32_t has_height;                 // height != nullptr
    const float* height;                 // nullable: all horizontal
    double g2l[12];
    const uint32_t* occ;                 // bit c: the shared grid has patches in cell c (the map merge's test)
    // per cell {first patch mean, stdev (float bits), begin, count}: K1's window rows stage
    // with one 16-byte load per cell, and a lookup off the window is one load for the cell and
    // its first patch (the same values as cell_start / patch)
    const uint4* cell_tab;
};

struct ContactC {
    double px, py, zp, zz;               // yaw-compensated body-frame x, y; zp = 0.0 * pz and
                                         // zz = (0.0 * px + 0.0 * py): the zero terms of
                                         // Affine3d * p (exact, uniform per step)
    double pz;
    uint32_t eval;                       // !(contact < 0.2)
    uint32_t end;                        // group ends after this contact
};

// The head of StepParams is laid out for K1's scalar loads at the point of use (field
// order matters: see k_project_weight); the rest is read before the particle loop.
struct StepParams {
    // ---- project (PoseEstimator::project): Philox key, odometry sampler, z motion
    uint64_t seed, proj_event, gbase;    // +0
    double mu[3];                        // +24
    double L00, L10, L11, L20, L21;      // +48
    double L22, slip_factor, yaw, max_yaw_dev;   // +88
    double z_delta, z_var;               // +120
    // ---- weighting (updateWeights)
    double me2, radius, corr;            // +136
    uint64_t min_contacts;               // +160
    uint32_t use_shape;                  // +168
    uint32_t m;                          // number of contacts
    uint32_t eval_mask, end_mask;        // bit i: contact i evaluated / ends its group
    uint32_t hash_use, use_slip;
    double spread_threshold, spread_trans, spread_rot;
    // ---- sizes
    uint64_t n, n_global;
    uint32_t J;                          // canonical chunk rows
    uint32_t use_window;                 // stage the MLS window under the cloud in LDS
    double win_margin;                   // world-frame margin around the last bounding box
    ContactC c[ESLAM_MAX_CONTACTS];
};

// one particle migrating between GPUs at a multi-GPU resample (72 bytes)
struct alignas(8) Rec {
    double x, y, th, z, zs, w, mprob;
    uint64_t lohi;                       // [lo, hi) of the outputs it fills (global, clipped)
    uint64_t src;                        // flags | global source index << 8
};
static_assert(sizeof(Rec) == 72, "record size");

// A resample to a count on a sharded filter (eslam_resample.hip, DESIGN.md 5 "Resample to a
// count, sharded"): what every draw's routing needs.  This rank owns the thresholds in
// (off, off + total] (rank 0 also T = 0) of the global fixed-point sum gtotal; the new shard table
// nb[] names the rank of every output; the records for rank d start at send_off[d].  A migrating
// particle travels as a Rec whose lohi is its output's index within the destination's new shard
// and whose src is flags | old global index << 8.
struct RsPlan {
    uint64_t off, total, gtotal;
    uint64_t n, ntiles;                  // this rank's particles and their tiles of C
    uint64_t samples;
    double inv_samples;
    uint64_t gbase;                      // this rank's first particle in the old global indexing
    uint64_t nb[kMaxRanks + 1];          // the new table
    uint64_t send_off[kMaxRanks + 1];    // records: first of every destination (+ their count)
    int32_t G, me;
    uint32_t set_weight, pad;            // multinomial: every output's weight is `weight`
    double weight;
};
// the call's counters (uint64 words): draws beyond the sum, records per destination, fill cursors,
// records this rank will receive (its outputs whose ancestors other ranks hold)
constexpr int kRsBeyond = 0, kRsCount = 1, kRsCursor = kRsCount + kMaxRanks, kRsRecv = kRsCursor + kMaxRanks,
              kRsWords = kRsRecv + 1;

// multi-GPU mark encoding (monotone in output order): records from lower ranks,
// then this rank's own particles, then records from higher ranks
constexpr uint32_t kMarkOwn = 1u << 30, kMarkHigh = 1u << 31;

// a pending resample gather, consumed by the next k_project_weight (or k_resample_gather)
struct GatherView {
    uint32_t* marks;
    const uint32_t* row_first;
    uint32_t* anc;                       // ancestors (global indices) when record
    const Rec* recs;                     // multi-GPU: migrated particles
    uint32_t record;
    uint32_t multi;                      // marks use the multi-GPU source encoding
};

// which chunks a k_project_weight launch processes: all (mode 0); the own chunks named by the
// device words cdev[0..1] (mode 1); the others, [0, c_lo) and [c_hi, nchunks) (mode 2)
struct ChunkSel {
    uint32_t mode;
    uint32_t pad;
    uint64_t c_lo, c_hi;
    const uint64_t* cdev;
};

// k_project_weight's single kernel argument: its fields are read with scalar loads from the
// kernel-argument segment where they are used (offsetof), see k_project_weight
struct K1Args {
    StepParams p;
    MapView map;
    GatherView gv;
    DevState s[2];
    Ctl* ctl;
    Shard* shards;
    LocalMaps store;                     // per-particle maps (the DELTA instantiations only)
    ChunkSel sel;                        // the chunks this launch processes
    double* bspill;                      // per chunk: the per-bucket sums a wave is not in (k1_bspill_bytes)
};
// K1 keeps the per-bucket sums of the bucket its wave is in in registers; a wave whose
// particles fall into several buckets parks the others per lane in its chunk's slot here
// (DM_NBUCKETS x {A, B} x 64 lanes), so the register file holds one pair instead of six
inline uint64_t k1_bspill_bytes(uint64_t chunks) { return chunks * DM_NBUCKETS * 2 * 64 * sizeof(double); }

// one scan patch of a map update (the scan MLS of processMap, in the yaw-free body frame)
struct ScanPatch {
    double x, y, z, stdev;
};
constexpr int kMaxScanPatches = 64;
// a map update merges a scan in parts of kScanPartSmall patches (a scan of at most that many:
// one part) or of kScanPartLarge (larger scans: fewer parts, so each tile is staged about once)
constexpr uint32_t kScanPartSmall = 64, kScanPartLarge = 256;
// processMap(scanMap, match = true) (k_map_match): every kMatchSampling-th scan patch
constexpr uint32_t kMatchSampling = 10;          // src/EmbodiedSlamFilter.cpp:216
constexpr double kMatchSigma = (double)0.2f;     // :217 (a float there)
struct MatchParams {
    uint64_t n;
    uint32_t m;                          // the sampled patches in sp
    uint32_t is_id;                      // the grid's global2local is the identity
    const ScanPatch* sp;                 // device copy of the sampled patches (more than kMaxScanPatches)
    ScanPatch spi[kMaxScanPatches];      // else the sampled patches themselves (sp null)
};
constexpr int kLmBlock = 128;                   // particles per block of the page plan (k_map_plan, k_recv_plan)
constexpr uint32_t kMergeCounterSlots = 256;   // the merge's statistics, spread over slots
constexpr uint32_t kMergeCounters = 7;

// the store names of both state buffers; the copy-on-write kernels use the current one
// (base ^ flip read on the device, so the host never waits for the commit)
struct SidRef {
    uint32_t* s0;
    uint32_t* s1;
    const Ctl* ctl;
};
// the copy-on-write scratch (u32 words): ref (pool), the two compactions' tile counts, the
// free stores (pool), the received particles (cap), the received count, the free count
struct CowScratch {
    uint32_t* ref;                       // particles naming each store
    uint32_t* counts;                    // 2 x (tiles + 1)
    uint32_t* frees;                     // the stores no particle names, in store order
    uint32_t* dups;                      // the particles received from another rank (sid = kSidRecord | record)
    uint32_t* ndup;
    uint32_t* nfree;
    uint32_t tiles;                      // compaction tiles over the pool (>= the tiles over the particles)
};
constexpr int kCompactItems = 8;                // k_compact_*: items per thread
constexpr int kCompactTileItems = kBlock * kCompactItems;
inline uint64_t cow_words(uint64_t cap)
{
    const uint64_t pool = store_pool(cap), tiles = (pool + kCompactTileItems - 1) / kCompactTileItems;
    return pool + 2 * (tiles + 1) + pool + cap + 2;
}
inline CowScratch cow_layout(uint32_t* base, uint64_t cap)
{
    const uint64_t pool = store_pool(cap), tiles = (pool + kCompactTileItems - 1) / kCompactTileItems;
    CowScratch c;
    c.ref = base;
    c.counts = c.ref + pool;
    c.frees = c.counts + 2 * (tiles + 1);
    c.dups = c.frees + pool;
    c.ndup = c.dups + cap;
    c.nfree = c.ndup + 1;
    c.tiles = (uint32_t)tiles;
    return c;
}
// k_map_plan -> k_map_merge, per particle (one 128-byte record): what the plan decided, so
// the merge's first memory round trip brings everything its page moves need
constexpr uint32_t kJobPlaced = 1u, kJobShared = 2u, kJobMore = 4u, kJobMoved = 8u;   // flags; tiles of pass 1 << 8
constexpr uint32_t kJobCovered = 16u;    // a patch of this part lands on a cell the shared grid covers
struct alignas(16) MergeJob {
    uint32_t X, T;                       // the table the particle names; the table its merge writes
    uint64_t gT;                         // tgen[T] << 32 | T: the owner word of T's pages
    int32_t na, nb;                      // the window's new centre
    int32_t ox, oy;                      // its old centre (ctr[X]; the plan has moved T's window)
    uint32_t flags;
    uint32_t need;                       // bit r: tile r of pass 1 takes a new page
    uint16_t L[8];                       // pass 1's tiles (slots, ascending)
    uint32_t P[8];                       // their pages in X (DM_LM_NONE: none)
    double z, zs;                        // zPos, zSigma (the offset patch)
    uint32_t src, pad[5];                // the particle the merge reads (gather); pad to 128 B
};
static_assert(sizeof(MergeJob) == 128, "merge job");

struct MergeParams {
    uint64_t n;
    uint32_t m;                          // scan patches
    uint32_t is_id;                      // the grid's global2local is the identity
    uint64_t* cnt;                       // kMergeCounters x kMergeCounterSlots: dropped patches, changed
                                         // tables, copies, patches on covered cells, cell writes, pages
                                         // taken, tiles the trail forgot (zeroed)
    const uint32_t* ref;                 // CowScratch::ref of this update
    const uint32_t* frees;               // CowScratch::frees: particle i's table if it writes a shared map
    uint32_t* off;                       // per particle: its first page of the plan within its plan block
                                         // (k_map_plan / k_recv_plan: the exclusive prefix of the needs)
    uint32_t* poff;                      // per block of kLmBlock particles: first page offset (+ total)
    MergeJob* job;                       // per particle: k_map_plan's record for the merge
    uint16_t* codes;                     // per particle: a part's scan-patch cell codes (plan; the part's stride)
    uint32_t* fault;                     // host-mapped fault word (kFaultPages)
    GatherView gv;                       // fuse: a pending resample gather runs in the merge (one GPU)
    uint64_t gbase;
    uint32_t fuse, aux;                  // aux: carry mprob / flags (ESLAM_FLAG_NO_AUX_GATHER unset)
    uint32_t acc, pad2;                  // acc: add this merge's counters to the update's (a later 64-patch part)
    const ScanPatch* sp;                 // the part's patches (device copy of the scan)
};

// ---- the shared map's merge (eslam_gpu_shared_map_update, eslam_shared_map.hip) ----------
// One run: particles [i0, i0 + np) x the scan's P patches = R records, record r = (i0 + r / P,
// r % P), so record order is the contract's (particle, patch) order.
struct SmRun {
    uint64_t i0;
    uint64_t R;                          // np * P < 2^32
    uint32_t P;
    uint32_t ncell;                      // width * height: also the key of a record that is not placed
    uint32_t is_id;                      // the grid's global2local is the identity
    uint32_t gath;                       // 0: the particles' own columns at i0 + ip.  1, a sharded run (i0 = 0): the
                                         //   DevState's x names the run's gathered records, kSmPoseWords doubles each
    const ScanPatch* sp;                 // the scan (device)
};
constexpr uint32_t kSmPoseWords = 5;     // a sharded run's pose record: x, y, theta, zPos, zSigma (40 bytes)
// the grid's arrays a merge reads and writes (fuses in place) or rebuilds into
struct SmGrid {
    uint32_t* cell_start;
    float2* patch;
    float* height;                       // null: all horizontal
    uint32_t* occ;
    uint4* cell_tab;
};
// the scratch of a run, bounded by max_records (and the cell count): about 32 bytes per record
struct SmScratch {
    uint32_t* keys;                      // R + 1: the records' cells in record order; after the sort, the
                                         //   segment-head flags and their exclusive scan (flag[R]: heads)
    uint32_t* vals;                      // R: the record indices; after the sort, the heads' positions
    uint32_t* keys_out;                  // R: cells, sorted (stable)
    uint32_t* order;                     // R: the records in sorted order
    float2* app;                         // R: patches a cell's segment appended, at the segment's start
    uint32_t* add;                       // per cell: patches this run appended (zeroed per run)
    uint32_t* segpos;                    // per cell with add > 0: its segment's start
    uint32_t* touched;                   // per cell: a placed patch reached it in this call
    uint64_t* cnt;                       // kSmCounters counters: the call's, and the current run's placed records
    void* sort_tmp;
    size_t sort_tmp_bytes;
};
enum SmCounter : uint32_t { kSmFused = 0, kSmAbsorbed, kSmInserted, kSmTouched, kSmRunPlaced, kSmCounters = 8 };
constexpr uint64_t kSmDefaultRecords = 1ull << 21;   // max_records = 0: 64 MiB of scratch

// ---- a particle's whole map as one grid (eslam_gpu_get_particle_grid, eslam_particle_grid.hip) --
// the scratch of a composition, carved from one allocation of the context (eslam_pgrid_work_bytes)
struct PgScratch {
    uint32_t* dir;                       // tx * ty: the page of the particle's table per grid tile (DM_LM_NONE: none)
    uint32_t* bsum;                      // per block of kBlock cells (+ 1): the composed lists' total length, then
                                         //   the exclusive scan of those (the last: the composed grid's patches)
    uint64_t* own;                       // the particle's own patches on the grid
    uint32_t tx, ty;                     // the grid in tiles of 8 x 8 cells (rounded up)
};

// ---- the scan MLS from a sensor reading (eslam_gpu_scan_from_*, eslam_scan.hip) --
// the reading: a laser scan (ranges) or a depth image (float bits), n points
struct ScanReading {
    uint32_t depth;                      // 0: laser, 1: depth image
    uint32_t n;
    const uint32_t* raw;                 // device: ranges (mm) or the image's float words
    double start_angle, angular_resolution;
    uint32_t min_range, max_range;
    uint32_t width, pad;
    double sx, sy, cx, cy;
};
// the scratch of a build, carved from one allocation of the context (scan_work_bytes); the u32
// arrays have n + 1 words and are reused from stage to stage as eslam_scan.hip lists
struct ScanWork {
    uint32_t* a;                         // the points' cells (ncell: not binned); later the clusters per segment
    uint32_t* b;                         // their z keys; the cells in z order; the head flags and their scan
    uint32_t* c;                         // the point indices; after the second sort, the points in canonical order
    uint32_t* d;                         // sorted keys of both sorts (the cells, in the end)
    uint32_t* e;                         // the points in z order; later the segments' first positions
    double* pz;                          // per point: height and its variance
    double* var;
    double* sz;                          // the same in canonical order
    double* sv;
    uint64_t* cnt;                       // kScanInvalid, kScanOutOfRange
    uint32_t* raw;                       // the reading
    void* sort_tmp;
    size_t sort_tmp_bytes;
};
enum ScanCounter : uint32_t { kScanInvalid = 0, kScanOutOfRange, kScanCounters = 4 };
constexpr uint64_t kScanMaxPoints = 1ull << 30;

// ---- snapshots (eslam_gpu_save / eslam_gpu_load, eslam_snapshot.hip) ---------
// the census of a save: the live tables and pages and their compact ids in canonical order
struct SnapCensus {
    uint32_t* first;                     // per pool table: the lowest particle naming it (0xffffffff: none)
    uint32_t* trank;                     // per pool table: its compact id
    uint32_t* tlist;                     // per compact id: the pool table (n entries)
    uint64_t* firstref;                  // per pool page: the lowest key (table rank x (W + V) + word) naming it
    uint32_t* prank;                     // per pool page: its compact id
    uint32_t* plist;                     // per compact id: the pool page
    uint32_t* counts;                    // the compactions' tile counts
};
// a sharded load's subset of a snapshot: the tables this rank's particles name and the pages
// those tables name, as bitmaps over the snapshot's compact ids; the local id of a set bit b
// is pre[b >> 5] + popc(bits[b >> 5] & below(b & 31)) (set bits keep their order)
struct SnapSubset {
    uint32_t* tbits;                     // (tables + 31) / 32 words
    uint32_t* tpre;                      // their exclusive popcount prefix, the total behind it
    uint32_t* pbits;                     // (pages + 31) / 32 words
    uint32_t* ppre;
    uint64_t tables, pages;              // the snapshot's counts (ids at or past them are never looked up)
};
constexpr uint64_t kSnapDefaultChunk = 64ull << 20;

// logDebug records of the last update (k_contact_records), indexed by the particle's
// position during that update: meas 4 doubles (x, y, zPos, theta), ncp, and maxc contact
// points of 6 doubles (surface point xyz, zdiff, zvar, prob)
struct DebugRec {
    double* meas;
    uint8_t* ncp;
    double* cp;
    uint32_t* resampled;                 // the update's resample decision (copied from Ctl)
    uint32_t maxc;
};

struct FinParams {
    uint64_t n_global;
    uint64_t min_effective;
    double discount;
    double spread_threshold;
    uint32_t mode;
    int32_t wexp;                        // scale exponent used by the statistics kernel
    uint32_t record;                     // 1: write update info
    uint32_t minstd_jump_n;              // A^n_global mod (2^31 - 1): the resample's N draws
    // multi-GPU only (null otherwise): the shards this rank all-gathered, zeroed once read,
    // and 3 words next to the gathered totals (resample, minstd_start, scan_shift) so the
    // host reads everything it needs for the all_to_all_v sizes with one copy
    Shard* local_shards;
    uint64_t* mirror;
};

// the finalize fused into the one-GPU K3 (k_normalize_segments<ITEMS, true>): block 0 runs
// k_finalize's block over the local shards and publishes epoch in *fin_word
struct FusedFin {
    Shard* shards;                       // the statistics shards (all ranks' on a sharded filter)
    FinParams fp;
    uint64_t* fin_word;
    uint64_t epoch;
    int nrec;                            // shards to reduce (kNShard, or kNShard x ranks)
};


struct ScanParams {
    uint64_t n, gbase, n_global;
    uint32_t phase_b;                    // apply phase-B factors
    uint32_t normalize;                  // divide by S
    uint32_t ntiles;
    uint32_t multi;                      // multi-GPU: tile prefixes + rank total, no marks
    uint32_t items;                      // particles per thread of K3: tile = kBlock * items
                                         // (2, 4 or kScanItems; sharded: kScanItems)
    uint32_t tag;                        // one GPU: this launch's tile-total tag (1..7, cycled per launch)
    uint32_t spin_limit;                 // polls of a cross-block wait before it gives up (kSpinLimit;
                                         // 0: give up at once, eslam_gpu_debug_set_spin_limit)
    uint32_t* fault;                     // host-mapped word: kFaultTimeout when a wait gave up
    uint32_t pub_stride;                 // one GPU: words between the replicas of K3's tile words
};
// K3 (one GPU) publishes each tile word in kPubReplicas copies, pub_stride words apart, and a
// tile reads the copy of its XCD (tile % kPubReplicas): every tile reads every earlier word, so
// one copy makes its few lines a hot spot of the memory system
constexpr uint32_t kPubReplicas = 8;

// A cross-block wait that gave up (a preceding tile's total or the fused finalize never
// arrived) poisons the filter: the device ORs kFaultTimeout into ctl->err and into a
// host-mapped word, writes nothing further, and every later launch that sees the bit in
// ctl->err returns at once; the host refuses the filter until it is re-initialised.
constexpr uint32_t kFaultTimeout = 4u;
// the per-particle maps' page pool could not hold a map update's pages even after a collection:
// the update wrote nothing and the filter is poisoned like a timeout (ESLAM_ERR_OUT_OF_MEMORY)
constexpr uint32_t kFaultPages = 8u;
constexpr uint32_t kSpinLimit = 1u << 18;    // x s_sleep(8) (512 clocks): ~60 ms


struct PlanParams {
    uint64_t n_global;
    int32_t rank, nranks;
    uint64_t gbase[kMaxRanks + 1];       // first global index of every rank (+ n_global)
    // per destination d != rank (host-computed from the all-gathered totals): this rank's
    // outputs in d's slice [sd[d], ed[d]) and their offsets in the send buffer
    uint64_t sd[kMaxRanks], ed[kMaxRanks];
    uint64_t send_off[kMaxRanks + 1];
    // the deferred exchange: the segments kernel writes the chunks of this rank's
    // slice whose outputs all come from its own particles, [chunk_sel[0], chunk_sel[1])
    uint64_t* chunk_sel;
    uint64_t n_local;
    uint32_t J;
};

// Chunks (64 J outputs each) of a rank's slice [W0, W0 + n) that hold only outputs of its own
// particles, whose outputs are [O0, O1) globally: the rest -- a prefix filled from lower ranks,
// a suffix from higher ranks -- needs the exchanged records.  Host and device compute it alike.
__host__ __device__ inline void own_chunks(uint64_t O0, uint64_t O1, uint64_t W0, uint64_t n, uint32_t J, uint64_t* c_lo,
                                           uint64_t* c_hi)
{
    const uint64_t csz = 64ull * J, nchunks = (n + csz - 1) / csz;
    const uint64_t lo = O0 <= W0 ? 0 : (O0 - W0 < n ? O0 - W0 : n);
    uint64_t hi = O1 <= W0 ? 0 : (O1 - W0 < n ? O1 - W0 : n);
    hi = hi < lo ? lo : hi;
    const uint64_t cl = (lo + csz - 1) / csz;
    uint64_t ch = hi == n ? nchunks : hi / csz;
    *c_lo = cl;
    *c_hi = ch < cl ? cl : ch;
}

// The pose distribution's Gaussian mixture (eslam_gmm.hip).
// Pass B's words: integer maxima of ordered keys (a minimum as the maximum of ~key) and counts,
// all zero before the kernel; the maxima mean something only when kGmmUsed is non-zero.
constexpr int kGmmMaxW = 0, kGmmMinX = 1, kGmmMaxX = 2, kGmmMinY = 3, kGmmMaxY = 4, kGmmUsed = 5, kGmmSkipped = 6;
constexpr int kGmmWords = 8;
constexpr int kGmmBoundsBlocks = 1024;       // blocks of pass B at most (each wave leaves kGmmWords words)
// finite doubles (-0.0 excluded) in unsigned integer order, and back
__host__ __device__ inline uint64_t gmm_key(double v)
{
    const uint64_t b = dm_bits(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double gmm_unkey(uint64_t k)
{
    return dm_from_bits((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}
// one pass' arguments: the centre, the weight scale 2^-E, the hard assignment's axis (0: x) and
// slabs [amin + k h, ...), and the parameters of the E-step
struct GmmPass {
    double cx, cy;
    double amin, h;
    int32_t E, axis;
    dm_gmm_comp c[DM_GMM_MAX];
};

// The pose estimate's moments (eslam_moments.hip).  Pass B's words: the maximum of
// the valid particles' weight keys (gmm_key) and the three counts, all zero before the kernel.
constexpr int kMomMaxW = 0, kMomCounted = 1, kMomGatedOut = 2, kMomSkipped = 3;
constexpr int kMomWords = 4;
constexpr int kMomBoundsBlocks = 1024;       // blocks of pass B at most (each wave leaves kMomWords words)
// a pass' arguments: the gate, the weight scale 2^-E and (pass 2) the mean the deviations are taken around
struct MomPass {
    dm_mom_gate g;
    double mean[4];
    int32_t E, pad;
};

// KLD-sampling's bin count (eslam_kld.hip).  A record of pass 1: the minima and
// maxima of the counted particles' cell indices (INT32_MAX / INT32_MIN where nothing was counted)
// and the counts of counted and skipped particles; the population count's record uses kKldCounted
constexpr int kKldIx0 = 0, kKldIx1 = 1, kKldIy0 = 2, kKldIy1 = 3, kKldCounted = 4, kKldSkipped = 5;
constexpr int kKldWords = 6;
constexpr int kKldBlocks = 1024;             // blocks of a pass at most (each leaves one record)
// the lattice and the box a marking pass sets bits in
struct KldGrid {
    double inv;                          // 1.0 / bin_xy
    uint32_t theta_bins, pad;
    int64_t ix0, iy0;                    // the box's origin
    uint64_t nx;                         // cells of a row of the box
};
struct KldScratch {
    int64_t* out;                        // kKldWords: a pass' folded record
    int64_t* part;                       // kKldBlocks records
    uint64_t* bits;                      // the bitmap's words
    uint64_t* all;                       // sharded: every rank's bitmap
};

#if defined(__HIPCC__)
// Rounds in which one lane ORs, for every lane of the wave that still has a bit to set in the
// same word, the combined mask; a lane left after them sets its own bit.
constexpr int kMarkPeel = 4;
// Sets bit `m` of bits[wi] for every lane with `need` (k_kld_mark, k_traj_level).  Called by whole
// waves.  The word is read first: the bitmap only ever gains bits, so a set bit read here is set
// for good and needs no atomic, and a stale clear one only costs the atomic.  A plain load: through
// the CU's L1 it was as fast as a device-scope load on a converged cloud and faster on a spread
// one.  One atomic per lane without the read took 43 ms on a converged cloud of 4M particles.
__device__ __forceinline__ void mark_bits_wave(uint64_t* bits, bool need, uint64_t wi, uint64_t m)
{
    if (need && (bits[wi] & m)) need = false;
    const uint32_t lane = threadIdx.x & 63u;
    for (int round = 0; round < kMarkPeel; ++round) {
        const unsigned long long act = __ballot(need);
        if (!act) return;
        const uint32_t leader = (uint32_t)__ffsll((long long)act) - 1u;
        const uint64_t lw = __shfl(wi, (int)leader, 64);
        const bool mine = need && wi == lw;
        uint64_t c = mine ? m : 0;
        for (int o = 32; o >= 1; o >>= 1) c |= __shfl_xor(c, o, 64);
        if (lane == leader) atomicOr((unsigned long long*)&bits[lw], (unsigned long long)c);
        if (mine) need = false;
    }
    if (need) atomicOr((unsigned long long*)&bits[wi], (unsigned long long)m);
}
#endif

// The trajectory log (eslam_trajectory.hip).  One ring entry's arrays, each with
// room for the log's max_particles: 44 bytes per particle
struct TrajEntry {
    double *x, *y, *z, *yaw, *zs;
    uint32_t* parent;                    // the slot of the particle's ancestor in the previous held entry
};
// a held entry as a query walks it (newest first) with the particles it holds
struct TrajLevel {
    TrajEntry e;
    uint32_t count, pad;
};
// k_traj_trace's output: a lineage's node in one entry
struct TrajNode {
    uint32_t slot, pad;
    double x, y, z, yaw, zs;
};
// a slot outside its entry: a walk that meets one ends there (a sound log holds none)
constexpr uint32_t kTrajNone = 0xffffffffu;

// The log of a sharded filter (eslam_gpu_trajectory_enable_sharded).  Slots are global: rank r
// holds the slots [b[r], b[r + 1]) of an entry recorded under the shard table b.  "Items of entry
// E by global slot" is one exchange (traj_fetch, eslam_host_trajectory.hip) with two kinds of
// item: a 4-byte word (a link) or a node, the slot's five values and its parent.
struct TrajTable {
    uint32_t b[kMaxRanks + 1];
    uint32_t G, me;
};
struct alignas(16) TrajItem {            // 48 bytes: three 16-byte accesses
    double x, y, z, yaw, zs;
    uint32_t parent, pad;
};
// what this rank serves: its part [first, first + count) of the entry (nodes), or of a word array
struct TrajSrc {
    const uint32_t* word;                // word items: word[slot - first]; null for node items
    TrajEntry e;
    uint64_t* bits;                      // the smoothed sweep: the bitmap over this rank's part (bit slot - first), or null
    uint32_t first, count;
};
constexpr int kTrajBucketBlocks = 1024;      // blocks of the bucketing kernels at most (each a contiguous range of requests)
// the bucketing's totals: [0, kMaxRanks) requests per owner, then kMaxRanks + 1 exclusive offsets
constexpr int kTrajTotWords = 2 * kMaxRanks + 1;

}  // namespace eslam_dev
