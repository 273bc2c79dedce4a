// eslam_ctx.h -- host-only: the context behind the C ABI of include/eslam_gpu.h, and the helpers
// that more than one host file uses (namespace eslam_host).  Included by the host files:
// eslam_ctx.hip (lifecycle, particles, the step, the resamplers), eslam_host_map.hip (the maps and
// the scan build), eslam_host_stats.hip (centroid, mixture, moments, KLD), eslam_host_trajectory.hip
// (the trajectory log and its queries), eslam_host_snapshot.hip (save and load) and
// eslam_host_comm.hip (the multi-GPU plumbing).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <string>
#include <vector>

#include "eslam_internal.h"
#include "eslam_launch.h"
#include "eslam_buf.h"

using namespace eslam_dev;
using namespace eslam_buf;

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
// ESLAM_FLAG_PROCESS_STATICS: the reference's function-static hash-respawn counter
// (src/PoseEstimator.cpp:239) and the C library's rand() (SurfaceHash::sample), shared by every
// context of the process that sets the flag -- Q11.  Not locked, like the reference's statics.
struct ProcessStatics {
    uint64_t hash_event = 0;
    dm_libc_rand_state libc;
    ProcessStatics() { dm_libc_srand(&libc, 1); }
};

// The owners of the context's device and pinned memory, grouped by what drops them together:
// assigning an empty group over one frees its buffers (free_particles, free_local_maps,
// free_debug, free_map).  The structs kernels take by value are filled from these.
struct ParticleBufs {                        // alloc_particles
    Dev<void> state_mem;
    Dev<uint32_t> marks, anc;
    Dev<uint32_t> tile_first;                // row_first: source of every 64-output row's first output
    Dev<uint64_t> tile_sum;                  // per scan tile: exact fixed-point weight total (sharded K3a), or
                                             // one GPU: tag << 61 | total published by K3 (zeroed at allocation)
    Dev<uint2> range;                        // per particle: [lo, hi) of its global outputs
    Dev<uint32_t> sid_mem;                   // 2 x cap: DevState::sid of both state buffers
    Dev<uint32_t> cow;                       // owner, counts, free and sharing lists + the copy count
    Dev<uint64_t> merge_cnt;                 // the map merge's statistics slots (2 x kMergeCounterSlots) and
                                             // the copy-on-write copies since the last merge
};
struct LocalMapBufs {                        // local_maps_reset
    Dev<int2> ctr;                           // the arrays of LocalMaps
    Dev<float2> page;
    Dev<uint64_t> owner;
    Dev<uint32_t> slot, tgen, frees;
    Dev<uint8_t> mark;
    Dev<uint32_t> off;                       // per particle: its first page in its plan block (MergeParams::off)
    Dev<MergeJob> job;                       // per particle: the plan's record (MergeParams::job)
    Dev<uint16_t> codes;                     // per particle: the plan's cell codes (MergeParams::codes): a small
                                             //   part's stride, grown for a large part's
    Dev<uint32_t> poff;                      // per merge block: page offsets (+ total)
    Dev<uint32_t> pgc;                       // the page collection's compaction counts
    Dev<ScanPatch> match_sp;                 // processMap match: the sampled scan patches
    Dev<void> census;                        // a snapshot's census: first, trank, tlist, firstref, prank, plist
    Dev<uint32_t> counts;                    // the census' tile counts
};
struct DebugBufs {                           // the arrays of DebugRec
    Dev<double> meas, cp;
    Dev<uint8_t> ncp;
    Dev<uint32_t> resampled;
};
struct GridBufs {                            // the shared grid's arrays (MapView, SmGrid)
    Dev<uint32_t> cells, occ;
    Dev<float2> patch;
    Dev<float> height;                       // empty: all horizontal
    Dev<uint4> cell_tab;
    SmGrid view() const { return SmGrid{cells, patch, height, occ, cell_tab}; }
};

// The trajectory log (eslam_gpu_trajectory_enable): a ring of `capacity` entries of
// max_particles particles each, 44 bytes per particle (x, y, z, yaw, zsigma as fp64 and the uint32
// parent: 185 MB per entry at 4M particles), and the two link buffers, all one block allocated at
// enable.  What the host keeps per entry is its particle count and its step id.
struct TrajectoryLog {
    bool on = false;
    uint32_t capacity = 0;
    uint64_t max_particles = 0;
    Dev<void> mem;
    uint64_t bytes = 0;
    std::vector<TrajEntry> entry;            // the ring entries' arrays within mem
    std::vector<uint32_t> count;             // per ring entry: the particles it holds
    std::vector<uint64_t> step;              // ... and its step id
    uint32_t* link[2] = {};                  // link[cur][i]: current particle i's ancestor's slot in the newest entry
    uint32_t cur = 0;
    uint64_t link_n = 0;                     // entries of link[cur]: the filter's count at the last record or composition
    uint32_t head = 0, held = 0;             // the ring entry the next record writes, the entries held
    uint64_t next_step = 0;                  // records since enable: the next entry's step id
    Dev<char> scratch;                       // the queries' scratch, kept between calls
    // The log of a sharded filter (eslam_gpu_trajectory_enable_sharded): max_particles, count and
    // link_n are this rank's, parent and link hold global slots.  Identical on every rank:
    bool sharded = false;
    std::vector<uint64_t> gcount;            // per ring entry: its global count
    std::vector<std::vector<uint64_t>> table;   // ... and the shard table it was recorded under (nranks + 1 bounds)
    std::vector<uint64_t> link_table;        // the table link[cur] is indexed under: the filter's at the last record or composition
    std::vector<uint64_t> max_all;           // every rank's max_particles
    bool link_identity = false;              // link[cur][i] == first + i: set by a record, cleared by a composition
    Dev<char> xa, xb;                        // the exchange's scratch: by the requests made; by those received and answered
    // the ring index of the j-th newest held entry (j < held)
    uint32_t at(uint32_t j) const { return (head + capacity - 1u - j) % capacity; }
};

struct eslam_ctx {
    eslam_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;            // destroyed (if owned) after every member below is gone
    bool own_stream = false;
    // particles
    uint64_t n = 0, cap = 0;
    uint64_t gbase = 0, n_global = 0;
    DevState st[2] = {};
    ParticleBufs pt;
    uint64_t* fin_word = nullptr;           // the fused finalize's epoch word (after the tile words)
    uint32_t pub_stride = 0;                // ScanParams::pub_stride
    uint64_t fin_epoch = 0;                 // fused finalize launches so far
    uint32_t scan_tag = 0;                  // the last K3 launch's tag (1..7)
    bool has_anc = false;
    // per-particle maps (ESLAM_FLAG_PARTICLE_MAPS): the tables, pages and the copy-on-write scratch
    LocalMaps lm = {};
    LocalMapBufs lmb;
    bool lm_ready = false;                   // lm sized for the current map and particle count
    // the scan of a map update on the device (MergeParams::sp): two slots, each staged through
    // pinned host memory; an update waits for the update before last to have read its slot
    Pinned<ScanPatch> scan_host[2];
    Dev<ScanPatch> scan_dev[2];
    Event scan_ev[2];
    uint32_t scan_slot = 0;
    // logDebug records of the last update (ESLAM_FLAG_RECORD_CONTACTS / log_debug)
    DebugRec dbg = {};
    DebugBufs dbgb;
    uint64_t dbg_cap = 0;
    bool dbg_valid = false;
    // statistics and control
    Dev<Shard> shards;
    Dev<Ctl> ctl;
    Pinned<Ctl> ctl_host;
    Pinned<uint32_t> fault_host;            // host-mapped: kFaultTimeout when a device wait gave up
    bool poisoned = false;                  // the particle set is undefined until re-initialised
    bool poison_pages = false;              // ... because the map pages ran out (kFaultPages)
    uint32_t spin_limit = kSpinLimit;       // polls of K3's cross-block waits (debug: 0 gives up at once)
    uint32_t debug_scan_items = 0;          // particles per thread of the one-GPU K3 (debug; 0: scan_items(n))
    Dev<uint32_t> jump;
    uint32_t jump_n = 1;                    // A^n_global, cached
    uint64_t jump_n_for = 0;
    Dev<double> scratch;                    // small device scratch (centroid, best index)
    Pinned<double> scratch_host;
    // map
    bool has_map = false;
    MapView map = {};
    GridBufs grid;
    uint64_t map_np = 0;                     // patches of the grid (cell_start[width * height])
    uint64_t map_np_cap = 0;                 // patches grid.patch / grid.height have room for
    // eslam_gpu_shared_map_update's scratch (SmScratch): one allocation, kept between calls
    Dev<void> sm_mem;
    // eslam_gpu_shared_map_update_sharded's exchange memory, kept between calls: a run's staged
    // pose records (one copy per rank), then the gathered run, at most (nranks + 1) x run
    // particles x 40 bytes
    Dev<void> sm_x;
    // eslam_gpu_get_particle_grid / eslam_gpu_adopt_particle_map's scratch (PgScratch), kept between calls
    Dev<void> pg_mem;
    // ... and the arrays the last export composed into, kept for the next one (room for pg_out_cap
    // patches on a grid of pg_out_cells cells; dropped with the map, handed over by an adoption)
    GridBufs pg_out;
    uint64_t pg_out_cap = 0, pg_out_cells = 0;
    // eslam_gpu_scan_from_laser / _depth: the build's scratch (ScanWork) and the last
    // built scan's patches (capacity in patches), both kept between calls
    Dev<void> scan_mem;
    Dev<eslam_scan_patch> scan_out;
    uint64_t scan_count = 0;                 // patches of the last built scan
    // eslam_gpu_save / eslam_gpu_load: two pinned and two device staging slots of
    // snap_cap bytes with their events (the census scratch is dropped with the local maps)
    Pinned<void> snap_host[2];
    Dev<void> snap_dev[2];
    uint64_t snap_cap = 0;
    Event snap_ev[2];
    uint32_t maxp = 4;
    // host-side filter state
    uint64_t proj_event = 0, init_event = 0, hash_event = 0;
    double ud_pose[12];
    double zcomp[4] = {1, 0, 0, 0};
    // multi-GPU (eslam_gpu_set_comm): this context is shard [gbase, gbase + n) of n_global
    bool sharded = false;
    bool statics_sharded = false;            // counted in g_statics_sharded
    eslam_comm comm = {};
    std::vector<uint64_t> gall;             // first global index of every rank (+ n_global)
    Dev<Shard> recs;                        // gathered records of all ranks
    Dev<uint64_t> mg;                       // MgBlock (device)
    void* rccl = nullptr;                   // ncclComm_t of eslam_gpu_set_comm_rccl (owned)
    Pinned<uint64_t> mg_host;               // host-mapped (k_segments_multi writes the totals there)
    uint64_t seg_epoch = 0;                 // the last k_segments_multi launch's epoch (mg_host[kHostEpoch])
    Dev<void> sendbuf, recvbuf;
    // per-particle maps on a sharded filter: the migrated particles' maps (a MapPayHdr per
    // record, then their pages as MapPayPage, in the records' order) and whether their tables
    // are still owed to them
    Dev<void> sendpay, recvpay, sendhdr, recvhdr;
    Dev<uint32_t> payoff;                    // header prefix (send side, then receive side)
    Dev<uint32_t> rhead;                     // received records: the record carrying each one's map
    uint64_t nrecv_maps = 0;                 // records whose maps wait in recvhdr / recvpay
    Dev<double> cent;                        // getCentroid's chunk records (sharded: sized by set_comm)
    Dev<double> gmm;                         // eslam_gpu_fit_pose_gmm's words, chunk records and exchange, grown on demand
    Dev<double> moments;                     // eslam_gpu_pose_moments' words, chunk records and exchange (gmm's layout), grown on demand
    Dev<char> kld;                           // eslam_gpu_kld_count's scratch (KldScratch: records, bitmap, the ranks'
                                             //   bitmaps), kept between calls
    Dev<double> bspill;                      // K1's parked per-bucket sums (k1_bspill_bytes)
    bool cow_pending = false;
    // a sharded update's exchange left for the next call: the segments kernel's
    // epoch and plan; the next step runs its own-output chunks before it completes it
    bool xpend = false;
    uint64_t xpend_epoch = 0;
    PlanParams xpend_pp = {};
    hipStream_t xstream = nullptr;           // the deferred exchange's stream (overlaps the own chunks)
    Event ev_seg;                            // recorded after the segments kernel
    Event ev_x;                              // recorded after the exchange's expand
    Pinned<void> stage;                      // pinned staging (host-memory comm)
    Dev<char> hostx;                         // host_allgather's words (device-memory comm), sized by set_comm
    // SurfaceHash (useHash)
    double map_scale[2] = {1, 1};
    bool has_hash = false;
    uint64_t hash_n = 0;
    Dev<double> d_hash;                      // 4 x hash_n: x, y, theta, z
    Dev<uint32_t> d_hash_blist;              // pose indices grouped by bucket, sweep order
    std::vector<uint32_t> hash_bstart;       // bins^2 + 1
    std::vector<int32_t> hash_bucket;        // per pose (sweep order)
    dm_libc_rand_state libc;                 // rand() of SurfaceHash::sample (glibc, seed 1)
    // the hash-respawn counter and rand() in use: this context's own, or the process's
    // (ESLAM_FLAG_PROCESS_STATICS: the reference's function statics, Q11)
    uint64_t* hash_ev = nullptr;
    dm_libc_rand_state* libcp = nullptr;
    Dev<void> hsend, hrecv, hsort;           // sharded respawn: candidate pairs out / in; their sort's arrays + scratch
    Dev<uint32_t> d_sort;                    // keys, vals, keys_out, order (4 x sort_cap)
    uint64_t sort_cap = 0;
    Dev<void> sort_tmp;
    size_t sort_tmp_bytes = 0;
    Dev<uint32_t> d_draws;
    // eslam_gpu_resample_stratified / _multinomial to another count: the cumulative sum, its
    // coarse level, the draws' ancestors and the compaction's counts (resample_to), kept between calls
    Dev<char> rs_mem;
    TrajectoryLog traj;
    // diagnostics
    std::string err;
    bool timing = false;
    Event ev[5];                            // events of the step being recorded
    EventRing ring{5, 4};                   // 5 events per recorded step (timing mode)
    EventRing mring{5, 4};                  // 5 events per recorded map update (timing mode)
    EventRing xring{2, 1};                  // 2 events per recorded map match (timing mode)
    eslam_kernel_times times = {};
};

#define HIPCHK(ctx, expr)                                                                    \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
            return ESLAM_ERR_HIP;                                                            \
        }                                                                                    \
    } while (0)

// multi-GPU scratch block (uint64 words, device + pinned host mirror)
namespace mg {
constexpr int kTotal = 0;                                   // this rank's fixed-point weight total
constexpr int kTotals = kTotal + 1;                         // [kMaxRanks] gathered totals
constexpr int kMirror = kTotals + kMaxRanks;                // [3] resample, minstd_start, scan_shift (k_finalize)
constexpr int kCounts = kMirror + 3;                        // [kMaxRanks] records sent to each rank
constexpr int kCountsAll = kCounts + kMaxRanks;             // [kMaxRanks^2] gathered counts
constexpr int kSendOff = kCountsAll + kMaxRanks * kMaxRanks;   // [kMaxRanks + 1]
constexpr int kSdEd = kSendOff + kMaxRanks + 1;             // [2 kMaxRanks]
constexpr int kFirstLast = kSdEd + 2 * kMaxRanks;           // [2 kMaxRanks]
constexpr int kBest = kFirstLast + 2 * kMaxRanks;           // [2] local best (key, global index)
constexpr int kBestAll = kBest + 2;                         // [2 kMaxRanks]
constexpr int kMaxW = kBestAll + 2 * kMaxRanks;             // local max weight (bits)
constexpr int kMaxWAll = kMaxW + 1;                         // [kMaxRanks]
constexpr int kHostEpoch = kMaxWAll + kMaxRanks;           // (mg_host only) the segments kernel's epoch
constexpr int kChunks = kHostEpoch + 1;                     // [2] own-output chunks of the slice (PlanParams::chunk_sel)
constexpr int kWords = kChunks + 2;
}  // namespace mg

// The helpers that cross the host files.  In a namespace: with external linkage they are dynamic
// symbols of the library, and a global `fail` or `grow` could be interposed by the application.
namespace eslam_host {

inline int fail(eslam_ctx* ctx, int code, const char* msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

// a buffer of at least `bytes`, contents not kept (Buf::grow: the old block is freed first)
template <typename B>
int grow(eslam_ctx* ctx, B& buf, uint64_t bytes)
{
    HIPCHK(ctx, buf.grow(bytes, ctx->stream));
    return ESLAM_OK;
}

inline bool particle_maps(const eslam_ctx* ctx) { return (ctx->cfg.flags & ESLAM_FLAG_PARTICLE_MAPS) != 0; }

inline const LocalMaps* store_of(const eslam_ctx* ctx) { return particle_maps(ctx) ? &ctx->lm : nullptr; }

// ---- eslam_ctx.hip
extern std::atomic<int> g_statics_sharded;
int settle(eslam_ctx* ctx);              // completes a deferred sharded exchange (run_update_tail_multi)
void free_particles(eslam_ctx* ctx);
void q_to_mat(const double q[4], double R[9]);
void q_mul(const double a[4], const double b[4], double r[4]);
void q_from_yaw(double angle, double q[4]);
void remove_yaw(const double q[4], double out[4]);
int check_poisoned(eslam_ctx* ctx);
int read_ctl(eslam_ctx* ctx);
int write_ctl(eslam_ctx* ctx);
int alloc_particles(eslam_ctx* ctx, uint64_t n);
int local_maps_reset(eslam_ctx* ctx);
int reset_ctl_for_new_particles(eslam_ctx* ctx, int wexp);
const double* hash_field(eslam_ctx* ctx, int f);
MergeParams merge_params(eslam_ctx* ctx, const CowScratch& cs);
GatherView gather_view(eslam_ctx* ctx);
int materialize(eslam_ctx* ctx);
int resample_to(eslam_ctx* ctx, uint64_t samples, bool multi, eslam_resample_info* info);
int resample_sharded(eslam_ctx* ctx, uint64_t samples, bool multi, eslam_resample_info* info);

// ---- eslam_host_stats.hip
// the ungated or gated pose moments (eslam_gpu_pose_moments' passes) of the context's n particles
// read from the state pair s0 / s1; rc: what preparing them returned (a sharded filter agrees on it)
int pose_moments_of(eslam_ctx* ctx, DevState s0, DevState s1, MomPass& P, int rc, eslam_pose_moments* out);

// ---- eslam_host_trajectory.hip (the callers test ctx->traj.on first)
// the end of a step or an update: materialises a pending gather, then records the particles as
// they stand; `updated`: an update ran, whose resample decision the device reads
int trajectory_record(eslam_ctx* ctx, bool updated);
// after a resample outside the step has written pt.anc for the filter's n outputs: link' = link o anc
int trajectory_compose(eslam_ctx* ctx);
// a new particle set: the log is emptied, the link the identity over the filter's n
int trajectory_reset(eslam_ctx* ctx);
// a sharded filter about to be resampled to the shard table nb[0 .. nranks]: false where the log
// of some rank (eslam_gpu_trajectory_enable_sharded) has no room for its new shard; the same on every rank
bool trajectory_holds(const eslam_ctx* ctx, const uint64_t* nb);

// ---- eslam_host_comm.hip
int comm_allgather(eslam_ctx* ctx, const void* dsend, void* drecv, uint64_t bytes);
int comm_alltoallv(eslam_ctx* ctx, const void* dsend, const uint64_t* sb, void* drecv, const uint64_t* rb,
                   hipStream_t stream = nullptr);
// all_gather of `bytes` per rank between host arrays, whichever kind of callback the user gave
// (device-memory callbacks: through ctx->hostx, which eslam_gpu_set_comm sizes for kHostXBytes per
// rank).  Every caller carries a static_assert that its words fit: host-memory callbacks do not
// pass through the buffer, so only that assert catches a caller that outgrows it.
constexpr uint64_t kHostXBytes = 6 * 8;   // the largest user: the snapshot plan's six words (snap_plan)
int host_allgather(eslam_ctx* ctx, const void* send, void* recv, uint64_t bytes);
// the check that the ranks of a collective call were given the same parameters: gathers `nwords`
// words of every rank and fails with ESLAM_ERR_INVALID_ARG and `msg` where a rank's differ from `mine`
int same_on_every_rank(eslam_ctx* ctx, const uint64_t* mine, uint32_t nwords, const char* msg);
// `rc` itself on an unsharded filter.  On a sharded one a collective: ESLAM_OK on a rank means
// every rank passed ESLAM_OK.  A failing rank keeps its own code (and message); the others return
// ESLAM_ERR_COMM with "<what>: rank R failed (C)".
int agree(eslam_ctx* ctx, int rc, const char* what);
// the chunk records of a sum over the particles, one per 64 J particles of every shard in the table
// gall[0..G]: each rank's count (nch, may be null), the largest (at least 1) and their sum
void chunk_shape(const uint64_t* gall, int G, uint32_t J, uint64_t* nch, uint64_t* maxch, uint64_t* total);
// every rank's `mine` (maxch records of R doubles, zero-padded) all-gathered into `all`, then each
// rank's nch[r] records copied to `a` in global chunk order
int gather_chunks(eslam_ctx* ctx, const uint64_t* nch, uint64_t maxch, uint32_t R, const double* mine, double* all, double* a);
uint64_t centroid_bytes(const uint64_t* gall, int G, uint32_t J);
// a shard table's buffers (may fail; nothing else changes), and the table itself (eslam_host_comm.hip)
int reserve_shard_table(eslam_ctx* ctx, int nranks, uint64_t n_global, const uint64_t* shard_gbase);
int apply_shard_table(eslam_ctx* ctx, int nranks, int rank, uint64_t n_global, const uint64_t* shard_gbase);
void rccl_release(eslam_ctx* ctx);

}  // namespace eslam_host

using namespace eslam_host;
