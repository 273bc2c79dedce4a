// eslam_launch.h -- every entry point the kernel files export to each other and to the host side
// (eslam_ctx.hip and the eslam_host_*.hip files), declared once.  Every .hip file includes it, the defining one too: the
// names have C linkage, so only a declaration the definition sees lets the compiler refuse a
// parameter list that has drifted from what the callers pass.
#pragma once

#include <hip/hip_runtime.h>

#include "eslam_internal.h"

using namespace eslam_dev;

extern "C" {

// ---- eslam_kernels.hip (the kernels of an update: the K1 family, the one-block scan, the weight path)
hipError_t eslam_launch_project_weight(int project, int weight, int maxp, DevState s0, DevState s1, const MapView* map,
                                       const StepParams* p, Ctl* ctl, Shard* shards, const GatherView* gv,
                                       const LocalMaps* store, hipStream_t stream, const ChunkSel* sel, double* bspill);
hipError_t eslam_launch_contact_records(DevState s0, DevState s1, const MapView* map, const StepParams* p, Ctl* ctl,
                                        const DebugRec* d, const LocalMaps* store, hipStream_t stream);
hipError_t eslam_launch_pack_records(DevState s0, DevState s1, const Ctl* ctl, uint64_t first, uint64_t stride, uint64_t count,
                                     uint64_t gbase, const uint32_t* anc, const DebugRec* d, eslam_particle_record* out,
                                     eslam_cpoint* cps, uint32_t max_cp, const uint64_t* slot, const double* remote,
                                     hipStream_t stream);
hipError_t eslam_launch_gather_records(const uint32_t* req, uint64_t nreq, uint64_t gbase, const DebugRec* d, double* items,
                                       hipStream_t stream);
hipError_t eslam_launch_scan_excl(uint32_t* a, uint64_t m, hipStream_t stream);
hipError_t eslam_launch_weight_stats(DevState s0, DevState s1, uint64_t n, uint32_t J, Ctl* ctl, Shard* shards,
                                     hipStream_t stream);
hipError_t eslam_launch_finalize(Shard* recs, int nrec, Ctl* ctl, const FinParams* fp, hipStream_t stream);
hipError_t eslam_launch_normalize_scan(DevState s0, DevState s1, const ScanParams* sp, Ctl* ctl, uint64_t* tile_sum,
                                       uint64_t* total, const FusedFin* ff, hipStream_t stream);
hipError_t eslam_launch_normalize_segments(DevState s0, DevState s1, const ScanParams* sp, Ctl* ctl, uint64_t* tile_pub,
                                           uint32_t* marks, uint32_t* tile_first, const uint32_t* jt, const FusedFin* ff,
                                           hipStream_t stream);
hipError_t eslam_launch_resample_gather(DevState s0, DevState s1, uint64_t n, uint64_t gbase, Ctl* ctl, const GatherView* gv,
                                        uint32_t aux, hipStream_t stream);
hipError_t eslam_launch_commit(Ctl* ctl, hipStream_t stream);
hipError_t eslam_launch_segments_multi(DevState s0, DevState s1, const ScanParams* sp, const PlanParams* pp, Ctl* ctl,
                                       const uint64_t* tile_prefix, uint32_t* marks, uint32_t* tile_first,
                                       const uint64_t* totals, const uint32_t* jt, uint2* range, uint64_t* first_last,
                                       uint64_t* host_out, uint64_t* host_epoch, uint64_t epoch, hipStream_t stream);
hipError_t eslam_launch_pack(DevState s0, DevState s1, Ctl* ctl, const PlanParams* pp, const uint2* range,
                             const uint64_t* first_last, uint64_t nsend, void* send, hipStream_t stream);
hipError_t eslam_launch_expand(const void* recv, uint64_t nrecv, uint64_t W0, uint32_t* marks, uint32_t* row_first,
                               hipStream_t stream);
uint64_t eslam_record_bytes(void);
hipError_t eslam_launch_init_gaussian(DevState s0, uint64_t n, uint64_t gbase, uint64_t seed, uint64_t ev, const double mu[3],
                                      const double sigma[3], double zpos, double zsigma, hipStream_t stream);
hipError_t eslam_launch_best_index(DevState s0, DevState s1, uint64_t n, Ctl* ctl, uint64_t* out2, hipStream_t stream);
hipError_t eslam_launch_centroid_chunks(DevState s0, DevState s1, uint64_t n, uint32_t J, Ctl* ctl, double* chunk_out,
                                        hipStream_t stream);
hipError_t eslam_launch_centroid_tree(double* a, double* b, uint64_t m, double* out, hipStream_t stream);
hipError_t eslam_launch_centroid(DevState s0, DevState s1, uint64_t n, uint32_t J, Ctl* ctl, double* tmp, double* out,
                                 hipStream_t stream);

// ---- eslam_particle_maps.hip (per-particle maps: the stores, the page budget, plan / match / merge, the migrating maps)
hipError_t eslam_launch_store_init(uint32_t* sid, const LocalMaps* lm, uint64_t n, uint64_t pool, hipStream_t stream);
hipError_t eslam_launch_store_refs(SidRef sid, uint64_t n, uint64_t pool, const CowScratch* cs, const GatherView* gv,
                                   uint32_t* tgen, hipStream_t stream);
hipError_t eslam_launch_map_plan(DevState s0, DevState s1, Ctl* ctl, const MapView* map, const LocalMaps* lm,
                                 const MergeParams* mp, uint32_t* pgc, hipStream_t stream);
hipError_t eslam_launch_map_match(DevState s0, DevState s1, const Ctl* ctl, const MapView* map, const LocalMaps* lm,
                                  const MatchParams* mp, hipStream_t stream);
hipError_t eslam_launch_map_merge(DevState s0, DevState s1, Ctl* ctl, const MapView* map, const LocalMaps* lm,
                                  const MergeParams* mp, hipStream_t stream);
hipError_t eslam_launch_store_receive(SidRef sid, Ctl* ctl, const LocalMaps* lm, const MergeParams* mp, uint64_t n,
                                      const CowScratch* cs, const void* hdr, uint64_t nrecv, uint32_t* hoff, uint32_t* head,
                                      const void* pay, uint32_t* pgc, hipStream_t stream);
hipError_t eslam_launch_pay_hdr(DevState s0, DevState s1, const Ctl* ctl, const void* send, uint64_t nsend, uint64_t gbase,
                                const LocalMaps* lm, const PaySeg* seg, void* hdr, uint32_t* off, hipStream_t stream);
hipError_t eslam_launch_pay_pack(DevState s0, DevState s1, const Ctl* ctl, const void* send, uint64_t nsend, uint64_t gbase,
                                 const LocalMaps* lm, const void* hdr, const uint32_t* off, void* pay, hipStream_t stream);

// ---- eslam_selftest.hip
hipError_t eslam_launch_selftest_math(int fn, const double* x, const double* y, double* out, uint64_t n, hipStream_t stream);
hipError_t eslam_launch_selftest_bm_radius(unsigned long long* bad, hipStream_t stream);

// ---- eslam_gmm.hip (the pose distribution's Gaussian mixture: pass B, a pass' chunk records, the tree)
hipError_t eslam_launch_gmm_bounds(DevState s0, DevState s1, uint64_t n, Ctl* ctl, uint64_t* part, uint64_t* out,
                                   hipStream_t stream);
hipError_t eslam_launch_gmm_pass(int K, int hard, DevState s0, DevState s1, uint64_t n, uint32_t J, Ctl* ctl, const GmmPass* P,
                                 double* chunk_out, hipStream_t stream);
hipError_t eslam_launch_gmm_tree(double* a, double* b, uint64_t m, uint32_t R, double* out, hipStream_t stream);

// ---- eslam_moments.hip (the pose estimate's moments: pass B, a pass' chunk records; the tree is eslam_launch_gmm_tree)
hipError_t eslam_launch_moments_bounds(DevState s0, DevState s1, uint64_t n, Ctl* ctl, const MomPass* P, uint64_t* part,
                                       uint64_t* out, hipStream_t stream);
hipError_t eslam_launch_moments_pass(int pass, DevState s0, DevState s1, uint64_t n, uint32_t J, Ctl* ctl, const MomPass* P,
                                     double* chunk_out, hipStream_t stream);

// ---- eslam_kld.hip (KLD-sampling's bin count: the box, the marked bitmap, its population count)
hipError_t eslam_launch_kld_bounds(DevState s0, DevState s1, uint64_t n, const Ctl* ctl, double inv, uint32_t theta_bins,
                                   int64_t* part, int64_t* out, hipStream_t stream);
hipError_t eslam_launch_kld_mark(DevState s0, DevState s1, uint64_t n, const Ctl* ctl, const KldGrid* g, uint64_t* bits,
                                 uint64_t words, hipStream_t stream);
hipError_t eslam_launch_kld_or(const uint64_t* all, uint32_t G, uint64_t words, uint64_t* bits, hipStream_t stream);
hipError_t eslam_launch_kld_popcount(const uint64_t* bits, uint64_t words, int64_t* part, int64_t* out, hipStream_t stream);

// ---- eslam_trajectory.hip (the trajectory log: the record, the link's composition, the two queries)
hipError_t eslam_launch_traj_iota(uint32_t* link, uint64_t n, hipStream_t stream);
hipError_t eslam_launch_traj_record(DevState s0, DevState s1, const Ctl* ctl, uint64_t n, int updated, const uint32_t* anc,
                                    const uint32_t* link, uint64_t nlink, uint32_t* link_next, const TrajEntry* e,
                                    hipStream_t stream);
hipError_t eslam_launch_traj_compose(const uint32_t* anc, const uint32_t* link, uint64_t nlink, uint32_t* link_next, uint64_t n,
                                     hipStream_t stream);
hipError_t eslam_launch_traj_trace(const uint32_t* leaf, uint64_t count, const uint32_t* link, uint64_t nlink, const TrajLevel* lv,
                                   uint32_t steps, TrajNode* out, hipStream_t stream);
hipError_t eslam_launch_traj_level(uint64_t n, const TrajLevel* L, uint32_t* a, DevState out, uint64_t* bits, hipStream_t stream);
// ... on a sharded filter: the exchange's kernels (bucket, serve, scatter) and its users'
hipError_t eslam_launch_traj_iota_from(uint32_t* link, uint64_t n, uint32_t first, hipStream_t stream);
void eslam_traj_bucket_shape(uint64_t count, uint32_t* nblocks, uint64_t* per);
hipError_t eslam_launch_traj_bucket(const uint32_t* slots, uint64_t count, const TrajTable* T, uint32_t* cnt, uint32_t* tot,
                                    uint32_t* req, uint32_t* pos, hipStream_t stream);
hipError_t eslam_launch_traj_serve(int node, const uint32_t* slots, uint64_t n, int own_only, const TrajTable* T, const TrajSrc* src,
                                   void* out, hipStream_t stream);
hipError_t eslam_launch_traj_scatter(int node, const void* in, const uint32_t* pos, uint64_t n, void* out, hipStream_t stream);
hipError_t eslam_launch_traj_sources(const Ctl* ctl, int updated, const uint32_t* anc, uint32_t first, uint64_t n, uint32_t* out,
                                     hipStream_t stream);
hipError_t eslam_launch_traj_record_sharded(DevState s0, DevState s1, const Ctl* ctl, uint64_t n, int updated, const uint32_t* anc,
                                            const uint32_t* pre, uint32_t first, uint32_t* link_next, const TrajEntry* e,
                                            hipStream_t stream);
hipError_t eslam_launch_traj_trace_take(const TrajItem* items, uint64_t count, uint32_t gcount, uint32_t* a, uint32_t steps, uint32_t j,
                                        TrajNode* out, hipStream_t stream);
hipError_t eslam_launch_traj_level_take(const TrajItem* items, uint64_t n, uint32_t* a, DevState out, hipStream_t stream);

// ---- eslam_resample.hip (resample to a count: the cumulative sum, the draws' searches, the gather)
uint64_t eslam_resample_tiles(uint64_t items);
hipError_t eslam_launch_rs_cumsum(DevState s0, DevState s1, uint64_t n, Ctl* ctl, uint32_t jump_samples, uint64_t* coarse,
                                  uint64_t* C, uint64_t* counter, hipStream_t stream);
hipError_t eslam_launch_rs_draw(int multinomial, uint64_t n, uint64_t samples, const Ctl* ctl, const uint32_t* jt,
                                const uint64_t* coarse, const uint64_t* C, uint32_t* anc, uint32_t* kept, uint64_t* counter,
                                hipStream_t stream);
hipError_t eslam_launch_rs_compact(uint64_t samples, const uint32_t* anc, const uint32_t* offs, uint32_t* out, hipStream_t stream);
hipError_t eslam_launch_rs_gather(DevState s0, DevState s1, const Ctl* ctl, DevState out, uint64_t m, const uint32_t* anc,
                                  int set_weight, double weight, uint32_t* anc_out, hipStream_t stream);
// ... on a sharded filter: C over the rank's shard, the draws routed by the all-gathered totals
hipError_t eslam_launch_rss_cumsum(DevState s0, DevState s1, uint64_t n, Ctl* ctl, uint64_t* coarse, uint64_t* C,
                                   uint64_t* counter, hipStream_t stream);
hipError_t eslam_launch_rss_census(const RsPlan* pl, const Ctl* ctl, const uint32_t* jt, uint32_t* kept, uint64_t* counter,
                                   hipStream_t stream);
hipError_t eslam_launch_rss_route(int multinomial, int fill, const RsPlan* pl, DevState s0, DevState s1, DevState out,
                                  const Ctl* ctl, const uint32_t* jt, const uint64_t* coarse, const uint64_t* C,
                                  const uint32_t* offs, void* send, uint32_t* anc_out, uint64_t* counter, hipStream_t stream);
hipError_t eslam_launch_rss_expand(const void* recv, uint64_t nrecv, DevState out, uint64_t n_out, uint32_t* anc_out,
                                   hipStream_t stream);

// ---- eslam_hash.hip
hipError_t eslam_launch_hash_sweep(const dm_hash_grid* g, const double* pts, const double* orient, uint32_t steps, int32_t* out,
                                   hipStream_t stream);
hipError_t eslam_launch_hash_poses(const dm_hash_grid* g, const double* pts, const double* orient, const uint64_t* ids,
                                   uint64_t count, double* hx, double* hy, double* hth, double* hz, hipStream_t stream);
hipError_t eslam_launch_init_from_hash(DevState s0, const uint32_t* idx, uint64_t n, const double* hx, const double* hy,
                                       const double* hth, const double* hz, hipStream_t stream);
hipError_t eslam_radix_sort_pairs_passes(uint32_t* keys, uint32_t* vals, uint32_t* keys_out, uint32_t* order, uint64_t n,
                                         void* tmp, size_t* tmp_bytes, int passes, hipStream_t stream);
hipError_t eslam_radix_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* keys_out, uint32_t* order, uint64_t n, void* tmp,
                                  size_t* tmp_bytes, hipStream_t stream);
hipError_t eslam_hash_sort(DevState s0, DevState s1, const Ctl* ctl, uint64_t n, uint32_t* keys, uint32_t* vals,
                           uint32_t* keys_out, uint32_t* order, void* tmp, size_t* tmp_bytes, hipStream_t stream);
hipError_t eslam_launch_hash_replace(DevState s0, DevState s1, const Ctl* ctl, const uint32_t* order, const uint32_t* draws,
                                     uint64_t k, const uint32_t* blist, uint32_t bstart, const double* hx, const double* hy,
                                     const double* hth, const double* hz, double weight, hipStream_t stream);
hipError_t eslam_launch_hash_candidates(const uint32_t* keys, const uint32_t* order, uint64_t cnt, uint64_t gbase, int nranks,
                                        void* send, hipStream_t stream);
hipError_t eslam_launch_hash_unpack(const void* recv, uint64_t m, uint32_t* keys, uint32_t* vals, hipStream_t stream);
hipError_t eslam_launch_hash_replace_global(DevState s0, DevState s1, const Ctl* ctl, const uint32_t* gorder,
                                            const uint32_t* draws, uint64_t k, uint64_t gbase, uint64_t n, const uint32_t* blist,
                                            uint32_t bstart, const double* hx, const double* hy, const double* hth,
                                            const double* hz, double weight, hipStream_t stream);

// ---- eslam_shared_map.hip
size_t eslam_sm_sort_bytes(uint64_t records);
hipError_t eslam_launch_sm_stage(DevState s0, DevState s1, const Ctl* ctl, uint64_t first, uint64_t cnt, uint32_t copies,
                                 double* out, hipStream_t stream);
hipError_t eslam_launch_sm_place(DevState s0, DevState s1, const Ctl* ctl, const MapView* map, const SmRun* run,
                                 const SmScratch* s, hipStream_t stream);
hipError_t eslam_launch_sm_merge(DevState s0, DevState s1, const Ctl* ctl, const SmRun* run, const SmGrid* cur,
                                 const SmGrid* next, const SmScratch* s, hipStream_t stream);

// ---- eslam_particle_grid.hip
// the scratch of a composition on a width x height grid: its size, and its arrays within `mem` (may be null: size only)
size_t eslam_pgrid_work_bytes(uint32_t width, uint32_t height, void* mem, PgScratch* s);
hipError_t eslam_launch_pgrid_count(const LocalMaps* lm, const uint32_t* sidp, const MapView* map, const PgScratch* s,
                                    hipStream_t stream);
hipError_t eslam_launch_pgrid_fill(const LocalMaps* lm, const MapView* map, const PgScratch* s, const SmGrid* cur,
                                   const SmGrid* out, hipStream_t stream);

// ---- eslam_scan.hip
// the scratch of a build of n points: its size, and its arrays within `mem` (may be null: size only)
size_t eslam_scan_work_bytes(uint64_t n, void* mem, ScanWork* w);
hipError_t eslam_launch_scan_order(const dm_scan_frame* f, const ScanReading* rd, const ScanWork* w, hipStream_t stream);
hipError_t eslam_launch_scan_count(const dm_scan_frame* f, const ScanWork* w, uint32_t nheads, uint32_t nbinned,
                                   hipStream_t stream);
hipError_t eslam_launch_scan_emit(const dm_scan_frame* f, const ScanWork* w, uint32_t nheads, uint32_t nbinned,
                                  eslam_scan_patch* out, hipStream_t stream);

// ---- eslam_snapshot.hip
hipError_t eslam_launch_snap_census_tables(const LocalMaps* lm, const SnapCensus* c, const uint32_t* sid, uint64_t n,
                                           hipStream_t stream);
hipError_t eslam_launch_snap_census_pages(const LocalMaps* lm, const SnapCensus* c, uint64_t T, hipStream_t stream);
hipError_t eslam_launch_snap_pack(int what, const LocalMaps* lm, const SnapCensus* c, const uint32_t* sid, uint64_t T,
                                  uint32_t tbase, uint32_t pbase, uint64_t k0, uint64_t cnt, uint32_t rw, void* out,
                                  hipStream_t stream);
hipError_t eslam_launch_snap_unpack(int what, const LocalMaps* lm, uint64_t k0, uint64_t cnt, uint32_t rw, const void* in,
                                    hipStream_t stream);
hipError_t eslam_launch_snap_finish(const LocalMaps* lm, uint64_t T, uint64_t P, hipStream_t stream);
hipError_t eslam_launch_snap_mark_ids(const uint32_t* ids, uint64_t n, uint32_t* bits, uint64_t limit, hipStream_t stream);
hipError_t eslam_launch_snap_mark_rows(const LocalMaps* lm, uint64_t T, uint32_t* bits, uint64_t limit, hipStream_t stream);
hipError_t eslam_launch_snap_rank_bits(const uint32_t* bits, uint64_t words, uint32_t* pre, hipStream_t stream);
hipError_t eslam_launch_snap_rank_sid(uint32_t* sid, uint64_t n, const SnapSubset* s, hipStream_t stream);
hipError_t eslam_launch_snap_renumber_tables(const LocalMaps* lm, uint64_t T, const SnapSubset* s, hipStream_t stream);
hipError_t eslam_launch_snap_unpack_owner_subset(const LocalMaps* lm, uint64_t k0, uint64_t cnt, const SnapSubset* s, const void* in,
                                                 hipStream_t stream);

}  // extern "C"
