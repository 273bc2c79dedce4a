/*
 * eslam_gpu.h -- C ABI of the MI355X-native eSLAM particle-filter core.
 *
 * Drop-in boundary for the per-step hot path of liyangSKD/slam-eslam:
 *
 *   EmbodiedSlamFilter::update(body2odometry, BodyContactState, ltc)   src/EmbodiedSlamFilter.cpp:353-369
 *     -> PoseEstimator::project                                         src/PoseEstimator.cpp:184-242
 *     -> PoseEstimator::update -> updateWeights                         src/PoseEstimator.cpp:244-352
 *          -> ContactModel::setContactPoints/evaluatePose/evaluateWeight/updateZPositionEstimate
 *                                                                       src/ContactModel.cpp:21-41,117-340
 *          -> GridAccess::get -> MLSMap::getPatch(p, patch, 3.0)        src/PoseEstimator.hpp:97-105
 *     -> ParticleFilter::normalizeWeights / resample_stratified         src/ParticleFilter.hpp:46-108
 *
 * Plain C: POD structs, pointers and sizes, no torch / HIP types in the signatures.  Every
 * entry point returns ESLAM_OK (0) or a negative ESLAM_ERR_* code; eslam_gpu_last_error()
 * gives the message (the reference's std::runtime_error texts where one exists).
 *
 * One context = one GPU (one process per GPU for multi-GPU; see eslam_gpu_set_comm).  A
 * context is not thread-safe.  Device memory is owned by the context; host buffers passed
 * in are owned by the caller and only read/written during the call.
 */
#ifndef ESLAM_GPU_H
#define ESLAM_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESLAM_ABI_VERSION 8

/* maximum number of contact points of one BodyContactState handled per step
 * (asguard: 4 wheels x 5 feet = 20, src/ContactModel.cpp grouping) */
#define ESLAM_MAX_CONTACTS 32

/* ---- status codes -------------------------------------------------------------------- */
#define ESLAM_OK 0
#define ESLAM_ERR_INVALID_ARG -1
#define ESLAM_ERR_NO_ENVIRONMENT -2      /* "No environment attached." src/PoseEstimator.cpp:259-260 */
#define ESLAM_ERR_ZERO_MEAS_VAR -3       /* "using a zero measurement variance leads to singularities" src/ContactModel.cpp:122-123 */
#define ESLAM_ERR_HASH_SAMPLE -4         /* "could not sample from pose hash." src/PoseEstimator.cpp:84 */
#define ESLAM_ERR_NO_MLS_GRID -5         /* "The provided environment does not contain an mls grid." src/EmbodiedSlamFilter.cpp:104 */
#define ESLAM_ERR_HIP -6                 /* HIP runtime failure (message has details) */
#define ESLAM_ERR_NOT_INITIALISED -7     /* no particles yet */
#define ESLAM_ERR_UNSUPPORTED -8
#define ESLAM_ERR_OUT_OF_MEMORY -9
#define ESLAM_ERR_COMM -10               /* a collective callback failed */

/* ---- Configuration (src/Configuration.hpp:12-213, the fields consumed on the path) ---- */
typedef struct eslam_config {
    uint64_t seed;                         /* Configuration::seed (42)                     */
    uint64_t particle_count;               /* Configuration::particleCount (250)           */
    uint64_t min_effective;                /* Configuration::minEffective (50)             */
    double initial_rotation_error[3];      /* (0, 0, 0.1)                                  */
    double initial_translation_error[3];   /* (0.1, 0.1, 1.0)                              */
    double measurement_error;              /* 0.1                                          */
    double discount_factor;                /* 0.9                                          */
    double spread_threshold;               /* 0.9                                          */
    double spread_translation_factor;      /* 0.1                                          */
    double spread_rotation_factor;         /* 0.05                                         */
    double slip_factor;                    /* 0.05                                         */
    double max_yaw_deviation;              /* 15 deg                                       */
    double measurement_threshold_distance; /* UpdateThreshold(0.1, 10 deg).distance       */
    double measurement_threshold_angle;    /*                             .angle           */
    /* ContactModelConfiguration (src/Configuration.hpp:51-81) */
    int32_t use_slip_update;               /* false                                        */
    int32_t use_shape_update;              /* true                                         */
    uint64_t min_contacts;                 /* 3                                            */
    double contact_likelihood_correction;  /* 0.33                                         */
    double contact_point_radius;           /* 0.01                                         */
    /* SurfaceHashConfig (src/Configuration.hpp:32-49) */
    int32_t hash_use;                      /* false                                        */
    uint64_t hash_period;                  /* 10                                           */
    double hash_percentage;                /* 0.05                                         */
    double hash_avg_factor;                /* 0.1                                          */
    uint64_t hash_slope_bins;              /* 20                                           */
    uint64_t hash_angular_steps;           /* 16                                           */
    int32_t log_debug;                     /* Configuration::logDebug (false)              */
    /* build-specific knobs (not in the reference) */
    uint32_t flags;                        /* ESLAM_FLAG_*                                 */
    /* per-particle maps (ESLAM_FLAG_PARTICLE_MAPS): the device page pool, in pages of 8 x 8
     * cells per particle (0: the default, 16); the pool is shared by all particles' maps and
     * collected when a map update needs more (ESLAM_ERR_OUT_OF_MEMORY when even that fails) */
    uint32_t local_map_pages;
    /* Configuration::maxSensorRange (3.0, src/Configuration.hpp:107): a particle's own map keeps
     * the tiles of 8 x 8 cells within this range of the particle             */
    double max_sensor_range;
    /* per-particle maps (ABI 7): tiles a map keeps after its window has left them (the trail;
     * the reference's MLSMap keeps every grid it made, src/EmbodiedSlamFilter.cpp:195-207), up
     * to this many per map (default 16; 0: tiles leaving the window are forgotten).  Their
     * pages come from the same pool (local_map_pages).                                       */
    uint32_t local_map_trail;
    /* rows of 64 particles per canonical summation chunk (ABI 8; 0: dm_chunk_rows(n_global),
     * the default).  The chunk fixes the order of the fp64 partial sums, so two
     * filters agree bit for bit only with the same value.  A sharded filter of G ranks may set
     * dm_chunk_rows(n_global / G) so that every rank's weighting kernel fills the chip (16M
     * over 8 ranks: 7 instead of 13); its one-GPU equal then sets the same.  At most 31.     */
    uint32_t sum_chunk_rows;
} eslam_config;

#define ESLAM_FLAG_RECORD_ANCESTORS 0x1u   /* keep the last resample's ancestor indices     */
#define ESLAM_FLAG_NO_MAP_LDS 0x2u         /* disable the LDS map window (global lookups)   */
#define ESLAM_FLAG_NO_AUX_GATHER 0x4u      /* do not carry mprob/floating through resample  */
#define ESLAM_FLAG_PARTICLE_MAPS 0x10u     /* useSharedMap = false: every particle its own local
                                              map (eslam_gpu_map_update)                      */
#define ESLAM_FLAG_RECORD_CONTACTS 0x8u    /* keep every update's cpoints, meas_pos, meas_theta
                                              (also on with log_debug); on a sharded filter
                                              download_records is then a collective          */
#define ESLAM_FLAG_PROCESS_STATICS 0x20u  /* Q11: the hash-respawn counter (the function static
                                              of src/PoseEstimator.cpp:239) and rand() are the
                                              process's, shared by every context that sets this
                                              flag (default: each context its own); one
                                              sharded (nranks > 1) context per process may
                                              set it: eslam_gpu_set_comm refuses a second
                                              (ranks in one process would share them)        */

void eslam_config_default(eslam_config* cfg);

/* ---- multi-level surface grid (envire::MLSGrid as consumed by GridAccess::get) ----------
 * Cells are (m, n) with m along x; cell index = n * width + m.  Patches of cell c are
 * patches[cell_start[c] .. cell_start[c+1]) in stored order.  getPatch(p, patch, 3.0)
 * transforms p by global2local, finds the cell with
 *   m = floor((x - offset_x) / scale_x), n = floor((y - offset_y) / scale_y),
 * and returns the first patch whose distance to the query patch (mean = p.z,
 * stdev = sqrt(measVar)) is below 3:  |mean_p - mean_q| / sqrt(stdev_p^2 + stdev_q^2)
 * (vertical patches, height > 0, span [mean - height, mean]).                           */
typedef struct eslam_mls_grid {
    uint32_t width, height;
    double scale_x, scale_y;
    double offset_x, offset_y;
    double global2local[12];               /* 3x4 row-major affine: GridAccess::C_global2local */
    const uint32_t* cell_start;            /* width*height + 1 entries                       */
    const float* patch_mean;               /* n_patches                                      */
    const float* patch_stdev;              /* n_patches                                      */
    const float* patch_height;             /* n_patches or NULL (all horizontal)             */
    uint64_t n_patches;
} eslam_mls_grid;

/* ---- per-step input: EmbodiedSlamFilter::update(body2odometry, bs, ltc) ---------------- */
typedef struct eslam_contact_point {       /* odometry::BodyContactPoint                    */
    double position[3];                    /* body frame                                    */
    float contact;                         /* contact probability, NaN = unknown (passes)   */
    int32_t group_id;                      /* -1 = ungrouped                                */
} eslam_contact_point;

typedef struct eslam_step_input {
    double body2odometry_rot[4];           /* quaternion (w, x, y, z) of body2odometry        */
    double body2odometry_trans[3];
    /* outputs of the external odometry::FootContact after odometry.update(bs, orientation):
     * getPoseDelta().position, getPositionError()(2,2) and the Gaussian that
     * getPoseDeltaSample2D() samples (mean dx, dy, dtheta; 3x3 covariance, row-major).
     *
     * The sampler draws mean + L z with L the lower Cholesky factor of sample_cov.  Only the
     * LOWER triangle is read, sample_cov[i * 3 + j] with i >= j; the entries above the
     * diagonal are never used for the factor (they need not mirror the lower ones).  A pivot
     * that is not positive (a zero variance, a rank-deficient or slightly indefinite matrix)
     * gives a zero column of L, never a NaN: the all-zero matrix samples the mean exactly.
     *
     * Accepted domain: every entry of sample_mean and of sample_cov (all nine) finite, and
     * no diagonal entry of sample_cov negative.  eslam_gpu_project, eslam_gpu_update and
     * eslam_gpu_step return ESLAM_ERR_INVALID_ARG for anything else, before any kernel runs
     * and with the particles, the counters and the random streams unchanged.                */
    double pose_delta_trans[3];
    double position_error_zz;
    double sample_mean[3];
    double sample_cov[9];
    uint32_t n_contacts;                   /* contacts[] entries used; a value above
                                            * ESLAM_MAX_CONTACTS is clamped to it (the step
                                            * equals the one given ESLAM_MAX_CONTACTS)       */
    uint32_t ltc_count;                    /* terrain classifications given (gate only)      */
    eslam_contact_point contacts[ESLAM_MAX_CONTACTS];
} eslam_step_input;

/* ---- particle state, structure of arrays (PoseParticle, src/PoseParticle.hpp:52-86) ----- */
typedef struct eslam_particles {
    double* x;                             /* position.x                                    */
    double* y;                             /* position.y                                    */
    double* orientation;
    double* zpos;
    double* zsigma;
    double* weight;
    double* mprob;
    uint8_t* floating;
    uint8_t* n_contact_points;             /* cpoints.size() of the last updateWeights       */
} eslam_particles;

/* result of one PoseEstimator::update (device-side values, read after eslam_gpu_sync) */
typedef struct eslam_update_info {
    double effective;                      /* normalizeWeights() return value                */
    double weight_sum;                     /* sum of weights before normalisation            */
    double floating_weight;                /* sum_data_weights / data_particles              */
    double max_weight;                     /* PoseEstimator::max_weight after the update      */
    uint64_t data_particles;
    uint64_t total_points;
    int32_t resampled;
    int32_t uniform_reset;                 /* sumWeights <= 0 branch taken                   */
    uint64_t resample_overruns;            /* draws beyond the cumulative sum (clamped, Q5)  */
    uint64_t update_count;
    /* the last eslam_gpu_map_update (per-particle maps): scan patches beyond a particle's
     * window (farther than max_sensor_range; summed over the particles); maps the merge
     * changed while another particle shared them (copy on write: written to a free table the
     * particle then names); maps the merge changed in all (cells, or the window moved); scan
     * patches that landed on cells the shared grid covers (not merged: the per-particle map
     * holds only cells the shared grid leaves empty)                            */
    uint64_t map_patches_dropped;
    uint64_t map_stores_copied;
    uint64_t map_stores_changed;
    uint64_t map_patches_covered;
    /* the device side of the same map update (not in the oracle: they depend on how the
     * pages were shared): cell writes (inserts and fuses), pages taken from the pool (copies
     * on write and new tiles), pages left in the pool's free list                           */
    uint64_t map_cells_written;
    uint64_t map_pages_taken;
    uint64_t map_pages_free;
    /* (ABI 7) tiles the last map update's windows left that a full trail could not keep
     * (forgotten; summed over the particles; in the oracle too)                              */
    uint64_t map_tiles_evicted;
} eslam_update_info;

/* ---- lifecycle ------------------------------------------------------------------------ */
typedef struct eslam_ctx eslam_ctx;

/* PoseEstimator(odometry, config) / EmbodiedSlamFilter(odoConfig, config): binds `device`. */
int eslam_gpu_create(const eslam_config* cfg, int device, eslam_ctx** out);
/* Never collective: an exchange a sharded filter still owes (see eslam_gpu_set_comm) is
 * dropped, so destroy is safe on one rank's error path and after the communicator is gone.
 * SPMD code calls eslam_gpu_finish on every rank first.                                  */
void eslam_gpu_destroy(eslam_ctx* ctx);
/* Collective on a sharded filter (every rank, at the same point): completes the last
 * update's deferred exchange if this rank still owes it, then waits for the stream; on one
 * GPU it only waits for the stream.  A rank whose filter a rank-local fault poisoned (e.g.
 * ESLAM_ERR_OUT_OF_MEMORY from its page pool) cannot take part: finish returns at once
 * there, and peers that still owe the exchange would wait for it.  Treat such an error as
 * fatal for the whole group (abort the communicator), as for any failed collective.       */
int eslam_gpu_finish(eslam_ctx* ctx);
const char* eslam_gpu_last_error(const eslam_ctx* ctx);
int eslam_gpu_abi_version(void);
/* SHA-256 (hex) of the sources, headers and compiler flags the library was built from
 * (slam-eslam_amd/build_lib.py source_hash): identifies the exact build a run loaded      */
const char* eslam_gpu_build_id(void);
/* run on a caller-provided hipStream_t (NULL = the context's own stream) */
int eslam_gpu_set_stream(eslam_ctx* ctx, void* hip_stream);

/* ---- environment: PoseEstimator::setEnvironment src/PoseEstimator.cpp:47-62 and
 * GridAccess::setMap src/PoseEstimator.hpp:68-95 (shared map, useShared = true).  Device
 * memory: 8 bytes per patch (+4 with heights) and about 20.2 bytes per cell (range word,
 * a 16-byte record of the cell's range and first patch, one occupancy bit)                 */
int eslam_gpu_set_map(eslam_ctx* ctx, const eslam_mls_grid* grid);

/* ---- initialisation -------------------------------------------------------------------
 * PoseEstimator::init(N, mu, sigma, zpos, zsigma)  src/PoseEstimator.cpp:88-102
 * mu/sigma = (x, y, theta).  weight = 0 (Q3), floating = true.                          */
int eslam_gpu_init_gaussian(eslam_ctx* ctx, uint64_t n, const double mu[3], const double sigma[3],
                            double zpos, double zsigma);
/* EmbodiedSlamFilter::init(env, pose, useSharedMap=true)  src/EmbodiedSlamFilter.cpp:70-177
 * pose = position[3] + quaternion (w,x,y,z); particle count / errors from the config.    */
int eslam_gpu_init_pose(eslam_ctx* ctx, const double position[3], const double orientation[4]);
/* replace the particle set (getParticles() is a mutable reference in the reference)       */
int eslam_gpu_upload_particles(eslam_ctx* ctx, uint64_t n, const eslam_particles* p);
int eslam_gpu_download_particles(eslam_ctx* ctx, eslam_particles* p);
/* edit particles [first, first + count) in place, the way the reference's callers edit the
 * vector getParticles() returns (processMap's weights, src/EmbodiedSlamFilter.cpp:183-220):
 * every non-NULL field of p (arrays of count values) overwrites that field; the particle
 * set, the per-particle maps, the RNG and the last update's records stay.  The weight scale
 * of the next update is then set from the largest weight, as eslam_gpu_upload_particles does,
 * so an edit through this call and a download / edit / upload of the whole set lead to the
 * same particles bit for bit.  On a sharded filter the call is collective, like the upload:
 * every rank makes it at the same point (count may be 0, and any field may be NULL), and
 * the ranks agree on the weight scale of the next update whichever of them wrote weights. */
int eslam_gpu_write_particles(eslam_ctx* ctx, uint64_t first, uint64_t count, const eslam_particles* p);

/* ---- per-particle local maps (useSharedMap = false) -----------------
 * EmbodiedSlamFilter::processMap(scanMap, match=false, update=true)
 * (src/EmbodiedSlamFilter.cpp:179-232) after PoseEstimator::cloneMaps (src/PoseEstimator.cpp:
 * 31-47): every particle's map is the shared grid plus its own patches in cells the grid
 * leaves empty, kept in a window of tiles of 8 x 8 cells centred on the particle that reaches
 * max_sensor_range (maxSensorRange, 3 m) in every direction.  A map update
 * moves each particle's window to the tile under the particle (the active-grid switch of
 * :195-207; tiles that leave the window are forgotten), places the scan patches at the
 * particle's pose (Translation(x, y, 0) * Rz(theta); offset patch zPos, zSigma) and, per
 * patch, inserts it into an empty cell or fuses it (variance-weighted) with the particle's
 * patch there when within 3 sigma; cells of the shared grid are not changed, and a patch
 * beyond the window is dropped (counted).  With an empty shared grid every particle starts
 * from an empty map, as the reference's clones of its empty grid template
 * (src/EmbodiedSlamFilter.cpp:131-134).  The contact update then reads each particle's own
 * map.  Particles that a resample copied share their tables and pages until a map update
 * writes them (copy on write).  set_map starts every particle's map over (empty).  Only the
 * insert-into-empty-cell rule is pinned by the reference (test/testMap.cpp:307-316);
 * envire's MLSGrid::merge is not in the reference.                                       */
typedef struct eslam_scan_patch {
    double position[3];                    /* yaw-free body frame (the scan MLS's cells)    */
    double stdev;                          /* sensor sigma of the patch                      */
} eslam_scan_patch;
/* Any count: a scan of more than 64 patches merges 64 at a time, in order (every cell sees
 * its patches in the scan's order); the update's counters add up over the parts
 * (map_stores_changed counts a map once per part that changed it).                          */
int eslam_gpu_map_update(eslam_ctx* ctx, const eslam_scan_patch* patches, uint32_t count);
/* processMap(scanMap, match = true, ...)  src/EmbodiedSlamFilter.cpp:214-221: the visual
 * weighting w *= pow(weight, 0.1f) of every particle against its own map (per-particle maps).
 * envire's MLSGrid::match is not in the reference, so the rule is this build's (DESIGN.md 5c,
 * parity unpinned): every 10th scan patch (sampling 10), placed like the merge, that lands on
 * a cell the particle's own map holds -- a tile inside both its window and the window the
 * next update centres on the particle -- scores exp(-d^2 / (2 sigma^2)), sigma 0.2f, d = the
 * patch's height + zPos - the cell's mean; weight = the mean score as a float (1 without a
 * matched cell).  Call it before eslam_gpu_map_update, as processMap does; weights are not
 * normalised.                                                                              */
int eslam_gpu_map_match(eslam_ctx* ctx, const eslam_scan_patch* patches, uint32_t count);
/* PoseEstimator::setEnvironment(env, map, useShared)  src/PoseEstimator.cpp:49-62: on = 1
 * gives every particle its own map (ESLAM_FLAG_PARTICLE_MAPS), 0 the shared map only.  Before
 * the particles are initialised (ESLAM_ERR_INVALID_ARG after).  On a sharded filter a
 * particle that a resample moves to another rank carries its own patches.                 */
int eslam_gpu_set_particle_maps(eslam_ctx* ctx, int on);
/* particle index's own patches (cell = n * width + m, mean, stdev), its window's tiles in slot
 * order and each tile's cells row by row; *count = how many it has (up to capacity written).
 * A debugging aid: one small host copy per page, and only the particle's own cells.  The map
 * a particle's lookups see is eslam_gpu_get_particle_grid below.                            */
int eslam_gpu_get_particle_map(eslam_ctx* ctx, uint64_t index, uint32_t* cells, float* mean, float* stdev,
                               uint32_t capacity, uint32_t* count);
/* particles[index].grid.getMap()  src/PoseEstimator.hpp:79-87 (GridAccess::getMap; the viewer
 * reads it, viz/EslamWidget.cpp:108-116): particle index's whole map as one MLS grid, composed
 * on the device.  Per cell the particle's own patch, if it has one there (a cell of a page of
 * its window or of its trail; height 0), then the shared grid's patches of the cell in their
 * order with their heights; cell_start is the exclusive prefix of those counts; scale, offset
 * and global2local are the shared grid's, and the composed grid has heights if and only if the
 * shared grid has.  A particle whose map was never centred gives the shared grid itself.
 * getPatch on this grid (the first patch of the cell's list that passes the 3-sigma gate)
 * answers as the particle's own lookups do, so a filter given the grid by eslam_gpu_set_map
 * weighs a particle at that pose exactly as this filter weighs particle index.
 * _size gives the composed patch count; the arrays are those of eslam_gpu_get_map
 * (cell_start: width * height + 1 entries, eslam_gpu_map_size; patch_height may be NULL).
 * Each call composes anew (the size call stops after the count); the device arrays composed
 * into, a second set of the grid's arrays, stay with the context for the next export until
 * the map is replaced.  Rank-local on a sharded filter: index is the local one.
 * Errors: ESLAM_ERR_INVALID_ARG (null pointers, no ESLAM_FLAG_PARTICLE_MAPS, index out of
 * range, patch_capacity below the composed count, a composed count past 2^32 - 1),
 * ESLAM_ERR_NO_ENVIRONMENT, ESLAM_ERR_NOT_INITIALISED, ESLAM_ERR_UNSUPPORTED (a grid of
 * 2^32 - 1 cells or more), ESLAM_ERR_OUT_OF_MEMORY (no device memory for the composed arrays);
 * a poisoned filter returns its fault.  The filter does not change.                        */
int eslam_gpu_particle_grid_size(eslam_ctx* ctx, uint64_t index, uint64_t* n_patches);
int eslam_gpu_get_particle_grid(eslam_ctx* ctx, uint64_t index, uint32_t* cell_start, float* mean, float* stdev,
                                float* patch_height /* may be NULL */, uint64_t patch_capacity);
/* Continue in particle index's map: leaves the context exactly as eslam_gpu_set_map of the grid
 * eslam_gpu_get_particle_grid(index) returns would, without the host round trip.  The composed
 * arrays become the shared grid, the pose hash is invalidated and every particle's own map
 * starts over, empty.  The new arrays exist before anything changes: ESLAM_ERR_OUT_OF_MEMORY
 * leaves the filter as it was.  On a sharded filter ESLAM_ERR_UNSUPPORTED, with no collective
 * run: export on the owning rank and give every rank the grid by eslam_gpu_set_map.  The other
 * errors are eslam_gpu_get_particle_grid's.                                                  */
int eslam_gpu_adopt_particle_map(eslam_ctx* ctx, uint64_t index);

/* ---- the shared map (useSharedMap = true): processMap's merge into the one grid ----------
 * EmbodiedSlamFilter::processMap(scanMap, match, update = true) with a shared map
 * (src/EmbodiedSlamFilter.cpp:184-227; the camera path's call at :301): every particle's pgrid
 * is the one shared grid, so the scan is merged into it once per particle, at that particle's
 * pose, in particle order.  envire's MLSGrid::merge is not in the reference, so the fuse rule
 * is this build's (parity unpinned):
 *   particles i = 0..N-1 in index order, scan patches k = 0..P-1 in scan order; a particle
 *   whose x - offset_x, y - offset_y or theta is not finite is skipped; a patch is placed as
 *   eslam_gpu_map_update places it (wz = z + zPos_i, var = stdev^2 + zSigma_i^2) and skipped
 *   when it falls off the grid.  A placed patch goes to the first patch of its cell, in list
 *   order, that passes getPatch's 3-sigma gate (dm_mls_gate): a horizontal one becomes their
 *   variance-weighted fusion (dm_lm_fuse), a vertical one (height > 0) stays and absorbs it;
 *   when none passes, {(float)wz, (float)sqrt(var), height 0} is appended to the cell's list.
 * A later particle sees what earlier ones wrote: the result is that of the sequential loop,
 * bit for bit, however the work is split.  Particles, weights and the RNG do not change; the
 * pose hash is not rebuilt (the reference builds it once, in init); later steps, matches and
 * eslam_gpu_hash_create see the merged grid.                                               */
typedef struct eslam_shared_merge_info {
    uint64_t particles_done;               /* particles worked through (all of them on success) */
    uint64_t patches_placed;               /* (particle, patch) pairs that landed on the grid  */
    uint64_t patches_off_grid;             /* pairs not placed: off the grid, or of a particle
                                              with a non-finite pose                           */
    uint64_t cells_touched;                /* distinct cells that received a placed patch      */
    uint64_t fused;                        /* placed patches fused into a horizontal patch     */
    uint64_t absorbed;                     /* placed patches a vertical patch absorbed (or a
                                              fuse left as it was): placed - fused - inserted  */
    uint64_t inserted;                     /* placed patches appended as new patches           */
    uint64_t n_patches;                    /* patches of the grid after the call               */
    uint64_t runs;                         /* runs the particles were worked through in        */
} eslam_shared_merge_info;
/* The particles are worked through in consecutive runs of whole particles, each of at most
 * max_records (particle, patch) records and at least one particle; a run places its records,
 * sorts them stably by cell, merges every touched cell's records in order and rebuilds the
 * grid's arrays.  max_records bounds the device scratch at about 32 bytes per record (plus 12
 * per cell); 0 means 2^21 records, 64 MiB.  The scratch stays with the context.  While the
 * call runs, a second copy of the grid's arrays exists.
 * Errors: ESLAM_ERR_INVALID_ARG (null arguments, a filter with ESLAM_FLAG_PARTICLE_MAPS,
 * non-finite patches), ESLAM_ERR_NO_ENVIRONMENT (no map), ESLAM_ERR_NOT_INITIALISED (no
 * particles), ESLAM_ERR_UNSUPPORTED (a sharded filter: every rank holds its own copy of the
 * grid, and the merge in global particle order is the collective
 * eslam_gpu_shared_map_update_sharded below; this call runs no collective),
 * ESLAM_ERR_OUT_OF_MEMORY (an allocation failed, or a run's placed patches could take the
 * grid past 2^32 - 1 patches).  After a failure the grid holds the runs merged before it
 * (info->particles_done particles).  count == 0 succeeds and changes nothing.  info may be
 * NULL.                                                                                    */
int eslam_gpu_shared_map_update(eslam_ctx* ctx, const eslam_scan_patch* patches, uint32_t count, uint64_t max_records,
                                eslam_shared_merge_info* info);
/* The same merge on a sharded filter (eslam_gpu_set_comm), a collective in SPMD order: every
 * rank passes the same scan and the same max_records.  The particles run in global index
 * order 0 .. n_global-1, and every rank merges every run into its own copy of the grid, so
 * afterwards every rank's grid (and the cell table and occupancy bits the step and the match
 * read) equals, byte for byte, the grid of one context holding all n_global particles.  Per
 * run the ranks exchange the run's poses (x, y, theta, zPos, zSigma: 40 bytes per particle,
 * one all_to_all_v), not the records.  The runs are those of the plain call with n = n_global,
 * and info (the same on every rank) counts global particles and records.
 * Memory: the plain call's scratch, bounded by max_records, plus the exchange memory of at
 * most (nranks + 1) x run particles x 40 bytes (a run has at most max_records / count
 * particles, at least one), kept with the context like the scratch.
 * Every check the plain call makes on its arguments and the filter's state runs before the
 * first collective, with the plain call's codes.  The ranks then compare {count, max_records,
 * a 64-bit hash of the patches' bytes}: when they differ every rank returns
 * ESLAM_ERR_INVALID_ARG and no grid has changed.  Before a run changes any grid the ranks
 * agree that each of them has the memory for it: when one has not, it returns its own code
 * (ESLAM_ERR_OUT_OF_MEMORY), the others ESLAM_ERR_COMM, and every rank holds the grid of the
 * same completed runs with the same info->particles_done; ESLAM_OK on one rank means every
 * rank succeeded.  A failed callback is ESLAM_ERR_COMM.  count == 0 succeeds and changes
 * nothing (the ranks still compare it).  On a filter that is not sharded this is the plain
 * call: the same bytes, the same counters.                                                 */
int eslam_gpu_shared_map_update_sharded(eslam_ctx* ctx, const eslam_scan_patch* patches, uint32_t count,
                                        uint64_t max_records, eslam_shared_merge_info* info);
/* the shared grid as the device holds it (after eslam_gpu_set_map and every merge since): its
 * size (any pointer may be NULL) ...                                                        */
int eslam_gpu_map_size(eslam_ctx* ctx, uint32_t* width, uint32_t* height, uint64_t* n_patches, int* has_height);
/* ... and its arrays: cell_start (width * height + 1 entries), mean and stdev (n_patches, at
 * most patch_capacity: ESLAM_ERR_INVALID_ARG when it holds more), patch_height (may be NULL;
 * zeros when the grid has no heights)                                                       */
int eslam_gpu_get_map(eslam_ctx* ctx, uint32_t* cell_start, float* mean, float* stdev, float* patch_height,
                      uint64_t patch_capacity);

/* ---- the scan MLS from a sensor reading ------------------------------------
 * EmbodiedSlamFilter::update(body2odometry, LaserScan, laser2body) and
 * update(body2odometry, DistanceImage, camera2body) (src/EmbodiedSlamFilter.cpp:311-351,
 * 239-309) hand the reading to envire's ScanMeshing / DistanceGridToPointcloud and MLSProjection,
 * which are not in the reference tree; the rule below is this build's (parity unpinned).  All
 * arithmetic is fp64 of eslam_detmath.h, no contraction.
 *   points   laser beam i: a = start_angle + i * angular_resolution, r = ranges[i] * 1e-3,
 *            q = (r cos a, r sin a, 0) (dm_sincos); valid when ranges[i] > 5 (the error codes) and
 *            min_range <= ranges[i] <= max_range; dropped (out of range) when r > max_sensor_range.
 *            depth pixel (u, v), d = data[v * width + u]: q = ((u scale_x + center_x) d,
 *            (v scale_y + center_y) d, d); valid when d is finite and > 0; dropped when
 *            d > max_sensor_range.
 *   placed   b = R_s2b q + t_s2b, p = R_w b with R_w = removeYaw(orientation): the yaw-free body
 *            frame of eslam_scan_patch.
 *   variance of p.z, first order in small rotation errors: about sensor axis e_k (sigma
 *            sensor_rot_sigma[k]) g = (R_w R_s2b).row(2) . (e_k x q); about body axis e_k (sigma
 *            body_rot_sigma[k]) g = R_w.row(2) . (e_k x b); var = sum sigma_k^2 g_k^2 over the six,
 *            at least min_sigma^2.
 *   cells    (floor(p.x / resolution), floor(p.y / resolution)) on a square grid centred on the
 *            scan frame's origin that holds every valid point (sized from max_sensor_range, the
 *            image's widest ray and |t_s2b|; below 2^32 - 1 cells, else ESLAM_ERR_INVALID_ARG).
 *   patches  a cell's points by ((float)p.z, point index) ascending; a point joins the current
 *            cluster when p.z - the previous p.z <= patch_thickness; a cluster's patch is the
 *            inverse-variance mean: w = 1 / var, mu = sum w z / sum w, v = 1 / sum w +
 *            sum w (z - mu)^2 / sum w, sums sequential in that order; position = (cell centre,
 *            mu), stdev = sqrt(v).  Patches come out by cell index (y-major), then by cluster.
 * The result does not depend on how the device splits the work.  Out of the rule: negative
 * information (gridUseNegativeInformation), the texture image, update(Featurecloud*).          */
typedef struct eslam_scan_params {
    double sensor2body[12];                /* laser2body / camera2body, 3x4 row-major         */
    double orientation[4];                 /* body2odometry's rotation, quaternion (w, x, y, z) */
    double sensor_rot_sigma[3];            /* (5 deg, 0, 0)  src/EmbodiedSlamFilter.cpp:323-325 */
    double body_rot_sigma[3];              /* (3 deg, 3 deg, 0)  :332-334                      */
    double min_sigma;                      /* 1e-3 (the z-sigma floor of :124); > 0            */
    double resolution;                     /* Configuration::gridResolution (0.05)             */
    double patch_thickness;                /* Configuration::gridPatchThickness (0.1)          */
    double max_sensor_range;               /* Configuration::maxSensorRange                    */
} eslam_scan_params;
/* identity transforms, the sigmas above, resolution 0.05, thickness 0.1, cfg's max_sensor_range */
int eslam_scan_params_default(const eslam_config* cfg, eslam_scan_params* p);

typedef struct eslam_laser_scan {          /* base::samples::LaserScan                         */
    double start_angle, angular_resolution;    /* radians                                      */
    uint32_t min_range, max_range;         /* millimetres                                      */
    uint32_t n;
    uint32_t pad;
    const uint32_t* ranges;                /* n, millimetres (1..5: error codes)               */
} eslam_laser_scan;

typedef struct eslam_depth_image {         /* base::samples::DistanceImage                     */
    uint32_t width, height;
    double scale_x, scale_y, center_x, center_y;
    const float* data;                     /* width * height, row-major, metres                */
} eslam_depth_image;

typedef struct eslam_scan_info {
    uint64_t points;                       /* beams or pixels                                  */
    uint64_t points_valid;                 /* points binned                                    */
    uint64_t points_invalid;
    uint64_t points_out_of_range;          /* valid readings beyond max_sensor_range           */
    uint64_t cells;                        /* cells with a point                               */
    uint64_t patches;
} eslam_scan_info;

/* Synchronous; the patches stay on the device with the context until the next build.  They need
 * no map and no particles and change neither; on a sharded filter they are rank-local (every
 * rank given the same reading holds the same patches).  A reading without a valid point
 * succeeds with 0 patches.  ESLAM_ERR_INVALID_ARG (with a message): null pointers, non-finite
 * transforms, orientations or sigmas, min_sigma, resolution, patch_thickness or
 * max_sensor_range <= 0, a zero-size image, non-finite image scales, more than 2^30 points.
 * info may be NULL.                                                                          */
int eslam_gpu_scan_from_laser(eslam_ctx* ctx, const eslam_laser_scan* scan, const eslam_scan_params* params,
                              eslam_scan_info* info);
int eslam_gpu_scan_from_depth(eslam_ctx* ctx, const eslam_depth_image* image, const eslam_scan_params* params,
                              eslam_scan_info* info);
/* the last built scan: *count = its patches, the first min(capacity, *count) copied to out
 * (out may be NULL with capacity 0)                                                          */
int eslam_gpu_scan_patches(eslam_ctx* ctx, eslam_scan_patch* out, uint64_t capacity, uint64_t* count);

/* ---- PoseParticle records with the debug fields (getParticles() for logging / viz) ------ */
/* ContactPoint  src/PoseParticle.hpp:20-43: one contact point evaluatePose pushed           */
typedef struct eslam_cpoint {
    double point[3];                       /* surface point: world x, y of the group's first
                                              valid contact and the patch mean (:163-171)   */
    double zdiff, zvar;                    /* ratio-weighted group averages                 */
    double prob;                           /* 1 (the slip update never reaches it, Q8)      */
} eslam_cpoint;

/* PoseParticle  src/PoseParticle.hpp:52-86 as the viz reads it (viz/ParticleVisualization.cpp) */
typedef struct eslam_particle_record {
    double position[2];
    double orientation, zpos, zsigma, mprob, weight;
    double meas_pos[3];                    /* (x, y, zPos) at the last updateWeights          */
    double meas_theta;                     /* orientation at the last updateWeights           */
    uint64_t index;                        /* global particle index                          */
    uint32_t n_cpoints;                    /* cpoints.size()                                 */
    uint8_t floating;
    uint8_t pad[3];
} eslam_particle_record;

/* Particles first, first + stride, ... (count of them) as records, gathered on the device
 * (one copy of count records; a strided subsample keeps logging cheap at millions of
 * particles).  With ESLAM_FLAG_RECORD_CONTACTS (or log_debug) the meas_* fields and up to
 * max_cpoints contact points per particle (cpoints: count x max_cpoints, may be NULL) are
 * those of the last update, carried through its resample like the reference's vectors;
 * otherwise meas_* are 0 and n_cpoints = the count of the last update.
 * Sharded with ESLAM_FLAG_RECORD_CONTACTS / log_debug: a collective (every rank calls it, in
 * the same order, count may be 0): a particle whose ancestor at the last update sat on another
 * rank gets that ancestor's records from it (two all_to_all_v); a rank whose own call fails
 * still takes part and makes every rank return an error.                                    */
int eslam_gpu_download_records(eslam_ctx* ctx, uint64_t first, uint64_t stride, uint64_t count,
                               eslam_particle_record* out, eslam_cpoint* cpoints, uint32_t max_cpoints);
int eslam_gpu_particle_count(const eslam_ctx* ctx, uint64_t* n);

/* ---- the hot path ----------------------------------------------------------------------- */
/* EmbodiedSlamFilter::update(body2odometry, bs, ltc): project, then the measurement update
 * when UpdateThreshold::test(udPose^-1 * body2odometry) (angle/distance swapped, Q6) or
 * ltc_count > 0.  *updated receives the bool.  Asynchronous on the context stream.
 * A zero measurement variance (measurementError = 0 and zSigma = 0; the throw of
 * src/ContactModel.cpp:122-123) returns ESLAM_ERR_ZERO_MEAS_VAR from this call: phase A has
 * run (such particles count as rejected with no contact points), phase B, normalisation and
 * the resample have not, and the update gate pose is not advanced.  Deviation: the reference
 * aborts its particle loop at the first such particle, leaving the later ones projected only. */
int eslam_gpu_step(eslam_ctx* ctx, const eslam_step_input* in, int* updated);
/* PoseEstimator::project(state, orientation)                                              */
int eslam_gpu_project(eslam_ctx* ctx, const eslam_step_input* in);
/* PoseEstimator::update(state, orientation, ltc): updateWeights, normalizeWeights, resample
 * if effective < minEffective.                                                             */
int eslam_gpu_update(eslam_ctx* ctx, const eslam_step_input* in);
/* wait for the stream; fetch the info of the last update (info may be NULL)               */
int eslam_gpu_sync(eslam_ctx* ctx, eslam_update_info* info);
/* The resample scan's blocks wait for each other (the fused finalize, the preceding tiles'
 * totals).  A wait that gives up -- never expected: the blocks it waits for are dispatched
 * first -- poisons the filter: nothing further is written, and every later call (step,
 * update, sync, download, the ParticleFilter API) returns ESLAM_ERR_HIP until init_* or
 * upload_particles starts over.  Testing only: polls before a wait gives up (default 2^18,
 * about 60 ms; 0 gives up at once, which forces the poisoned path).                        */
int eslam_gpu_debug_set_spin_limit(eslam_ctx* ctx, uint32_t polls);
/* Testing only: particles per thread of the one-GPU resample scan (1, 2, 4 or 8; 0 restores
 * the rule by particle count).  The tile totals are exact integers, so the tile size never
 * changes a result; the hook lets small filters run the instantiation of large ones.       */
int eslam_gpu_debug_set_scan_items(eslam_ctx* ctx, uint32_t items);
/* eslam_config.min_effective of this context from the next update on (every update reads it): 0
 * never resamples, a value above the particle count resamples at every update.  The ranks of a
 * sharded filter set the same value.                                                          */
int eslam_gpu_set_min_effective(eslam_ctx* ctx, uint64_t min_effective);

/* ---- ParticleFilter<T> API (src/ParticleFilter.hpp:34-173) ------------------------------ */
int eslam_gpu_get_weights_sum(eslam_ctx* ctx, double* sum);          /* getWeightsSum :34-39     */
int eslam_gpu_normalize_weights(eslam_ctx* ctx, double* effective);  /* normalizeWeights :46-70 */
int eslam_gpu_resample(eslam_ctx* ctx);        /* resample() -> resample_stratified(N) :72-108 */
/* resample_stratified(samples) :85-108 and resample_multinomial(samples) :120-148: resample the
 * weights as they stand (as eslam_gpu_resample: a deferred exchange is settled and a pending
 * gather run first, the contact records are invalidated) to `samples` particles.  Both use the
 * fixed-point cumulative sum C_i and shift of eslam_gpu_resample (61 - (dm_weight_exp(S) + 1),
 * S the exact weight sum) and move the minstd state on by exactly `samples` draws.
 *   stratified   draw k < samples is T_k = fx((k + U_k) / samples); particle i fills the outputs
 *                [#{T <= C_(i-1)}, #{T <= C_i}), the last particle every draw up to `samples`
 *                (the Q5 clamp, counted in overruns); weights are carried (Q4).  samples == n is
 *                eslam_gpu_resample, bit for bit.
 *   multinomial  draw n is T_n = fx(U_n), U_n the boost uniform of the (n+1)-th minstd draw; its
 *                ancestor is the first i with T_n <= C_i (the reference's r_n <= sum); a draw
 *                with T_n > C_(N-1) is dropped and counted (unnormalised weights summing below 1);
 *                the outputs keep draw order, n_after = samples - dropped, and every output's
 *                weight is 1.0 / (double)n_before (:140, the old count).
 * The outputs carry every field of their ancestor (mprob, floating, the contact count, also
 * under ESLAM_FLAG_NO_AUX_GATHER when the count changes: a set of another size has no old
 * values to keep); with
 * ESLAM_FLAG_RECORD_ANCESTORS eslam_gpu_get_ancestors returns n_after ancestors in the old
 * indexing.  Every later call works at n_after particles, the sum contract's chunk rows
 * included, as in a filter initialised at that count.  Shrinking keeps the allocation; growing
 * beyond it allocates the larger particle set before anything changes
 * (ESLAM_ERR_OUT_OF_MEMORY: the filter is as it was).  Synchronous.
 * Limits: samples == 0 or samples >= 2^32 - 1 is ESLAM_ERR_INVALID_ARG with nothing changed
 * (deviation: the reference would empty the filter).  A multinomial call that drops every draw
 * leaves no particles: later calls return ESLAM_ERR_NOT_INITIALISED as before init.  With
 * ESLAM_FLAG_PARTICLE_MAPS, samples may not exceed the count the filter was initialised with
 * (the tables and pages are sized then): ESLAM_ERR_UNSUPPORTED, nothing changed, the RNG not
 * advanced; within it a copy names its ancestor's table and shares its pages until a map update
 * writes them.  A sharded filter accepts only a stratified call with samples == n_global (the
 * sharded eslam_gpu_resample); anything else is ESLAM_ERR_UNSUPPORTED on every rank, before any
 * collective.  The collective forms that take a sharded filter to any count are
 * eslam_gpu_resample_stratified_sharded / _multinomial_sharded below.  info may be NULL.    */
typedef struct {
    uint64_t n_before;   /* particles before the call                                  */
    uint64_t n_after;    /* particles after it                                         */
    uint64_t overruns;   /* stratified: draws beyond the cumulative sum (clamped, Q5)  */
    uint64_t dropped;    /* multinomial: draws with no particle (r_n > the weight sum) */
} eslam_resample_info;
int eslam_gpu_resample_stratified(eslam_ctx* ctx, uint64_t samples, eslam_resample_info* info);
int eslam_gpu_resample_multinomial(eslam_ctx* ctx, uint64_t samples, eslam_resample_info* info);
/* The same two calls on a sharded filter (eslam_gpu_set_comm), to any count.  Collective: every
 * rank calls in the same order with the same `samples`.  Afterwards the ranks' shards, in rank
 * order, are bit for bit the particle set one context holding the same global particles has after
 * eslam_gpu_resample_stratified / _multinomial(samples): every field, the weights (carried, or
 * 1.0 / (double)n_before with n_before the old global count), the ancestors (old global
 * indices), the minstd state (moved on by `samples` draws on every rank) and info (global
 * n_before, n_after, overruns, dropped, the same on every rank).
 * The new layout: the filter is sharded by eslam_gpu_shard_bounds(n_after, nranks,
 * cfg.sum_chunk_rows), as though eslam_gpu_set_comm had been called with that table before the
 * particles were set: the local count, n_global, the rank's first index and every buffer sized
 * by the table follow it, and so do the summation chunk rows.  A rank whose new shard exceeds its
 * capacity allocates the larger particle set before anything changes.  Every later call works
 * at the new count.  A deferred exchange of the previous update is settled first.
 * Refused on every rank alike, before any collective, with nothing changed:
 *   ESLAM_ERR_INVALID_ARG   samples == 0 or samples > 2^30 - 64 (eslam_gpu_set_comm's limit);
 *                           stratified: a count eslam_gpu_shard_bounds cannot split over the ranks
 *   ESLAM_ERR_UNSUPPORTED   ESLAM_FLAG_PARTICLE_MAPS (the tables and pages would have to travel)
 * A multinomial call learns n_after from its draws; every rank counts the same dropped draws.
 * n_after == 0 or a count that cannot be split is ESLAM_ERR_INVALID_ARG on every rank with
 * nothing changed, the minstd state included (it is committed only with the new particle set;
 * the one-GPU call moves it first).  A rank that cannot allocate tells the others in the call's
 * small all_gathers before any rank changes anything: it returns its own code, the others
 * ESLAM_ERR_COMM, the filter is as it was on all of them.
 * On a context that is not sharded these are the plain calls.  A stratified call at n_global on
 * the canonical table is the sharded eslam_gpu_resample.                                    */
int eslam_gpu_resample_stratified_sharded(eslam_ctx* ctx, uint64_t samples, eslam_resample_info* info);
int eslam_gpu_resample_multinomial_sharded(eslam_ctx* ctx, uint64_t samples, eslam_resample_info* info);
/* The canonical shard table of an n_global-particle filter over nranks ranks: near-equal shards
 * whose starts are multiples of the summation chunk (64 x the chunk rows of n_global;
 * sum_chunk_rows: eslam_config::sum_chunk_rows, 0 for the default).  bounds_out takes nranks + 1
 * entries, from 0 to n_global.  ESLAM_ERR_INVALID_ARG when n_global has fewer chunks than there
 * are ranks (a shard would be empty).  Pure host code: no context, no GPU.                   */
int eslam_gpu_shard_bounds(uint64_t n_global, int32_t nranks, uint32_t sum_chunk_rows, uint64_t* bounds_out);
/* the context's current table (nranks + 1 entries; capacity: the entries bounds_out has room for) */
int eslam_gpu_get_shard_bounds(eslam_ctx* ctx, uint64_t* bounds_out, uint32_t capacity);
int eslam_gpu_get_best_particle_index(eslam_ctx* ctx, uint64_t* index);  /* :160-173 (Q16)  */
/* PoseEstimator::getCentroid src/PoseEstimator.cpp:354-383 (normalises in place, Q15):
 * position[3] + quaternion (w,x,y,z)                                                        */
int eslam_gpu_get_centroid(eslam_ctx* ctx, double position[3], double orientation[4]);
/* the yaw-free body orientation (w,x,y,z) of the last step -- zCompensatedOrientation of
 * ContactModel::setContactPoints src/ContactModel.cpp:21-41 --, the factor getCentroid composes its
 * orientation with after the yaw about Z; the identity before any step.  Reads host state only. */
int eslam_gpu_get_z_compensated_orientation(eslam_ctx* ctx, double orientation[4]);

/* ---- PoseDistribution::gmm (src/PoseParticle.hpp:88-114): a 2-D Gaussian mixture over (x, y) --
 * Fitted by EM on the device over the particles as they stand (a deferred exchange is settled
 * and a pending gather run first) and their current weights at any scale, normalised or not.
 * envire's GaussianMixture / ExpectationMaximization are not in the reference tree: the rule is
 * this build's own, all fp64 through eslam_detmath.h, every sum in getCentroid's
 * order, so one GPU, a sharded filter and the CPU restatement give the same bits.  In short:
 * particles with finite x, y, w and w > 0 are fitted (the others skipped and counted); weights
 * are scaled by 2^-weight_exp and coordinates taken relative to the bounding box's centre; the
 * particles start in `components` equal slabs along the box's longer axis (slab order is the
 * order of `out`); then up to max_iterations fused E+M passes, stopping when the mean
 * log-likelihood moves by at most `tolerance` between two passes (from the second pass on).
 * A component that gathers no weight, or whose covariance + min_variance I is not positive
 * definite, is dead: it takes no further part and reports weight 0, mean 0, covariance 0 (from
 * the next M-step on).  The fit changes nothing in the filter: particles, weights (no in-place
 * normalise, unlike eslam_gpu_get_centroid), RNG, maps and pose hash are as before.  Synchronous;
 * needs particles, no map.
 * ESLAM_ERR_INVALID_ARG (checked before any launch or collective): a null ctx, params or out;
 * components 0 or > ESLAM_GMM_MAX_COMPONENTS; tolerance negative or NaN; min_variance not finite
 * or <= 0.  ESLAM_ERR_NOT_INITIALISED: no particles.  A poisoned filter returns its fault.
 * No fitted particle: ESLAM_OK, components_live 0, every output zero.
 * Sharded filters: a collective in SPMD order.  The ranks first compare their parameters (one
 * all_gather of host words; a mismatch is ESLAM_ERR_INVALID_ARG on every rank); every rank
 * returns the one-GPU result bit for bit and takes the same stop decision.                  */
#define ESLAM_GMM_MAX_COMPONENTS 8
typedef struct eslam_gmm_params {
    uint32_t components;       /* K, 1..ESLAM_GMM_MAX_COMPONENTS                               */
    uint32_t max_iterations;   /* 0: the initial assignment's parameters, log_likelihood NaN   */
    double tolerance;          /* on the mean log-likelihood of successive passes              */
    double min_variance;       /* added to the covariances' diagonal in the E-step (m^2)       */
} eslam_gmm_params;
void eslam_gmm_params_default(eslam_gmm_params* p);   /* 3 components, 10 iterations, 1e-5, 1e-6 */
typedef struct eslam_gmm_component {
    double weight;
    double mean[2];
    double cov[3];             /* xx, xy, yy */
} eslam_gmm_component;
typedef struct eslam_gmm_info {
    uint32_t components_live;  /* components that would take part in a further E-step          */
    uint32_t iterations;       /* fused passes run                                             */
    uint32_t converged;        /* the stop test passed                                         */
    uint32_t live_mask;        /* bit k: component k (out[k]) is live; components_live bits set */
    uint64_t particles_used, particles_skipped;
    double log_likelihood;     /* weighted mean log-likelihood measured by the last pass, i.e. */
                               /* of the parameters BEFORE the last M-step (NaN: no pass ran)  */
    double centre[2];          /* the bounding box's centre the sums were taken around         */
    int32_t weight_exp;        /* E with 2^(E-1) <= max w < 2^E                                */
} eslam_gmm_info;
int eslam_gpu_fit_pose_gmm(eslam_ctx* ctx, const eslam_gmm_params* params, eslam_gmm_component* out /* params->components */,
                           eslam_gmm_info* info /* may be NULL */);

/* ---- the pose estimate with its covariance: moments over (x, y, z, yaw), summed on the device --
 * Over the particles as they stand (a deferred exchange is settled and a pending gather run
 * first) and their current weights at any scale, normalised or not.  The rule is this build's own
 * (DESIGN.md 5i), all fp64 through eslam_detmath.h, every sum in getCentroid's order, so one GPU,
 * a sharded filter and the CPU restatement give the same bits.  In short: a particle is valid when
 * x, y, zpos, orientation, zsigma and w are finite and w > 0 (the others are skipped and counted).
 * With a gate a valid particle is counted when it lies inside the ellipse
 * (p - centre)^T cov^-1 (p - centre) <= chi2 over p = (x, y) -- a GMM component with chi2 = 9 is
 * its 3-sigma ellipse, the identity with chi2 = r^2 a circle -- else it is gated out and counted as
 * such; without a gate every valid particle is counted.  Weights are scaled by 2^-weight_exp, the
 * exponent of the largest VALID weight (the gate never moves the scale).  mean is the weighted
 * mean of x, y, z and the circular mean of the yaw, atan2 of the weighted sums of sin and cos
 * (0 when both vanish), in (-pi, pi]: unlike eslam_gpu_get_centroid's linear mean it holds when
 * the cloud straddles the +-pi cut or its yaws differ by whole turns.  cov is the weighted
 * covariance of the deviations from the mean, the yaw's wrapped to one turn around the circular
 * mean.  The call changes nothing in the filter: particles, weights (no in-place normalise), RNG,
 * maps and pose hash are as before.  Synchronous; needs particles, no map.
 * ESLAM_ERR_INVALID_ARG (checked before any launch or collective): a null ctx or out; a gate
 * whose cov has a determinant xx yy - xy^2 that is not finite or not > 0, or xx <= 0, whose chi2
 * is not finite or negative, or whose centre is not finite.  ESLAM_ERR_NOT_INITIALISED: no
 * particles.  A poisoned filter returns its fault.
 * No counted particle: ESLAM_OK, the counts filled, every double zero.
 * Sharded filters: a collective in SPMD order.  The ranks first compare their gates (one
 * all_gather of host words; a mismatch is ESLAM_ERR_INVALID_ARG on every rank); every rank
 * returns the one-GPU result bit for bit.                                                    */
typedef struct eslam_pose_gate { double centre[2]; double cov[3] /* xx, xy, yy */; double chi2; } eslam_pose_gate;
typedef struct eslam_pose_moments {
    uint64_t particles_counted, particles_gated_out, particles_skipped;
    double mean[4];          /* x, y, z, yaw: yaw the circular mean in (-pi, pi]           */
    double cov[16];          /* row-major, symmetric, over (x, y, z, yaw deviation)         */
    double z_within;         /* weighted mean of zSigma^2: add to cov[10] for the total z variance */
    double yaw_resultant;    /* mean resultant length R in [0, 1]                           */
    double effective;        /* (sum w)^2 / sum w^2 of the counted particles                */
    double weight_share;     /* counted weight / valid weight (1 without a gate)            */
    int32_t weight_exp, pad;
} eslam_pose_moments;
int eslam_gpu_pose_moments(eslam_ctx* ctx, const eslam_pose_gate* gate /* may be NULL */, eslam_pose_moments* out);

/* ---- the trajectory: particle ancestry and poses per step, traced and smoothed on the device ----
 * The reference keeps its history inside each particle's MLSMap and in the logged
 * PoseDistribution stream; this build keeps a log on the device.  It is opt-in,
 * created by eslam_gpu_trajectory_enable (no eslam_config field): a ring of capacity_steps
 * entries allocated in full at once, each SoA for up to max_particles particles (0: the
 * context's particle capacity, which then must not be 0): x, y, z, yaw, zsigma as fp64 and
 * parent as uint32, the slot of the particle's ancestor in the previous held entry.  That is 44
 * bytes per particle per entry, 185 MB per entry at 4M particles, plus two link arrays of 4 bytes
 * per particle.  No allocation happens on the step path; an allocation that fails at enable is
 * ESLAM_ERR_OUT_OF_MEMORY with the context as it was.  When the ring is full the oldest entry is
 * overwritten.  Enabling an enabled log replaces it (empty); disable frees it; clear empties it and
 * keeps it enabled.  An entry's step id is the number of records taken since enable before it.
 *   record   at the end of every eslam_gpu_step (its update gate open or closed: the particles
 *            moved) and every eslam_gpu_update whose kernels were enqueued (one that then returns
 *            ESLAM_ERR_ZERO_MEAS_VAR has recorded, without a resample); eslam_gpu_project alone
 *            records nothing.  Enqueued on the context's stream, no host wait: the pending
 *            resample gather is materialised (so no later kernel fuses it: the feature's per-step
 *            cost), then one kernel copies the five columns of the particles as they stand --
 *            after the resample when one happened -- and writes parent.
 *   link     link[i] is the slot, in the newest entry, of the ancestor of the current particle i:
 *            the identity after a record.  parent[i] = link[anc[i]] when the update resampled
 *            (anc: eslam_gpu_get_ancestors' array; the decision is read on the device), else
 *            link[i].  A resample outside the step (eslam_gpu_resample, _resample_stratified,
 *            _resample_multinomial, _resample_kld) composes link'[i] = link[anc[i]] over its
 *            outputs instead of recording, so entries may hold different particle counts.  One
 *            that would leave more than max_particles particles is ESLAM_ERR_INVALID_ARG before
 *            anything changes, and so is an upload, init or load of more.
 *   cleared  (still enabled) by eslam_gpu_upload_particles, the eslam_gpu_init_* calls and every
 *            eslam_gpu_load*; snapshots do not carry the log.  eslam_gpu_write_particles and the
 *            hash respawn keep the slot's lineage: the pose jumps between two entries.  The map
 *            calls do not touch it.
 * While the log is enabled the filter keeps ancestors as with ESLAM_FLAG_RECORD_ANCESTORS.  The
 * filter itself -- particles, weights, RNG, maps -- is bit for bit what it is without the log.
 *
 * Sharded filters keep the log through eslam_gpu_trajectory_enable_sharded, called after
 * eslam_gpu_set_comm* like the other *_sharded calls.  Plain eslam_gpu_trajectory_enable on a
 * sharded filter is ESLAM_ERR_UNSUPPORTED, and so is eslam_gpu_set_comm* on a context whose log
 * is enabled.  On a context that is not sharded the _sharded call is the plain one.
 *   enable   a collective in SPMD order; every rank passes the same capacity_steps.
 *            max_particles is per rank: the slots of this rank's part of an entry (0: the rank's
 *            particle capacity).  The ranks agree in one small all_gather before anything
 *            changes: a rank that cannot enable (its arguments, no memory) returns its own code
 *            and the others ESLAM_ERR_COMM; differing capacity_steps are ESLAM_ERR_INVALID_ARG on
 *            every rank.  capacity_steps == 0 is refused before the collective.
 *   contract the ranks' entries, in rank order, are slot for slot the entries of one context
 *            that holds all n_global particles and took the same calls.  parent and link hold
 *            GLOBAL slots: indices into the previous held entry / the newest entry in the layout
 *            (shard table) that entry was recorded under; n_global <= 2^30 - 64 fits the uint32.
 *            Per entry the host keeps the shard table (nranks + 1 bounds), the global count and
 *            the step id, identical on every rank.
 *   record   as on one GPU, at the end of every eslam_gpu_step / eslam_gpu_update; the update's
 *            deferred exchange is settled first, then the gather is materialised, then the
 *            record kernel runs.  While the link is the identity (since the last record) the
 *            parents are the ancestors themselves (old global indices) and the record adds no
 *            collective; after a resample outside the step, link[anc[i]] is fetched from its owner.
 *   resample eslam_gpu_resample_*_sharded (and the sharded eslam_gpu_resample, _resample_kld)
 *            compose the link across the ranks, from the old shard table to the new one.  One
 *            that would give any rank more than that rank's max_particles is
 *            ESLAM_ERR_INVALID_ARG on every rank with nothing changed: for the stratified call
 *            before any collective (the shards follow from eslam_gpu_shard_bounds(samples)), for
 *            the multinomial call where it learns n_after.
 *   calls    disable and info are local; clear, eslam_gpu_get_trajectories and
 *            eslam_gpu_trajectory_smoothed are collectives.  info: entries, first_step, last_step
 *            and capacity_steps as on one GPU, particles the newest entry's GLOBAL count,
 *            max_particles and bytes this rank's.
 *   queries  get_trajectories: every rank passes the same list of GLOBAL particle indices and
 *            the same capacity, and receives the whole result; slot is the global slot and
 *            particles the entry's global count, so the result is byte for byte the one
 *            context's.  An index >= n_global, like every argument error, is refused before the
 *            first collective; lists that differ between the ranks (count or capacity, then
 *            contents, compared by all_gather) are ESLAM_ERR_INVALID_ARG on every rank.
 *            trajectory_smoothed: every rank receives, per held entry, the one context's
 *            estimate bit for bit; distinct_ancestors is the sum of the owners' marked slots.
 *   failures a rank that fails inside a query or a composition (scratch memory) says so in the
 *            counts the exchange gathers: it returns its code, the others ESLAM_ERR_COMM, none waits.
 *
 * eslam_gpu_get_trajectories: for each current particle indices[k] (< the particle count, repeats
 * allowed) its lineage: from link[index] in the newest entry along parent back through the
 * newest *steps = min(entries held, capacity) entries, written oldest first at
 * out[k * capacity .. k * capacity + *steps).  A node is the entry's step id and particle count,
 * the ancestor's slot in it and its five values as recorded.  An empty log or capacity 0:
 * ESLAM_OK with *steps = 0.  ESLAM_ERR_INVALID_ARG: a null ctx or steps, null indices or out where
 * they are needed, an index >= the particle count, the log not enabled.
 * eslam_gpu_trajectory_smoothed: for each of the newest *entries = min(entries held, capacity)
 * entries k, oldest first, the fixed-lag smoothed estimate: the pose moments of the ancestors at
 * entry k of the current particles under the current weights.  With a_newest = link and
 * a_{k-1}[i] = parent_k[a_k[i]], out[k].moments is bit for bit what eslam_gpu_pose_moments
 * without a gate gives on n particles whose (x, y, zpos, orientation, zsigma) are those of slot
 * a_k[i] of entry k and whose weight is the current w[i], in the order of i; distinct_ancestors is
 * the number of distinct values of a_k (where it reaches 1 every older entry holds one common
 * ancestor).  Needs particles (ESLAM_ERR_NOT_INITIALISED); an empty log: ESLAM_OK, *entries = 0.
 * Both queries are synchronous, settle and materialise first like eslam_gpu_pose_moments, and
 * change nothing in the filter or the log.                                                    */
typedef struct eslam_trajectory_info {
    uint32_t enabled, capacity_steps;
    uint64_t max_particles;
    uint64_t entries;                 /* entries held                                          */
    uint64_t first_step, last_step;   /* step ids of the oldest and newest held entry (0: none) */
    uint64_t particles;               /* of the newest held entry                              */
    uint64_t bytes;                   /* device memory of the ring and the link arrays         */
} eslam_trajectory_info;
typedef struct eslam_trajectory_pose { uint64_t step; uint32_t slot, particles; double x, y, z, yaw, zsigma; } eslam_trajectory_pose;
typedef struct eslam_trajectory_estimate { uint64_t step; uint64_t distinct_ancestors; eslam_pose_moments moments; } eslam_trajectory_estimate;
int eslam_gpu_trajectory_enable(eslam_ctx* ctx, uint32_t capacity_steps, uint64_t max_particles /* 0: the context's capacity */);
int eslam_gpu_trajectory_enable_sharded(eslam_ctx* ctx, uint32_t capacity_steps, uint64_t max_particles /* per rank; 0: the rank's capacity */);
int eslam_gpu_trajectory_disable(eslam_ctx* ctx);
int eslam_gpu_trajectory_clear(eslam_ctx* ctx);
int eslam_gpu_trajectory_info(eslam_ctx* ctx, eslam_trajectory_info* info);
int eslam_gpu_get_trajectories(eslam_ctx* ctx, const uint64_t* indices, uint64_t count,
                               eslam_trajectory_pose* out /* count x capacity */, uint64_t capacity,
                               uint64_t* steps /* nodes written per index */);
int eslam_gpu_trajectory_smoothed(eslam_ctx* ctx, eslam_trajectory_estimate* out, uint64_t capacity, uint64_t* entries);

/* ---- KLD-sampling (Fox 2003): the particle count the posterior needs --------------------------
 * The reference takes `samples` from its caller (src/ParticleFilter.hpp); the rule is this
 * build's own.  A fixed lattice over (x, y, yaw) is anchored at the world origin;
 * the occupied bins k of the particles as they stand (a deferred exchange is settled and a
 * pending gather run first) are counted on the device, exactly, and the smallest count whose
 * Kullback-Leibler distance to the posterior stays below epsilon with probability 1 - delta is
 * computed on the host.  Everything is fp64 without contraction through eslam_detmath.h
 * (dm_kld_index, dm_kld_bound, dm_kld_samples), so one GPU, a sharded filter and the CPU
 * restatement (tests/c/kld_ref.c) give the same info bit for bit.
 *   counted   x, y, theta and w finite, w > 0, and both cell indices fit an int32; every other
 *             particle is skipped (particles_skipped)
 *   lattice   inv = 1.0 / bin_xy; ix = (int32) floor(x * inv), iy likewise; u = theta *
 *             DM_INV_2PI, u -= floor(u), it = (uint32) floor(u * theta_bins), it == theta_bins
 *             (u rounded to 1.0) wraps to 0
 *   box       origin = the minima of ix and iy over the counted particles (sharded: global),
 *             bins = {nx, ny, theta_bins} with nx = ix1 - ix0 + 1; a particle's bit is
 *             ((iy - iy0) * nx + (ix - ix0)) * theta_bins + it of a bitmap of nx * ny * theta_bins
 *             bits.  More bits than max_bins (0: 2^27 bits, 16 MiB): ESLAM_ERR_UNSUPPORTED ("cloud
 *             too spread for the bin size"), info filled as far as the box, nothing changed
 *   k         bins_occupied, the bitmap's population count
 *   bound     k <= 1: 0.  Else a = 2.0 / (9.0 * (k - 1)), t = (1.0 - a) + sqrt(a) * z_quantile,
 *             bound = ((k - 1) / (2.0 * epsilon)) * t * t * t
 *   samples   ceil(bound), then in this order, each step that applies setting its bit in clamped:
 *             bit 0 raised to n_min; bit 1 cut to n_max (0: none) and to the largest count the
 *             resample accepts (2^32 - 2; sharded 2^30 - 64) -- a non-finite bound or one at or
 *             above 2^63 counts as above both; bit 2 cut to the capacity on a filter with
 *             ESLAM_FLAG_PARTICLE_MAPS; bit 3 held at the current global count n when
 *             |samples - n| <= min_change * n (in fp64)
 * No counted particle: ESLAM_OK, k 0, origin 0, bins {0, 0, theta_bins}, samples from bound 0.
 * eslam_gpu_kld_count changes nothing in the filter (particles, weights, RNG, maps, hash);
 * synchronous; needs particles, no map.
 * eslam_gpu_resample_kld counts, then resamples to info.samples: eslam_gpu_resample_stratified /
 * _multinomial (params->multinomial), on a sharded filter the _sharded calls.  Whatever that
 * resample refuses comes back with its own code and nothing changed (a sharded count with fewer
 * summation chunks than ranks, no memory to grow).  A stratified call at an unchanged count is
 * eslam_gpu_resample.  A sharded filter with ESLAM_FLAG_PARTICLE_MAPS cannot change its count,
 * and the count is known only after the collectives: the call is ESLAM_ERR_UNSUPPORTED before
 * any collective unless n_min == n_max == the current global count.  Both infos may be NULL.
 * ESLAM_ERR_INVALID_ARG (before any launch or collective): a null ctx, params or (kld_count)
 * info; bin_xy not finite or <= 0; theta_bins outside 1..4096; multinomial > 1; epsilon not
 * finite or <= 0; z_quantile not finite or < 0; n_min 0; n_max non-zero and below n_min;
 * min_change negative or NaN.  ESLAM_ERR_NOT_INITIALISED: no particles.
 * Sharded filters: both calls are collectives in SPMD order.  The ranks compare their parameters
 * (one all_gather of host words: a mismatch is ESLAM_ERR_INVALID_ARG on every rank), all-gather
 * the six words of box and counts, agree that every rank has the bitmap's memory, all-gather
 * the bitmaps and OR them.  Every rank gets the one-GPU info bit for bit.                   */
typedef struct eslam_kld_params {
    double bin_xy;        /* metres, finite, > 0                                   */
    uint32_t theta_bins;  /* yaw bins per turn, 1..4096                            */
    uint32_t multinomial; /* 0 stratified, 1 multinomial (eslam_gpu_resample_kld)  */
    double epsilon;       /* KL bound, finite, > 0                                 */
    double z_quantile;    /* upper 1 - delta quantile of N(0,1), finite, >= 0      */
    uint64_t n_min;       /* >= 1                                                  */
    uint64_t n_max;       /* 0 = only the call's own limits; else >= n_min         */
    double min_change;    /* hysteresis, fraction of the current count, >= 0       */
    uint64_t max_bins;    /* bitmap bits; 0 = 2^27                                 */
} eslam_kld_params;
/* 0.1 m, 36 bins, stratified, epsilon 0.05, z 2.3263478740408408 (delta 0.01),
 * n_min = cfg->particle_count (1 when that is 0 or cfg is NULL), n_max 0, min_change 0, max_bins 0 */
void eslam_kld_params_default(const eslam_config* cfg, eslam_kld_params* p);
typedef struct eslam_kld_info {
    uint64_t particles_counted, particles_skipped, bins_occupied;
    int64_t origin[2];    /* ix0, iy0 */
    uint64_t bins[3];     /* nx, ny, theta_bins */
    double bound;
    uint64_t samples;
    uint32_t clamped, pad;
} eslam_kld_info;
int eslam_gpu_kld_count(eslam_ctx* ctx, const eslam_kld_params* params, eslam_kld_info* info);
int eslam_gpu_resample_kld(eslam_ctx* ctx, const eslam_kld_params* params, eslam_kld_info* info /* may be NULL */,
                           eslam_resample_info* rinfo /* may be NULL */);

/* ---- resume state: RNG + the filter scalars (bit-exact resume with the particles) ------- */
typedef struct eslam_rng_state {
    uint32_t minstd_x;                     /* ParticleFilter::rand_gen state                */
    uint32_t pad;
    uint64_t project_count;                /* Philox event counter of project()              */
    uint64_t init_count;
    uint64_t hash_count;
    double max_weight;                     /* PoseEstimator::max_weight                      */
    double ud_pose[12];                    /* EmbodiedSlamFilter::udPose, 3x4 row-major      */
    uint32_t libc_rand[34];                /* SurfaceHash::sample's rand() (glibc TYPE_3)    */
    uint32_t libc_rand_pos;
    uint32_t pad2;
} eslam_rng_state;
int eslam_gpu_get_rng_state(eslam_ctx* ctx, eslam_rng_state* st);
int eslam_gpu_set_rng_state(eslam_ctx* ctx, const eslam_rng_state* st);

/* ---- snapshots: everything a filter needs to continue bit for bit -------------------------
 * One blob (little-endian, layout in DESIGN.md 5e) holds the particles, the RNG state and the
 * scalars the next update reads, the shared grid as the device holds it now, the pose hash,
 * and with ESLAM_FLAG_PARTICLE_MAPS every particle's map: tables and pages under compact ids
 * in a canonical order (tables by the lowest particle naming them, pages by first reference),
 * sharing and page ownership kept.  The bytes depend on the filter's logical state only.
 * The format carries its own version; ESLAM_ABI_VERSION is unchanged.
 *
 * The blob is produced and consumed on the device in chunks of at most chunk_bytes (0: 64 MiB;
 * any value from 4 KiB up; a table row longer than that goes as one chunk), through two pinned
 * and two device staging buffers the context keeps.  A callback returning non-zero ends the
 * call with ESLAM_ERR_COMM.
 *
 * Save first does what eslam_gpu_download_particles does (a pending gather is run), and
 * changes nothing a later step, map update, match, download or counter can see.
 * Load works on a context that was only created (no set_map / init_* / hash_create) and
 * replaces whatever a live one holds.  It checks the header, the section sizes and, on the
 * host, every table and page id before a kernel reads it: ESLAM_ERR_INVALID_ARG for a blob
 * that fails, or whose ESLAM_FLAG_PARTICLE_MAPS bit, window half-widths (max_sensor_range) or
 * local_map_trail differ from the context's; ESLAM_ERR_OUT_OF_MEMORY for more live pages than
 * the context's pool (local_map_pages may differ from the saving context's).  After a failed
 * load the context holds no particles and is not poisoned.  The rest of the configuration is
 * the context's own, as with eslam_gpu_upload_particles.
 * Not carried: the last update's eslam_update_info, the RECORD_CONTACTS records, the
 * ancestors and the kernel times; after a load they read as after upload_particles.
 *
 * Positional forms (eslam_gpu_save_at / eslam_gpu_load_at): the same version-1 blob as one
 * logical file of info->bytes bytes, written and read by offset.  On a one-GPU filter save_at
 * writes every byte of [0, bytes) exactly once, the bytes eslam_gpu_save_stream writes, and
 * load_at is load_stream reading by offset (known_bytes: the file's size when known, else 0).
 *
 * Sharded filters (eslam_gpu_set_comm, any nranks): save_at, load_at, eslam_gpu_snapshot_size
 * and eslam_gpu_load (every rank holds the whole blob) are collectives in SPMD order.  The
 * ranks write one blob between them: rank 0 the header, grid, hash and scalars; every rank its
 * shard of the particle arrays, and its tables and pages behind those of the ranks below it
 * (shards are contiguous and tables and pages are rank-local, so rank-major order is the
 * canonical order).  Without per-particle maps the blob is the one-GPU filter's, byte for byte.
 * With them it differs only in how tables are shared across shard boundaries (a sharded filter
 * keeps one copy per rank), never in what a particle's own map shows.  Any layout loads any
 * blob whose n is its n_global (else ESLAM_ERR_INVALID_ARG, before any collective): each rank
 * reads the shared parts, its shard of the particles, and the tables and pages its particles
 * name; a table named from both sides of a shard boundary is loaded by both ranks.  The page
 * pool check is per rank.  Both calls end with an all_gather of the ranks' return codes:
 * ESLAM_OK on one rank means every rank wrote or loaded its part; a failing rank returns its
 * own code, the others ESLAM_ERR_COMM, and after a failed load every rank holds no particles.
 * info: bytes, particles, tables, pages and sections are the filter's on every rank, chunks
 * counts this rank's callbacks.  eslam_gpu_save, eslam_gpu_save_stream and
 * eslam_gpu_load_stream return ESLAM_ERR_UNSUPPORTED on a sharded filter, before any
 * collective: a sequential stream cannot carry a part of a file.                            */
#define ESLAM_SNAPSHOT_VERSION 1
#define ESLAM_SNAPSHOT_GRID 0x1u
#define ESLAM_SNAPSHOT_HASH 0x2u
#define ESLAM_SNAPSHOT_PARTICLES 0x4u
#define ESLAM_SNAPSHOT_SCALARS 0x8u
#define ESLAM_SNAPSHOT_MAPS 0x10u
typedef struct eslam_snapshot_info {
    uint64_t bytes;                        /* size of the snapshot                          */
    uint64_t particles, tables, pages;     /* distinct live tables / pages written          */
    uint64_t grid_patches, hash_poses, chunks;
    uint32_t version, sections;            /* ESLAM_SNAPSHOT_VERSION; ESLAM_SNAPSHOT_* mask  */
} eslam_snapshot_info;
typedef int (*eslam_write_fn)(void* user, const void* data, uint64_t bytes);  /* 0 = ok */
typedef int (*eslam_read_fn)(void* user, void* data, uint64_t bytes);         /* 0 = ok */
typedef int (*eslam_pwrite_fn)(void* user, uint64_t offset, const void* data, uint64_t bytes); /* 0 = ok */
typedef int (*eslam_pread_fn)(void* user, uint64_t offset, void* data, uint64_t bytes);        /* 0 = ok */

int eslam_gpu_snapshot_size(eslam_ctx* ctx, eslam_snapshot_info* info);
int eslam_gpu_save_stream(eslam_ctx* ctx, eslam_write_fn w, void* user, uint64_t chunk_bytes, eslam_snapshot_info* info);
int eslam_gpu_load_stream(eslam_ctx* ctx, eslam_read_fn r, void* user, uint64_t chunk_bytes, eslam_snapshot_info* info);
/* thin wrappers over the stream forms: capacity below the snapshot's size, or bytes other
 * than the blob's own size, are ESLAM_ERR_INVALID_ARG                                      */
int eslam_gpu_save(eslam_ctx* ctx, void* buf, uint64_t capacity, uint64_t chunk_bytes, eslam_snapshot_info* info);
int eslam_gpu_load(eslam_ctx* ctx, const void* buf, uint64_t bytes, uint64_t chunk_bytes, eslam_snapshot_info* info);
/* the blob by offset; the only forms a sharded filter saves through                          */
extern int eslam_gpu_save_at(eslam_ctx* ctx, eslam_pwrite_fn w, void* user, uint64_t chunk_bytes, eslam_snapshot_info* info);
extern int eslam_gpu_load_at(eslam_ctx* ctx, eslam_pread_fn r, void* user, uint64_t known_bytes /* 0: unknown */,
                             uint64_t chunk_bytes, eslam_snapshot_info* info);

/* ---- SurfaceHash (useHash = true): pose hash of the map by terrain slope ----------------
 * SurfaceHash::create  src/SurfaceHash.hpp:155-231 on the map of eslam_gpu_set_map, with
 * the config's hash_slope_bins / hash_angular_steps (a sweep over segments x cells on the
 * GPU).  eslam_gpu_init_pose builds it on demand when config.hash_use is set and then
 * initialises from it (PoseEstimator::init(N, hash) src/PoseEstimator.cpp:75-86); with
 * hash_use, every hash_period-th project (starting with the first) runs sampleFromHash
 * (src/PoseEstimator.cpp:130-182, 238-240).  rand() is glibc's generator seeded with 1
 * (the reference never seeds it), one state per context.                                  */
int eslam_gpu_hash_create(eslam_ctx* ctx);
/* PoseEstimator::init(N, hash): particle i = a uniformly drawn hash pose                   */
int eslam_gpu_init_hash(eslam_ctx* ctx, uint64_t n);
/* number of hash poses; bucket_sizes (slope_bins^2 entries, bucket = bx * bins + by) or NULL */
int eslam_gpu_hash_info(eslam_ctx* ctx, uint64_t* n_poses, uint32_t* bucket_sizes);
/* the hash poses in sweep order (x, y, theta, z) and their buckets; any pointer may be NULL */
int eslam_gpu_hash_poses(eslam_ctx* ctx, double* x, double* y, double* theta, double* z, int32_t* bucket);

/* ---- multi-GPU: one context per GPU holds a contiguous shard of ONE global filter -------
 * The library is transport-agnostic: it calls the collectives below at the three exchange
 * points of an update.  In production they are torch.distributed over RCCL
 * (xGMI) on device buffers (slam-eslam_amd/eslam_dist.py); tests use gloo on host buffers.
 *   1. all_gather of the exact per-rank weighting statistics (~0.5 KB per rank)
 *      -> every rank finalises the same global floating weight, weight sum, effective N
 *   2. all_gather of the per-rank fixed-point weight totals (8 B per rank)
 *      -> global cumulative-sum offsets for the stratified draws
 *   3. all_gather of the per-destination send counts + all_to_all_v of the particles
 *      whose stratified draws land on another rank (72-byte records)
 * Results are bit-identical to the single-GPU run of the same global filter.          */
typedef struct eslam_comm {
    void* user;
    int32_t rank, nranks;
    int32_t device_memory;                 /* 1: callbacks take device pointers (RCCL)     */
    int32_t pad;
    /* recv[r * bytes .. (r+1) * bytes) <- send of rank r.  stream: the context's HIP
     * stream when device_memory (the collective is ordered after the work already on it
     * and work queued after the call returns must see its result), NULL otherwise.        */
    int (*allgather)(void* user, const void* send, void* recv, uint64_t bytes, void* stream);
    /* send_bytes[r] bytes to rank r (packed in rank order), recv_bytes[r] from rank r    */
    int (*alltoallv)(void* user, const void* send, const uint64_t* send_bytes, void* recv,
                     const uint64_t* recv_bytes, void* stream);
} eslam_comm;

/* Make this context shard [gbase, gbase + n_local) of an n_global-particle filter; call
 * before init.  shard_gbase lists the first global index of every rank (nranks + 1
 * entries, strictly increasing, last = n_global <= 2^30 - 64); every entry must be a multiple
 * of 64 * dm_chunk_rows_cfg(n_global, sum_chunk_rows) (the canonical summation chunk) except the last.
 * The context's config particle_count is the global count.  Sharded contexts support
 * the hot path (step/project/update/sync), init, upload/download of the local shard,
 * weights sum / normalise / resample, the best particle (global index), the centroid, the
 * hash respawn, per-particle maps and the merge into the shared map
 * (eslam_gpu_shared_map_update_sharded), each equal to one GPU bit for bit.  comm == NULL
 * returns the context to one GPU.
 * Calls on a sharded filter follow SPMD order: every rank makes the same sequence of
 * calls that update, write, normalise, resample or reduce (they run collectives).  The
 * rank-local getters (download, records, particle maps, particle grids, RNG state, hash poses) may be
 * called by any subset of ranks: the only collective they can run is the previous
 * update's deferred exchange, which every rank completes exactly once -- in a getter, in
 * its next collective call or in eslam_gpu_finish -- so the ranks stay matched.         */
int eslam_gpu_set_comm(eslam_ctx* ctx, const eslam_comm* comm, uint64_t n_global, const uint64_t* shard_gbase);

/* ---- multi-GPU over RCCL, driven from the library (no callback into the host language) --
 * SURVEY.md 8(b) "comm_init(nranks, rank, ncclUniqueId*)"; the reference has one CPU
 * filter and no distribution (src/EmbodiedSlamFilter.hpp:29-39 owns it by value).
 * eslam_gpu_rccl_unique_id: rank 0 creates the 128-byte RCCL id (ncclGetUniqueId) that the
 * caller broadcasts to every rank by any means.  eslam_gpu_set_comm_rccl: every rank then
 * joins the communicator (ncclCommInitRank, collective: all ranks must call it) and the
 * context becomes shard `rank` exactly as eslam_gpu_set_comm makes it; the exchanges are
 * ncclAllGather and grouped ncclSend/ncclRecv on the context's stream.  RCCL is loaded at
 * run time (librccl.so.1); without it these return ESLAM_ERR_UNSUPPORTED.                 */
#define ESLAM_RCCL_ID_BYTES 128
int eslam_gpu_rccl_unique_id(uint8_t id[ESLAM_RCCL_ID_BYTES]);
int eslam_gpu_set_comm_rccl(eslam_ctx* ctx, int32_t nranks, int32_t rank, const uint8_t id[ESLAM_RCCL_ID_BYTES],
                            uint64_t n_global, const uint64_t* shard_gbase);

/* ---- diagnostics ------------------------------------------------------------------------- */
/* ancestor index of every particle of the last resample (needs ESLAM_FLAG_RECORD_ANCESTORS) */
int eslam_gpu_get_ancestors(eslam_ctx* ctx, uint32_t* out, uint64_t n);
/* per-kernel timing of the last step, milliseconds (HIP events on the context stream)     */
typedef struct eslam_kernel_times {
    float project_weight_ms;
    float finalize_ms;
    float normalize_scan_ms;
    float resample_ms;
    float total_ms;
    /* eslam_gpu_map_update (per-particle maps), averaged over the map updates of the timed
     * region: the pending resample gather (sharded filters; one GPU fuses it into the merge),
     * the tables' sharing classes and the free-table list (copy on write's bookkeeping), the
     * plan (k_map_plan, the page budget and, when the free pages run short, the collection),
     * the merge kernel with its counters, and the whole call                               */
    float map_gather_ms;
    float map_cow_ms;
    float map_merge_ms;
    float map_total_ms;
    float map_plan_ms;
    /* eslam_gpu_map_match (ABI 6): the call's gather and k_map_match, averaged over the
     * matches of the timed region                                                         */
    float map_match_ms;
} eslam_kernel_times;
int eslam_gpu_enable_timing(eslam_ctx* ctx, int enable);
int eslam_gpu_get_kernel_times(eslam_ctx* ctx, eslam_kernel_times* t);
/* evaluate the deterministic math on the device for n inputs (tests/test_gpu_math.py):
 * fn: 0 exp, 1 log, 2 sin, 3 cos, 4 erfc, 5 sqrt, 6 div(x, y), 7 pdf/cdf ratio(x, y),
 *     8 pow(x, y), 9 fx61(x) as bits, 13 sin(2 pi x), 14 cos(2 pi x) (Box-Muller angle),
 *     20..25: the butterflies' lane exchange, out[i] = x[i ^ 2^(fn - 20)] (n a multiple of 256) */
int eslam_gpu_selftest_math(int device, int fn, const double* x, const double* y, double* out, uint64_t n);
/* the Box-Muller radius sqrt(-2 log u) with the range-restricted dm_log_pos / dm_sqrt_pos
 * against the general dm_log / dm_sqrt, on the device, for all 2^32 uniform words: the
 * number of words whose results differ in any bit (0 expected)                           */
int eslam_gpu_selftest_bm_radius(int device, uint64_t* mismatches);
/* the device's stable radix sort of (key, value) pairs (the hash respawn's select order)  */
int eslam_gpu_selftest_sort(int device, const uint32_t* keys, const uint32_t* vals, uint64_t n, uint32_t* keys_out,
                            uint32_t* vals_out);

#ifdef __cplusplus
}
#endif
#endif /* ESLAM_GPU_H */
