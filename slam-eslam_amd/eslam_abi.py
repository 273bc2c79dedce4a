"""ctypes mirror of include/eslam_gpu.h (the C ABI of the MI355X eSLAM core).

Shared by the product wrapper (eslam_amd.py), the tests and bench.py.  Field order and
types must match the header exactly; tests/test_abi.py checks sizes against the C compiler.
"""
import ctypes as C

MAX_CONTACTS = 32

OK = 0
ERR_INVALID_ARG = -1
ERR_NO_ENVIRONMENT = -2
ERR_ZERO_MEAS_VAR = -3
ERR_HASH_SAMPLE = -4
ERR_NO_MLS_GRID = -5
ERR_HIP = -6
ERR_NOT_INITIALISED = -7
ERR_UNSUPPORTED = -8
ERR_OUT_OF_MEMORY = -9
ERR_COMM = -10

FLAG_RECORD_ANCESTORS = 0x1
FLAG_NO_MAP_LDS = 0x2
FLAG_NO_AUX_GATHER = 0x4
FLAG_RECORD_CONTACTS = 0x8
FLAG_PARTICLE_MAPS = 0x10
FLAG_PROCESS_STATICS = 0x20


class Config(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64),
        ("particle_count", C.c_uint64),
        ("min_effective", C.c_uint64),
        ("initial_rotation_error", C.c_double * 3),
        ("initial_translation_error", C.c_double * 3),
        ("measurement_error", C.c_double),
        ("discount_factor", C.c_double),
        ("spread_threshold", C.c_double),
        ("spread_translation_factor", C.c_double),
        ("spread_rotation_factor", C.c_double),
        ("slip_factor", C.c_double),
        ("max_yaw_deviation", C.c_double),
        ("measurement_threshold_distance", C.c_double),
        ("measurement_threshold_angle", C.c_double),
        ("use_slip_update", C.c_int32),
        ("use_shape_update", C.c_int32),
        ("min_contacts", C.c_uint64),
        ("contact_likelihood_correction", C.c_double),
        ("contact_point_radius", C.c_double),
        ("hash_use", C.c_int32),
        ("hash_period", C.c_uint64),
        ("hash_percentage", C.c_double),
        ("hash_avg_factor", C.c_double),
        ("hash_slope_bins", C.c_uint64),
        ("hash_angular_steps", C.c_uint64),
        ("log_debug", C.c_int32),
        ("flags", C.c_uint32),
        ("local_map_pages", C.c_uint32),
        ("max_sensor_range", C.c_double),
        ("local_map_trail", C.c_uint32),
        ("sum_chunk_rows", C.c_uint32),
    ]


class MlsGrid(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("scale_x", C.c_double),
        ("scale_y", C.c_double),
        ("offset_x", C.c_double),
        ("offset_y", C.c_double),
        ("global2local", C.c_double * 12),
        ("cell_start", C.POINTER(C.c_uint32)),
        ("patch_mean", C.POINTER(C.c_float)),
        ("patch_stdev", C.POINTER(C.c_float)),
        ("patch_height", C.POINTER(C.c_float)),
        ("n_patches", C.c_uint64),
    ]


class ContactPoint(C.Structure):
    _fields_ = [
        ("position", C.c_double * 3),
        ("contact", C.c_float),
        ("group_id", C.c_int32),
    ]


class StepInput(C.Structure):
    _fields_ = [
        ("body2odometry_rot", C.c_double * 4),
        ("body2odometry_trans", C.c_double * 3),
        ("pose_delta_trans", C.c_double * 3),
        ("position_error_zz", C.c_double),
        ("sample_mean", C.c_double * 3),
        ("sample_cov", C.c_double * 9),
        ("n_contacts", C.c_uint32),
        ("ltc_count", C.c_uint32),
        ("contacts", ContactPoint * MAX_CONTACTS),
    ]


class Particles(C.Structure):
    _fields_ = [
        ("x", C.POINTER(C.c_double)),
        ("y", C.POINTER(C.c_double)),
        ("orientation", C.POINTER(C.c_double)),
        ("zpos", C.POINTER(C.c_double)),
        ("zsigma", C.POINTER(C.c_double)),
        ("weight", C.POINTER(C.c_double)),
        ("mprob", C.POINTER(C.c_double)),
        ("floating", C.POINTER(C.c_uint8)),
        ("n_contact_points", C.POINTER(C.c_uint8)),
    ]


class ScanPatch(C.Structure):
    """eslam_scan_patch: one cell of the scan MLS merged by a map update"""
    _fields_ = [
        ("position", C.c_double * 3),
        ("stdev", C.c_double),
    ]


class SharedMergeInfo(C.Structure):
    """eslam_shared_merge_info: the counters of eslam_gpu_shared_map_update"""
    _fields_ = [
        ("particles_done", C.c_uint64),
        ("patches_placed", C.c_uint64),
        ("patches_off_grid", C.c_uint64),
        ("cells_touched", C.c_uint64),
        ("fused", C.c_uint64),
        ("absorbed", C.c_uint64),
        ("inserted", C.c_uint64),
        ("n_patches", C.c_uint64),
        ("runs", C.c_uint64),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class ScanParams(C.Structure):
    """eslam_scan_params: how a sensor reading becomes the scan MLS"""
    _fields_ = [
        ("sensor2body", C.c_double * 12),
        ("orientation", C.c_double * 4),
        ("sensor_rot_sigma", C.c_double * 3),
        ("body_rot_sigma", C.c_double * 3),
        ("min_sigma", C.c_double),
        ("resolution", C.c_double),
        ("patch_thickness", C.c_double),
        ("max_sensor_range", C.c_double),
    ]


class LaserScan(C.Structure):
    """eslam_laser_scan: base::samples::LaserScan (ranges in millimetres)"""
    _fields_ = [
        ("start_angle", C.c_double),
        ("angular_resolution", C.c_double),
        ("min_range", C.c_uint32),
        ("max_range", C.c_uint32),
        ("n", C.c_uint32),
        ("pad", C.c_uint32),
        ("ranges", C.POINTER(C.c_uint32)),
    ]


class DepthImage(C.Structure):
    """eslam_depth_image: base::samples::DistanceImage (row-major float metres)"""
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("scale_x", C.c_double),
        ("scale_y", C.c_double),
        ("center_x", C.c_double),
        ("center_y", C.c_double),
        ("data", C.POINTER(C.c_float)),
    ]


class ScanInfo(C.Structure):
    """eslam_scan_info: the counters of eslam_gpu_scan_from_laser / _depth"""
    _fields_ = [
        ("points", C.c_uint64),
        ("points_valid", C.c_uint64),
        ("points_invalid", C.c_uint64),
        ("points_out_of_range", C.c_uint64),
        ("cells", C.c_uint64),
        ("patches", C.c_uint64),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


def laser_scan(ranges, start_angle, angular_resolution, min_range, max_range):
    """(eslam_laser_scan, the uint32 array it points into -- keep it alive)"""
    import numpy as np
    r = np.ascontiguousarray(ranges, dtype=np.uint32)
    s = LaserScan()
    s.start_angle, s.angular_resolution = float(start_angle), float(angular_resolution)
    s.min_range, s.max_range, s.n = int(min_range), int(max_range), int(r.size)
    s.ranges = r.ctypes.data_as(C.POINTER(C.c_uint32))
    return s, r


def depth_image(data, scale_x, scale_y, center_x, center_y):
    """(eslam_depth_image of a (height, width) float array, the float32 array it points into)"""
    import numpy as np
    d = np.ascontiguousarray(data, dtype=np.float32)
    im = DepthImage()
    im.height, im.width = (int(d.shape[0]), int(d.shape[1])) if d.ndim == 2 else (0, 0)
    im.scale_x, im.scale_y, im.center_x, im.center_y = float(scale_x), float(scale_y), float(center_x), float(center_y)
    im.data = d.ctypes.data_as(C.POINTER(C.c_float))
    return im, d


class CPoint(C.Structure):
    """eslam_cpoint: ContactPoint (src/PoseParticle.hpp:20-43)"""
    _fields_ = [
        ("point", C.c_double * 3),
        ("zdiff", C.c_double),
        ("zvar", C.c_double),
        ("prob", C.c_double),
    ]


class ParticleRecord(C.Structure):
    """eslam_particle_record: PoseParticle with its debug fields (src/PoseParticle.hpp:52-86)"""
    _fields_ = [
        ("position", C.c_double * 2),
        ("orientation", C.c_double),
        ("zpos", C.c_double),
        ("zsigma", C.c_double),
        ("mprob", C.c_double),
        ("weight", C.c_double),
        ("meas_pos", C.c_double * 3),
        ("meas_theta", C.c_double),
        ("index", C.c_uint64),
        ("n_cpoints", C.c_uint32),
        ("floating", C.c_uint8),
        ("pad", C.c_uint8 * 3),
    ]


class UpdateInfo(C.Structure):
    _fields_ = [
        ("effective", C.c_double),
        ("weight_sum", C.c_double),
        ("floating_weight", C.c_double),
        ("max_weight", C.c_double),
        ("data_particles", C.c_uint64),
        ("total_points", C.c_uint64),
        ("resampled", C.c_int32),
        ("uniform_reset", C.c_int32),
        ("resample_overruns", C.c_uint64),
        ("update_count", C.c_uint64),
        ("map_patches_dropped", C.c_uint64),
        ("map_stores_copied", C.c_uint64),
        ("map_stores_changed", C.c_uint64),
        ("map_patches_covered", C.c_uint64),
        ("map_cells_written", C.c_uint64),
        ("map_pages_taken", C.c_uint64),
        ("map_pages_free", C.c_uint64),
        ("map_tiles_evicted", C.c_uint64),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class ResampleInfo(C.Structure):
    """eslam_resample_info (include/eslam_gpu.h)."""
    _fields_ = [
        ("n_before", C.c_uint64),
        ("n_after", C.c_uint64),
        ("overruns", C.c_uint64),
        ("dropped", C.c_uint64),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


GMM_MAX_COMPONENTS = 8


class GmmParams(C.Structure):
    """eslam_gmm_params (include/eslam_gpu.h)."""
    _fields_ = [
        ("components", C.c_uint32),
        ("max_iterations", C.c_uint32),
        ("tolerance", C.c_double),
        ("min_variance", C.c_double),
    ]


class GmmComponent(C.Structure):
    """eslam_gmm_component: weight, mean (x, y), covariance (xx, xy, yy)."""
    _fields_ = [
        ("weight", C.c_double),
        ("mean", C.c_double * 2),
        ("cov", C.c_double * 3),
    ]


class GmmInfo(C.Structure):
    """eslam_gmm_info (include/eslam_gpu.h)."""
    _fields_ = [
        ("components_live", C.c_uint32),
        ("iterations", C.c_uint32),
        ("converged", C.c_uint32),
        ("live_mask", C.c_uint32),
        ("particles_used", C.c_uint64),
        ("particles_skipped", C.c_uint64),
        ("log_likelihood", C.c_double),
        ("centre", C.c_double * 2),
        ("weight_exp", C.c_int32),
    ]

    def as_dict(self):
        return {f: (list(getattr(self, f)) if f == "centre" else getattr(self, f)) for f, _ in self._fields_}


class PoseGate(C.Structure):
    """eslam_pose_gate: the ellipse (p - centre)^T cov^-1 (p - centre) <= chi2 over p = (x, y); cov as xx, xy, yy."""
    _fields_ = [
        ("centre", C.c_double * 2),
        ("cov", C.c_double * 3),
        ("chi2", C.c_double),
    ]

    def __init__(self, centre=(0.0, 0.0), cov=(1.0, 0.0, 1.0), chi2=9.0):
        super().__init__((C.c_double * 2)(*centre), (C.c_double * 3)(*cov), chi2)


class PoseMoments(C.Structure):
    """eslam_pose_moments (include/eslam_gpu.h)."""
    _fields_ = [
        ("particles_counted", C.c_uint64),
        ("particles_gated_out", C.c_uint64),
        ("particles_skipped", C.c_uint64),
        ("mean", C.c_double * 4),
        ("cov", C.c_double * 16),
        ("z_within", C.c_double),
        ("yaw_resultant", C.c_double),
        ("effective", C.c_double),
        ("weight_share", C.c_double),
        ("weight_exp", C.c_int32),
        ("pad", C.c_int32),
    ]

    def as_dict(self):
        return {f: (list(getattr(self, f)) if f in ("mean", "cov") else getattr(self, f)) for f, _ in self._fields_}

    def doubles(self):
        """the 24 doubles in the struct's order"""
        return list(self.mean) + list(self.cov) + [self.z_within, self.yaw_resultant, self.effective, self.weight_share]

    def as_tuple(self):
        """every field, the doubles as their bits (NaN compares equal to itself)"""
        import struct
        d = self.doubles()
        return (self.particles_counted, self.particles_gated_out, self.particles_skipped) + \
            struct.unpack(f"<{len(d)}Q", struct.pack(f"<{len(d)}d", *d)) + (self.weight_exp, self.pad)


class KldParams(C.Structure):
    """eslam_kld_params (include/eslam_gpu.h); the defaults are eslam_kld_params_default's but for
    n_min, which that takes from the configuration."""
    _fields_ = [
        ("bin_xy", C.c_double),
        ("theta_bins", C.c_uint32),
        ("multinomial", C.c_uint32),
        ("epsilon", C.c_double),
        ("z_quantile", C.c_double),
        ("n_min", C.c_uint64),
        ("n_max", C.c_uint64),
        ("min_change", C.c_double),
        ("max_bins", C.c_uint64),
    ]

    def __init__(self, bin_xy=0.1, theta_bins=36, multinomial=0, epsilon=0.05, z_quantile=2.3263478740408408, n_min=1,
                 n_max=0, min_change=0.0, max_bins=0):
        super().__init__(bin_xy, theta_bins, multinomial, epsilon, z_quantile, n_min, n_max, min_change, max_bins)


class KldInfo(C.Structure):
    """eslam_kld_info (include/eslam_gpu.h)."""
    _fields_ = [
        ("particles_counted", C.c_uint64),
        ("particles_skipped", C.c_uint64),
        ("bins_occupied", C.c_uint64),
        ("origin", C.c_int64 * 2),
        ("bins", C.c_uint64 * 3),
        ("bound", C.c_double),
        ("samples", C.c_uint64),
        ("clamped", C.c_uint32),
        ("pad", C.c_uint32),
    ]

    def as_dict(self):
        return {f: (list(getattr(self, f)) if f in ("origin", "bins") else getattr(self, f)) for f, _ in self._fields_}

    def as_tuple(self):
        """every field, the bound as its bits (NaN compares equal to itself)"""
        import struct
        return (self.particles_counted, self.particles_skipped, self.bins_occupied, tuple(self.origin), tuple(self.bins),
                struct.unpack("<Q", struct.pack("<d", self.bound))[0], self.samples, self.clamped, self.pad)


class TrajectoryInfo(C.Structure):
    """eslam_trajectory_info (include/eslam_gpu.h).  On a sharded filter's log
    (eslam_gpu_trajectory_enable_sharded) `particles` is the newest entry's global count, while
    `max_particles` and `bytes` are this rank's."""
    _fields_ = [
        ("enabled", C.c_uint32),
        ("capacity_steps", C.c_uint32),
        ("max_particles", C.c_uint64),
        ("entries", C.c_uint64),
        ("first_step", C.c_uint64),
        ("last_step", C.c_uint64),
        ("particles", C.c_uint64),
        ("bytes", C.c_uint64),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class TrajectoryPose(C.Structure):
    """eslam_trajectory_pose: a lineage's node in one entry of the log."""
    _fields_ = [
        ("step", C.c_uint64),
        ("slot", C.c_uint32),
        ("particles", C.c_uint32),
        ("x", C.c_double),
        ("y", C.c_double),
        ("z", C.c_double),
        ("yaw", C.c_double),
        ("zsigma", C.c_double),
    ]


class TrajectoryEstimate(C.Structure):
    """eslam_trajectory_estimate: an entry's smoothed estimate."""
    _fields_ = [
        ("step", C.c_uint64),
        ("distinct_ancestors", C.c_uint64),
        ("moments", PoseMoments),
    ]


class RngState(C.Structure):
    _fields_ = [
        ("minstd_x", C.c_uint32),
        ("pad", C.c_uint32),
        ("project_count", C.c_uint64),
        ("init_count", C.c_uint64),
        ("hash_count", C.c_uint64),
        ("max_weight", C.c_double),
        ("ud_pose", C.c_double * 12),
        ("libc_rand", C.c_uint32 * 34),
        ("libc_rand_pos", C.c_uint32),
        ("pad2", C.c_uint32),
    ]


class KernelTimes(C.Structure):
    _fields_ = [
        ("project_weight_ms", C.c_float),
        ("finalize_ms", C.c_float),
        ("normalize_scan_ms", C.c_float),
        ("resample_ms", C.c_float),
        ("total_ms", C.c_float),
        ("map_gather_ms", C.c_float),
        ("map_cow_ms", C.c_float),
        ("map_merge_ms", C.c_float),
        ("map_total_ms", C.c_float),
        ("map_plan_ms", C.c_float),
        ("map_match_ms", C.c_float),
    ]


SNAPSHOT_VERSION = 1
SNAPSHOT_GRID, SNAPSHOT_HASH, SNAPSHOT_PARTICLES, SNAPSHOT_SCALARS, SNAPSHOT_MAPS = 0x1, 0x2, 0x4, 0x8, 0x10


class SnapshotInfo(C.Structure):
    """eslam_snapshot_info (include/eslam_gpu.h)."""
    _fields_ = [
        ("bytes", C.c_uint64),
        ("particles", C.c_uint64),
        ("tables", C.c_uint64),
        ("pages", C.c_uint64),
        ("grid_patches", C.c_uint64),
        ("hash_poses", C.c_uint64),
        ("chunks", C.c_uint64),
        ("version", C.c_uint32),
        ("sections", C.c_uint32),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)     # eslam_write_fn
READ_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)      # eslam_read_fn

# the snapshot entry points of include/eslam_gpu.h (after the eslam_ctx*): name -> argument types
SNAPSHOT_PROTOTYPES = {
    "eslam_gpu_snapshot_size": [C.POINTER(SnapshotInfo)],
    "eslam_gpu_save_stream": [WRITE_FN, C.c_void_p, C.c_uint64, C.POINTER(SnapshotInfo)],
    "eslam_gpu_load_stream": [READ_FN, C.c_void_p, C.c_uint64, C.POINTER(SnapshotInfo)],
    "eslam_gpu_save": [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(SnapshotInfo)],
    "eslam_gpu_load": [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(SnapshotInfo)],
}

# eslam_pwrite_fn / eslam_pread_fn: (user, offset, data, bytes)
PWRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64)
PREAD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64)

# the positional forms (one file written and read by offset; what a sharded filter saves through)
SNAPSHOT_AT_PROTOTYPES = {
    "eslam_gpu_save_at": [PWRITE_FN, C.c_void_p, C.c_uint64, C.POINTER(SnapshotInfo)],
    "eslam_gpu_load_at": [PREAD_FN, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(SnapshotInfo)],
}

ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p,
                           C.POINTER(C.c_uint64), C.c_void_p)


class Comm(C.Structure):
    """eslam_comm (include/eslam_gpu.h)."""
    _fields_ = [
        ("user", C.c_void_p),
        ("rank", C.c_int32), ("nranks", C.c_int32),
        ("device_memory", C.c_int32), ("pad", C.c_int32),
        ("allgather", ALLGATHER_FN),
        ("alltoallv", ALLTOALLV_FN),
    ]


MAX_RANKS = 16


CHUNK_WAVES, CHUNK_CAP = 5120, 13


def chunk_rows(n_global, fixed=0):
    """dm_chunk_rows_cfg (include/eslam_detmath.h): rows of 64 lanes per canonical summation
    chunk -- eslam_config.sum_chunk_rows when set (`fixed`), else sized to whole generations of
    the weighting kernel's resident waves."""
    if fixed:
        return int(fixed)
    rows = (n_global + 63) // 64
    per = CHUNK_WAVES * CHUNK_CAP
    slots = (1 if rows <= per else -(-rows // per)) * CHUNK_WAVES
    return max(1, -(-rows // slots))


def shard_bounds(n_global, nranks, fixed=0):
    """First global index of every rank (+ n_global): near-equal shards whose starts are
    multiples of the summation chunk (64 * chunk_rows; `fixed`: eslam_config.sum_chunk_rows),
    as eslam_gpu_set_comm requires."""
    csz = 64 * chunk_rows(n_global, fixed)
    chunks = -(-n_global // csz)
    if chunks < nranks:
        raise ValueError(f"{n_global} particles cannot be split into {nranks} chunk-aligned shards")
    g = [min(n_global, (chunks * r // nranks) * csz) for r in range(nranks)] + [n_global]
    if any(g[r + 1] <= g[r] for r in range(nranks)):
        raise ValueError("empty shard")
    return g


SHARD_BOUNDS_ARGTYPES = [C.c_uint64, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]


def shard_bounds_c(lib, n_global, nranks, fixed=0):
    """eslam_gpu_shard_bounds of a loaded library: shard_bounds in C (what a resample of a sharded
    filter to another count lays the filter out by).  ValueError where shard_bounds raises."""
    if nranks < 1:
        raise ValueError("nranks must be at least 1")
    fn = lib.eslam_gpu_shard_bounds
    fn.argtypes = SHARD_BOUNDS_ARGTYPES
    fn.restype = C.c_int
    out = (C.c_uint64 * (nranks + 1))()
    rc = fn(n_global, nranks, fixed, out)
    if rc != 0:
        raise ValueError(f"{n_global} particles cannot be split into {nranks} chunk-aligned shards ({rc})")
    return [int(v) for v in out]


def default_config(lib=None):
    """eslam_config_default() restated (src/Configuration.hpp:85-111 defaults)."""
    import math
    c = Config()
    c.seed = 42
    c.particle_count = 250
    c.min_effective = 50
    c.initial_rotation_error[:] = [0.0, 0.0, 0.1]
    c.initial_translation_error[:] = [0.1, 0.1, 1.0]
    c.measurement_error = 0.1
    c.discount_factor = 0.9
    c.spread_threshold = 0.9
    c.spread_translation_factor = 0.1
    c.spread_rotation_factor = 0.05
    c.slip_factor = 0.05
    c.max_yaw_deviation = 15 * math.pi / 180.0
    c.measurement_threshold_distance = 0.1
    c.measurement_threshold_angle = 10 * math.pi / 180.0
    c.use_slip_update = 0
    c.use_shape_update = 1
    c.min_contacts = 3
    c.contact_likelihood_correction = 0.33
    c.contact_point_radius = 0.01
    c.hash_use = 0
    c.hash_period = 10
    c.hash_percentage = 0.05
    c.hash_avg_factor = 0.1
    c.hash_slope_bins = 20
    c.hash_angular_steps = 16
    c.log_debug = 0
    c.flags = 0
    c.local_map_pages = 0
    c.max_sensor_range = 3.0
    c.local_map_trail = 16
    c.sum_chunk_rows = 0
    return c


# ---------------------------------------------------------------------------------------
# numpy helpers
# ---------------------------------------------------------------------------------------
def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


class ParticleArrays:
    """Host SoA buffers + the eslam_particles view onto them."""

    def __init__(self, n):
        import numpy as np
        self.n = n
        self.x = np.zeros(n)
        self.y = np.zeros(n)
        self.orientation = np.zeros(n)
        self.zpos = np.zeros(n)
        self.zsigma = np.zeros(n)
        self.weight = np.zeros(n)
        self.mprob = np.zeros(n)
        self.floating = np.zeros(n, dtype=np.uint8)
        self.n_contact_points = np.zeros(n, dtype=np.uint8)

    def view(self):
        p = Particles()
        for f in ("x", "y", "orientation", "zpos", "zsigma", "weight", "mprob"):
            setattr(p, f, _ptr(getattr(self, f), C.c_double))
        p.floating = _ptr(self.floating, C.c_uint8)
        p.n_contact_points = _ptr(self.n_contact_points, C.c_uint8)
        return p

    FIELDS = ("x", "y", "orientation", "zpos", "zsigma", "weight", "mprob", "floating", "n_contact_points")

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}


class GridArrays:
    """An MLS grid held in numpy arrays + the eslam_mls_grid view onto them."""

    def __init__(self, width, height, scale, offset, cell_start, mean, stdev, height_arr=None,
                 global2local=None):
        import numpy as np
        self.width, self.height = int(width), int(height)
        self.scale = (float(scale[0]), float(scale[1]))
        self.offset = (float(offset[0]), float(offset[1]))
        self.cell_start = np.ascontiguousarray(cell_start, dtype=np.uint32)
        self.mean = np.ascontiguousarray(mean, dtype=np.float32)
        self.stdev = np.ascontiguousarray(stdev, dtype=np.float32)
        self.patch_height = None if height_arr is None else np.ascontiguousarray(height_arr, dtype=np.float32)
        self.g2l = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0] if global2local is None else list(global2local)
        assert self.cell_start.shape[0] == self.width * self.height + 1
        assert int(self.cell_start[-1]) == self.mean.shape[0] == self.stdev.shape[0]

    def view(self):
        g = MlsGrid()
        g.width, g.height = self.width, self.height
        g.scale_x, g.scale_y = self.scale
        g.offset_x, g.offset_y = self.offset
        g.global2local[:] = self.g2l
        g.cell_start = _ptr(self.cell_start, C.c_uint32)
        g.patch_mean = _ptr(self.mean, C.c_float)
        g.patch_stdev = _ptr(self.stdev, C.c_float)
        g.patch_height = None if self.patch_height is None else _ptr(self.patch_height, C.c_float)
        g.n_patches = int(self.mean.shape[0])
        return g
