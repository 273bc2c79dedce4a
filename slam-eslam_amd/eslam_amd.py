"""Python binding of libeslam_gpu.so (the MI355X eSLAM core) through its C ABI.

This is the host-side mirror of the reference's API for tests and benchmarks:
``EmbodiedSlamFilter`` (src/EmbodiedSlamFilter.hpp:58-74) and the ``PoseEstimator`` /
``ParticleFilter<T>`` calls it forwards (src/PoseEstimator.hpp:123-134,
src/ParticleFilter.hpp:34-173).  Every call goes to the GPU; there is no CPU fallback --
a missing library or GPU raises.
"""
import ctypes as C
import os

import numpy as np

import eslam_abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ESLAM_GPU_LIB", os.path.join(HERE, "lib", "libeslam_gpu.so"))

_lib = None


class EslamError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def build_id():
    """SHA-256 of the sources the loaded library was built from (eslam_gpu_build_id)."""
    return load_library().eslam_gpu_build_id().decode()


def load_library(path=LIB_PATH):
    """Load libeslam_gpu.so and declare every entry point of include/eslam_gpu.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"libeslam_gpu.so not built ({path}); run __graft_entry__.build()")
    L = C.CDLL(path)
    L.eslam_gpu_build_id.restype = C.c_char_p
    if "ESLAM_GPU_LIB" not in os.environ:
        # the in-tree library must be the build of these sources (build_lib.source_hash)
        import build_lib
        want, got = build_lib.source_hash(), L.eslam_gpu_build_id().decode()
        if got != want:
            raise RuntimeError(f"{path} was built from other sources (build id {got[:12]}, sources {want[:12]}); "
                               "run __graft_entry__.build()")
    vp = C.c_void_p
    dp = C.POINTER(C.c_double)
    L.eslam_config_default.argtypes = [C.POINTER(A.Config)]
    L.eslam_config_default.restype = None
    L.eslam_gpu_abi_version.restype = C.c_int
    L.eslam_gpu_create.argtypes = [C.POINTER(A.Config), C.c_int, C.POINTER(vp)]
    L.eslam_gpu_destroy.argtypes = [vp]
    L.eslam_gpu_destroy.restype = None
    L.eslam_gpu_finish.argtypes = [vp]
    L.eslam_gpu_last_error.argtypes = [vp]
    L.eslam_gpu_last_error.restype = C.c_char_p
    L.eslam_gpu_set_stream.argtypes = [vp, vp]
    L.eslam_gpu_set_map.argtypes = [vp, C.POINTER(A.MlsGrid)]
    L.eslam_gpu_init_gaussian.argtypes = [vp, C.c_uint64, dp, dp, C.c_double, C.c_double]
    L.eslam_gpu_init_pose.argtypes = [vp, dp, dp]
    L.eslam_gpu_upload_particles.argtypes = [vp, C.c_uint64, C.POINTER(A.Particles)]
    L.eslam_gpu_download_particles.argtypes = [vp, C.POINTER(A.Particles)]
    L.eslam_gpu_write_particles.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(A.Particles)]
    L.eslam_gpu_map_update.argtypes = [vp, C.POINTER(A.ScanPatch), C.c_uint32]
    if hasattr(L, "eslam_gpu_map_match"):                 # absent from older builds (A/B runs)
        L.eslam_gpu_map_match.argtypes = [vp, C.POINTER(A.ScanPatch), C.c_uint32]
    if hasattr(L, "eslam_gpu_shared_map_update"):        # absent from older builds (A/B runs)
        L.eslam_gpu_shared_map_update.argtypes = [vp, C.POINTER(A.ScanPatch), C.c_uint32, C.c_uint64,
                                                  C.POINTER(A.SharedMergeInfo)]
        L.eslam_gpu_map_size.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_int)]
        L.eslam_gpu_get_map.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.POINTER(C.c_float), C.c_uint64]
    if hasattr(L, "eslam_gpu_shared_map_update_sharded"):   # absent from older builds (A/B runs)
        L.eslam_gpu_shared_map_update_sharded.argtypes = [vp, C.POINTER(A.ScanPatch), C.c_uint32, C.c_uint64,
                                                          C.POINTER(A.SharedMergeInfo)]
    if hasattr(L, "eslam_gpu_scan_from_laser"):          # absent from older builds (A/B runs)
        L.eslam_scan_params_default.argtypes = [C.POINTER(A.Config), C.POINTER(A.ScanParams)]
        L.eslam_gpu_scan_from_laser.argtypes = [vp, C.POINTER(A.LaserScan), C.POINTER(A.ScanParams), C.POINTER(A.ScanInfo)]
        L.eslam_gpu_scan_from_depth.argtypes = [vp, C.POINTER(A.DepthImage), C.POINTER(A.ScanParams), C.POINTER(A.ScanInfo)]
        L.eslam_gpu_scan_patches.argtypes = [vp, C.POINTER(A.ScanPatch), C.c_uint64, C.POINTER(C.c_uint64)]
    L.eslam_gpu_set_particle_maps.argtypes = [vp, C.c_int]
    L.eslam_gpu_get_particle_map.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                             C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]
    if hasattr(L, "eslam_gpu_get_particle_grid"):        # absent from older builds (A/B runs)
        L.eslam_gpu_particle_grid_size.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.eslam_gpu_get_particle_grid.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint64]
        L.eslam_gpu_adopt_particle_map.argtypes = [vp, C.c_uint64]
    L.eslam_gpu_download_records.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(A.ParticleRecord),
                                             C.POINTER(A.CPoint), C.c_uint32]
    L.eslam_gpu_particle_count.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.eslam_gpu_step.argtypes = [vp, C.POINTER(A.StepInput), C.POINTER(C.c_int)]
    L.eslam_gpu_project.argtypes = [vp, C.POINTER(A.StepInput)]
    L.eslam_gpu_update.argtypes = [vp, C.POINTER(A.StepInput)]
    L.eslam_gpu_sync.argtypes = [vp, C.POINTER(A.UpdateInfo)]
    if hasattr(L, "eslam_gpu_set_min_effective"):        # absent from older builds (A/B runs)
        L.eslam_gpu_set_min_effective.argtypes = [vp, C.c_uint64]
    if hasattr(L, "eslam_gpu_debug_set_spin_limit"):     # absent from older builds (A/B runs)
        L.eslam_gpu_debug_set_spin_limit.argtypes = [vp, C.c_uint32]
    if hasattr(L, "eslam_gpu_debug_set_scan_items"):     # absent from older builds (A/B runs)
        L.eslam_gpu_debug_set_scan_items.argtypes = [vp, C.c_uint32]
    L.eslam_gpu_get_weights_sum.argtypes = [vp, dp]
    L.eslam_gpu_normalize_weights.argtypes = [vp, dp]
    L.eslam_gpu_resample.argtypes = [vp]
    L.eslam_gpu_resample_stratified.argtypes = [vp, C.c_uint64, C.POINTER(A.ResampleInfo)]
    L.eslam_gpu_resample_multinomial.argtypes = [vp, C.c_uint64, C.POINTER(A.ResampleInfo)]
    # a library without them is an error at the call
    if hasattr(L, "eslam_gpu_resample_stratified_sharded"):
        L.eslam_gpu_resample_stratified_sharded.argtypes = [vp, C.c_uint64, C.POINTER(A.ResampleInfo)]
        L.eslam_gpu_resample_multinomial_sharded.argtypes = [vp, C.c_uint64, C.POINTER(A.ResampleInfo)]
        L.eslam_gpu_shard_bounds.argtypes = A.SHARD_BOUNDS_ARGTYPES
        L.eslam_gpu_get_shard_bounds.argtypes = [vp, C.POINTER(C.c_uint64), C.c_uint32]
    L.eslam_gpu_get_best_particle_index.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.eslam_gpu_get_centroid.argtypes = [vp, dp, dp]
    # a library without it is an error at the call
    if hasattr(L, "eslam_gpu_fit_pose_gmm"):
        L.eslam_gmm_params_default.argtypes = [C.POINTER(A.GmmParams)]
        L.eslam_gmm_params_default.restype = None
        L.eslam_gpu_fit_pose_gmm.argtypes = [vp, C.POINTER(A.GmmParams), C.POINTER(A.GmmComponent), C.POINTER(A.GmmInfo)]
    if hasattr(L, "eslam_gpu_pose_moments"):
        L.eslam_gpu_pose_moments.argtypes = [vp, C.POINTER(A.PoseGate), C.POINTER(A.PoseMoments)]
    # a library without them is an error at the call
    if hasattr(L, "eslam_gpu_kld_count"):
        L.eslam_kld_params_default.argtypes = [C.POINTER(A.Config), C.POINTER(A.KldParams)]
        L.eslam_kld_params_default.restype = None
        L.eslam_gpu_kld_count.argtypes = [vp, C.POINTER(A.KldParams), C.POINTER(A.KldInfo)]
        L.eslam_gpu_resample_kld.argtypes = [vp, C.POINTER(A.KldParams), C.POINTER(A.KldInfo), C.POINTER(A.ResampleInfo)]
    # a library without them is an error at the call
    if hasattr(L, "eslam_gpu_trajectory_enable"):
        L.eslam_gpu_trajectory_enable.argtypes = [vp, C.c_uint32, C.c_uint64]
        L.eslam_gpu_trajectory_disable.argtypes = [vp]
        L.eslam_gpu_trajectory_clear.argtypes = [vp]
        L.eslam_gpu_trajectory_info.argtypes = [vp, C.POINTER(A.TrajectoryInfo)]
        L.eslam_gpu_get_trajectories.argtypes = [vp, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(A.TrajectoryPose), C.c_uint64,
                                                 C.POINTER(C.c_uint64)]
        L.eslam_gpu_trajectory_smoothed.argtypes = [vp, C.POINTER(A.TrajectoryEstimate), C.c_uint64, C.POINTER(C.c_uint64)]
    if hasattr(L, "eslam_gpu_trajectory_enable_sharded"):
        L.eslam_gpu_trajectory_enable_sharded.argtypes = [vp, C.c_uint32, C.c_uint64]
    L.eslam_gpu_get_rng_state.argtypes = [vp, C.POINTER(A.RngState)]
    L.eslam_gpu_set_rng_state.argtypes = [vp, C.POINTER(A.RngState)]
    L.eslam_gpu_get_ancestors.argtypes = [vp, C.POINTER(C.c_uint32), C.c_uint64]
    L.eslam_gpu_enable_timing.argtypes = [vp, C.c_int]
    L.eslam_gpu_get_kernel_times.argtypes = [vp, C.POINTER(A.KernelTimes)]
    L.eslam_gpu_selftest_math.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.c_uint64]
    up = C.POINTER(C.c_uint32)
    L.eslam_gpu_selftest_sort.argtypes = [C.c_int, up, up, C.c_uint64, up, up]
    if hasattr(L, "eslam_gpu_selftest_bm_radius"):       # absent from older builds (A/B runs)
        L.eslam_gpu_selftest_bm_radius.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
    L.eslam_gpu_set_comm.argtypes = [vp, C.POINTER(A.Comm), C.c_uint64, C.POINTER(C.c_uint64)]
    L.eslam_gpu_rccl_unique_id.argtypes = [C.POINTER(C.c_uint8)]
    L.eslam_gpu_set_comm_rccl.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_uint64,
                                          C.POINTER(C.c_uint64)]
    L.eslam_gpu_hash_create.argtypes = [vp]
    L.eslam_gpu_init_hash.argtypes = [vp, C.c_uint64]
    L.eslam_gpu_hash_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.eslam_gpu_hash_poses.argtypes = [vp, dp, dp, dp, dp, C.POINTER(C.c_int32)]
    # a library without them is an error at the call
    for name, args in {**A.SNAPSHOT_PROTOTYPES, **A.SNAPSHOT_AT_PROTOTYPES}.items():
        if hasattr(L, name):
            getattr(L, name).argtypes = [vp] + args
    _lib = L
    return L


def _dv(v):
    return (C.c_double * len(v))(*v)


_SNAP_HEADER = 336


class _SnapshotGrid:
    """The grid geometry in a snapshot's header: what get_map() needs of the
    GridArrays a set_map() would have left."""

    def __init__(self, head):
        d = np.frombuffer(head[64:192], "<f8")
        self.scale = (float(d[0]), float(d[1]))
        self.offset = (float(d[2]), float(d[3]))
        self.g2l = [float(v) for v in d[4:16]]


class GpuFilter:
    """One eslam_ctx: the PoseEstimator / EmbodiedSlamFilter of one GPU."""

    def __init__(self, cfg=None, device=0):
        self.L = load_library()
        self.cfg = cfg if cfg is not None else A.default_config()
        h = C.c_void_p()
        rc = self.L.eslam_gpu_create(C.byref(self.cfg), device, C.byref(h))
        if rc != 0:
            raise EslamError(rc, f"eslam_gpu_create failed ({rc}) -- is an MI355X visible?")
        self.h = h
        self._grid = None

    def close(self):
        if getattr(self, "h", None):
            self.L.eslam_gpu_destroy(self.h)
            self.h = None

    def finish(self):
        """eslam_gpu_finish: collective on a sharded filter (completes an exchange still owed)."""
        if getattr(self, "h", None):
            self._check(self.L.eslam_gpu_finish(self.h))

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise EslamError(rc, self.L.eslam_gpu_last_error(self.h).decode())
        return rc

    # -- environment / init -------------------------------------------------------------
    def set_map(self, grid):
        self._grid = grid
        g = grid.view()
        self._check(self.L.eslam_gpu_set_map(self.h, C.byref(g)))

    def init_gaussian(self, n, mu, sigma, zpos, zsigma):
        self._check(self.L.eslam_gpu_init_gaussian(self.h, n, _dv(mu), _dv(sigma), zpos, zsigma))

    def init_pose(self, position, orientation):
        self._check(self.L.eslam_gpu_init_pose(self.h, _dv(position), _dv(orientation)))

    def upload(self, pa):
        v = pa.view()
        self._check(self.L.eslam_gpu_upload_particles(self.h, pa.n, C.byref(v)))

    def download(self):
        n = self.count()
        pa = A.ParticleArrays(n)
        v = pa.view()
        self._check(self.L.eslam_gpu_download_particles(self.h, C.byref(v)))
        return pa

    def write(self, first, pa):
        """eslam_gpu_write_particles: particles [first, first + pa.n) take pa's fields (a
        collective on a sharded filter: every rank calls it, pa.n may be 0)"""
        v = pa.view()
        self._check(self.L.eslam_gpu_write_particles(self.h, first, pa.n, C.byref(v)))

    def download_records(self, first=0, stride=1, count=None, max_cpoints=0):
        """eslam_gpu_download_records: particles first + k * stride as PoseParticle records
        (numpy structured array) and, with max_cpoints, their contact points
        (count x max_cpoints eslam_cpoint, numpy structured)."""
        n = self.count()
        if count is None:
            count = 0 if first >= n else (n - 1 - first) // max(stride, 1) + 1
        recs = (A.ParticleRecord * max(count, 1))()
        cps = (A.CPoint * max(count * max_cpoints, 1))() if max_cpoints else None
        self._check(self.L.eslam_gpu_download_records(self.h, first, stride, count, recs, cps, max_cpoints))
        r = np.ctypeslib.as_array(recs)[:count].copy()
        c = np.ctypeslib.as_array(cps)[:count * max_cpoints].reshape(count, max_cpoints).copy() if max_cpoints else None
        return r, c

    def set_particle_maps(self, on=True):
        """PoseEstimator::setEnvironment(..., useShared=not on) before init: per-particle maps"""
        self._check(self.L.eslam_gpu_set_particle_maps(self.h, 1 if on else 0))

    def map_update(self, patches):
        """eslam_gpu_map_update: processMap's merge of a scan into every particle's map"""
        self._check(self.L.eslam_gpu_map_update(self.h, patches, len(patches)))

    def map_match(self, patches):
        """eslam_gpu_map_match: processMap's visual weighting (match = true) against each
        particle's map: the shared grid, or its own map (per-particle maps)"""
        self._check(self.L.eslam_gpu_map_match(self.h, patches, len(patches)))

    def shared_map_update(self, patches, max_records=0):
        """eslam_gpu_shared_map_update: processMap's merge of a scan into the shared grid, once
        per particle in index order (useSharedMap = true); returns the SharedMergeInfo.  On an
        error the EslamError carries the counters of the runs merged before it (`.info`)."""
        info = A.SharedMergeInfo()
        rc = self.L.eslam_gpu_shared_map_update(self.h, patches, len(patches), max_records, C.byref(info))
        if rc != 0:
            e = EslamError(rc, self.L.eslam_gpu_last_error(self.h).decode())
            e.info = info
            raise e
        return info

    def shared_map_update_sharded(self, patches, max_records=0):
        """eslam_gpu_shared_map_update_sharded: the same merge on a sharded filter, in global
        particle order into every rank's copy of the grid.  A collective: every rank passes the
        same scan and max_records.  On a filter that is not sharded it is shared_map_update."""
        info = A.SharedMergeInfo()
        rc = self.L.eslam_gpu_shared_map_update_sharded(self.h, patches, len(patches), max_records, C.byref(info))
        if rc != 0:
            e = EslamError(rc, self.L.eslam_gpu_last_error(self.h).decode())
            e.info = info
            raise e
        return info

    def scan_params(self):
        """eslam_scan_params_default for this filter's configuration (A.ScanParams)"""
        p = A.ScanParams()
        self.L.eslam_scan_params_default(C.byref(self.cfg), C.byref(p))
        return p

    def scan_patches(self):
        """eslam_gpu_scan_patches: the last built scan (a ctypes array of eslam_scan_patch, as the
        map updates take it)"""
        n = C.c_uint64()
        self._check(self.L.eslam_gpu_scan_patches(self.h, None, 0, C.byref(n)))
        out = (A.ScanPatch * n.value)()
        if n.value:
            self._check(self.L.eslam_gpu_scan_patches(self.h, out, n.value, C.byref(n)))
        return out

    def scan_from_laser(self, ranges, start_angle, angular_resolution, min_range, max_range, params=None):
        """eslam_gpu_scan_from_laser: the scan MLS of a laser scan (ranges: uint32 millimetres),
        built on the device; returns (ScanPatch array, ScanInfo).  params: A.ScanParams
        (default: scan_params())."""
        s, _keep = A.laser_scan(ranges, start_angle, angular_resolution, min_range, max_range)
        p = params if params is not None else self.scan_params()
        info = A.ScanInfo()
        self._check(self.L.eslam_gpu_scan_from_laser(self.h, C.byref(s), C.byref(p), C.byref(info)))
        return self.scan_patches(), info

    def scan_from_depth(self, data, scale_x, scale_y, center_x, center_y, params=None):
        """eslam_gpu_scan_from_depth: the scan MLS of a distance image (data: (height, width)
        float metres), built on the device; returns (ScanPatch array, ScanInfo)."""
        im, _keep = A.depth_image(data, scale_x, scale_y, center_x, center_y)
        p = params if params is not None else self.scan_params()
        info = A.ScanInfo()
        self._check(self.L.eslam_gpu_scan_from_depth(self.h, C.byref(im), C.byref(p), C.byref(info)))
        return self.scan_patches(), info

    def get_map(self):
        """eslam_gpu_get_map: the shared grid as the device holds it (GridArrays with the
        geometry of the grid given to set_map)"""
        if self._grid is None:
            raise EslamError(A.ERR_NO_ENVIRONMENT, "No environment attached.")
        w, h, n, hh = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_int()
        self._check(self.L.eslam_gpu_map_size(self.h, C.byref(w), C.byref(h), C.byref(n), C.byref(hh)))
        cells = np.zeros(w.value * h.value + 1, np.uint32)
        mean = np.zeros(n.value, np.float32)
        sd = np.zeros(n.value, np.float32)
        hgt = np.zeros(n.value, np.float32) if hh.value else None
        fp = C.POINTER(C.c_float)
        self._check(self.L.eslam_gpu_get_map(self.h, cells.ctypes.data_as(C.POINTER(C.c_uint32)), mean.ctypes.data_as(fp),
                                             sd.ctypes.data_as(fp), hgt.ctypes.data_as(fp) if hh.value else None, n.value))
        g = self._grid
        return A.GridArrays(w.value, h.value, g.scale, g.offset, cells, mean, sd, hgt, g.g2l)

    def particle_map(self, i, cap=1024):
        """particle i's own patches: (cells, mean, stdev), tiles in slot order, cells row by row"""
        while True:
            cells = np.zeros(cap, np.uint32)
            mean = np.zeros(cap, np.float32)
            sd = np.zeros(cap, np.float32)
            c = C.c_uint32()
            self._check(self.L.eslam_gpu_get_particle_map(self.h, i, cells.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                          mean.ctypes.data_as(C.POINTER(C.c_float)),
                                                          sd.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(c)))
            if c.value <= cap:
                return cells[:c.value], mean[:c.value], sd[:c.value]
            cap = c.value

    def particle_grid(self, i, capacity=None):
        """eslam_gpu_get_particle_grid: particles[i].grid.getMap(), particle i's whole map (its
        own patch per cell, then the shared grid's) composed on the device, as GridArrays with
        the shared grid's geometry: what set_map() takes.  capacity: the patch arrays' size
        (default: eslam_gpu_particle_grid_size)."""
        if self._grid is None:
            raise EslamError(A.ERR_NO_ENVIRONMENT, "No environment attached.")
        w, h, hh, n = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_uint64()
        self._check(self.L.eslam_gpu_map_size(self.h, C.byref(w), C.byref(h), None, C.byref(hh)))
        self._check(self.L.eslam_gpu_particle_grid_size(self.h, i, C.byref(n)))
        cap = n.value if capacity is None else capacity
        cells = np.zeros(w.value * h.value + 1, np.uint32)
        mean = np.zeros(max(cap, 1), np.float32)
        sd = np.zeros(max(cap, 1), np.float32)
        hgt = np.zeros(max(cap, 1), np.float32) if hh.value else None
        fp = C.POINTER(C.c_float)
        self._check(self.L.eslam_gpu_get_particle_grid(self.h, i, cells.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                       mean.ctypes.data_as(fp), sd.ctypes.data_as(fp),
                                                       hgt.ctypes.data_as(fp) if hh.value else None, cap))
        g, k = self._grid, n.value
        return A.GridArrays(w.value, h.value, g.scale, g.offset, cells, mean[:k], sd[:k], hgt[:k] if hh.value else None, g.g2l)

    def adopt_particle_map(self, i):
        """eslam_gpu_adopt_particle_map: continue in particle i's map, as set_map(particle_grid(i))
        without the host round trip: it becomes the shared grid and every particle's own map
        starts over, empty"""
        self._check(self.L.eslam_gpu_adopt_particle_map(self.h, i))

    def count(self):
        n = C.c_uint64()
        self._check(self.L.eslam_gpu_particle_count(self.h, C.byref(n)))
        return n.value

    # -- SurfaceHash ----------------------------------------------------------------------
    def hash_create(self):
        self._check(self.L.eslam_gpu_hash_create(self.h))

    def init_hash(self, n):
        self._check(self.L.eslam_gpu_init_hash(self.h, n))

    def hash_info(self):
        n = C.c_uint64()
        bins = self.cfg.hash_slope_bins
        sizes = np.zeros(bins * bins, dtype=np.uint32)
        self._check(self.L.eslam_gpu_hash_info(self.h, C.byref(n), sizes.ctypes.data_as(C.POINTER(C.c_uint32))))
        return n.value, sizes

    def hash_poses(self):
        n, _ = self.hash_info()
        out = [np.zeros(n) for _ in range(4)]
        bucket = np.zeros(n, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._check(self.L.eslam_gpu_hash_poses(self.h, *[ptr(a) for a in out], bucket.ctypes.data_as(C.POINTER(C.c_int32))))
        return out + [bucket]

    # -- hot path -------------------------------------------------------------------------
    def step(self, st):
        u = C.c_int(0)
        self._check(self.L.eslam_gpu_step(self.h, C.byref(st), C.byref(u)))
        return bool(u.value)

    def project(self, st):
        self._check(self.L.eslam_gpu_project(self.h, C.byref(st)))

    def update(self, st):
        self._check(self.L.eslam_gpu_update(self.h, C.byref(st)))

    def sync(self):
        info = A.UpdateInfo()
        self._check(self.L.eslam_gpu_sync(self.h, C.byref(info)))
        return info

    def set_min_effective(self, min_effective):
        """eslam_gpu_set_min_effective: Configuration::minEffective from the next update on (0: no
        update resamples; above the particle count: every update does)."""
        self._check(self.L.eslam_gpu_set_min_effective(self.h, min_effective))
        self.cfg.min_effective = min_effective

    def debug_set_spin_limit(self, polls):
        """Testing only: polls of K3's cross-block waits before they give up (0: at once)."""
        self._check(self.L.eslam_gpu_debug_set_spin_limit(self.h, polls))

    def debug_set_scan_items(self, items):
        """Testing only: particles per thread of the one-GPU resample scan (1, 2, 4 or 8; 0: the
        rule by particle count).  The tile size never changes a result."""
        self._check(self.L.eslam_gpu_debug_set_scan_items(self.h, items))

    # -- ParticleFilter API ----------------------------------------------------------------
    def weights_sum(self):
        s = C.c_double()
        self._check(self.L.eslam_gpu_get_weights_sum(self.h, C.byref(s)))
        return s.value

    def normalize(self):
        e = C.c_double()
        self._check(self.L.eslam_gpu_normalize_weights(self.h, C.byref(e)))
        return e.value

    def resample(self):
        self._check(self.L.eslam_gpu_resample(self.h))

    def resample_stratified(self, samples):
        """eslam_gpu_resample_stratified: resample_stratified(samples), to any count (weights
        carried); returns the ResampleInfo"""
        info = A.ResampleInfo()
        self._check(self.L.eslam_gpu_resample_stratified(self.h, samples, C.byref(info)))
        return info

    def resample_multinomial(self, samples):
        """eslam_gpu_resample_multinomial: resample_multinomial(samples); draws beyond the weight
        sum are dropped, every weight becomes 1 / n_before; returns the ResampleInfo"""
        info = A.ResampleInfo()
        self._check(self.L.eslam_gpu_resample_multinomial(self.h, samples, C.byref(info)))
        return info

    def resample_stratified_sharded(self, samples):
        """eslam_gpu_resample_stratified_sharded: resample_stratified(samples) on a sharded filter,
        to any count.  A collective: every rank passes the same samples.  Afterwards the filter is
        sharded by shard_bounds_c(n_after, nranks) (get_shard_bounds).  On a filter that is not
        sharded it is resample_stratified.  Returns the ResampleInfo (global counts)."""
        info = A.ResampleInfo()
        self._check(self.L.eslam_gpu_resample_stratified_sharded(self.h, samples, C.byref(info)))
        return info

    def resample_multinomial_sharded(self, samples):
        """eslam_gpu_resample_multinomial_sharded: resample_multinomial(samples) on a sharded
        filter (see resample_stratified_sharded); n_after is samples less the dropped draws."""
        info = A.ResampleInfo()
        self._check(self.L.eslam_gpu_resample_multinomial_sharded(self.h, samples, C.byref(info)))
        return info

    def get_shard_bounds(self):
        """eslam_gpu_get_shard_bounds: the sharded filter's current table, nranks + 1 entries"""
        out = (C.c_uint64 * (A.MAX_RANKS + 1))()
        self._check(self.L.eslam_gpu_get_shard_bounds(self.h, out, A.MAX_RANKS + 1))
        b = [int(v) for v in out]
        return b[:b.index(max(b)) + 1]

    def best_index(self):
        i = C.c_uint64()
        self._check(self.L.eslam_gpu_get_best_particle_index(self.h, C.byref(i)))
        return i.value

    def centroid(self):
        p = (C.c_double * 3)()
        q = (C.c_double * 4)()
        self._check(self.L.eslam_gpu_get_centroid(self.h, p, q))
        return list(p), list(q)

    def fit_pose_gmm(self, components=3, max_iterations=10, tolerance=1e-5, min_variance=1e-6):
        """eslam_gpu_fit_pose_gmm: the 2-D Gaussian mixture over the particles' (x, y) by EM on the
        device; the filter is unchanged.  Returns (weights[K], means[K, 2],
        covs[K, 3] as xx, xy, yy, GmmInfo) in slab order, dead components as zeros.  A collective
        on a sharded filter."""
        p = A.GmmParams(components, max_iterations, tolerance, min_variance)
        out = (A.GmmComponent * max(int(components), 1))()
        info = A.GmmInfo()
        self._check(self.L.eslam_gpu_fit_pose_gmm(self.h, C.byref(p), out, C.byref(info)))
        k = int(components)
        weights = np.array([out[i].weight for i in range(k)], dtype=np.float64)
        means = np.array([list(out[i].mean) for i in range(k)], dtype=np.float64).reshape(k, 2)
        covs = np.array([list(out[i].cov) for i in range(k)], dtype=np.float64).reshape(k, 3)
        return weights, means, covs, info

    def pose_moments(self, gate=None):
        """eslam_gpu_pose_moments: the pose estimate -- the weighted mean of (x, y, z), the circular
        mean of the yaw -- with its 4 x 4 covariance, summed on the device; the
        filter is unchanged.  gate: None, or a PoseGate whose ellipse selects the particles
        counted.  Returns the PoseMoments.  A collective on a sharded filter."""
        out = A.PoseMoments()
        self._check(self.L.eslam_gpu_pose_moments(self.h, None if gate is None else C.byref(gate), C.byref(out)))
        return out

    def kld_params(self, **params):
        """eslam_kld_params_default for this filter's configuration (n_min = its particle_count),
        then the given fields"""
        p = A.KldParams()
        self.L.eslam_kld_params_default(C.byref(self.cfg), C.byref(p))
        for k, v in params.items():
            if k not in dict(A.KldParams._fields_):
                raise TypeError(f"eslam_kld_params has no field {k!r}")
            setattr(p, k, v)
        return p

    def kld_count(self, **params):
        """eslam_gpu_kld_count: the occupied bins of the pose lattice, counted on the device, and
        the particle count KLD-sampling asks for; the filter is unchanged.  params:
        fields of eslam_kld_params over kld_params()'s defaults.  Returns the KldInfo; an
        EslamError carries what the call filled in as .info.  A collective on a sharded filter."""
        p = self.kld_params(**params)
        info = A.KldInfo()
        try:
            self._check(self.L.eslam_gpu_kld_count(self.h, C.byref(p), C.byref(info)))
        except EslamError as e:
            e.info = info
            raise
        return info

    def resample_kld(self, **params):
        """eslam_gpu_resample_kld: kld_count, then the resample to its count (stratified, or
        multinomial=1).  Returns (KldInfo, ResampleInfo); an EslamError carries the KldInfo as
        .info.  A collective on a sharded filter."""
        p = self.kld_params(**params)
        info, rinfo = A.KldInfo(), A.ResampleInfo()
        try:
            self._check(self.L.eslam_gpu_resample_kld(self.h, C.byref(p), C.byref(info), C.byref(rinfo)))
        except EslamError as e:
            e.info = info
            raise
        return info, rinfo

    # -- the trajectory log ------------------------------------------------------
    def trajectory_enable(self, capacity_steps, max_particles=0):
        """eslam_gpu_trajectory_enable: from now on every step and update ends with a record of
        the particles' poses and ancestry in a ring of capacity_steps entries on the device, each
        with room for max_particles (0: the filter's capacity) particles."""
        self._check(self.L.eslam_gpu_trajectory_enable(self.h, capacity_steps, max_particles))

    def trajectory_enable_sharded(self, capacity_steps, max_particles=0):
        """eslam_gpu_trajectory_enable_sharded: the log of a sharded filter, a collective called by
        every rank with the same capacity_steps after the communicator is set.  max_particles is
        per rank (0: the rank's capacity).  From then on trajectories() takes global particle
        indices and, like trajectory_smoothed(), returns on every rank what one filter holding all
        the particles returns.  On a filter that is not sharded: trajectory_enable."""
        self._check(self.L.eslam_gpu_trajectory_enable_sharded(self.h, capacity_steps, max_particles))

    def trajectory_disable(self):
        """eslam_gpu_trajectory_disable: frees the log"""
        self._check(self.L.eslam_gpu_trajectory_disable(self.h))

    def trajectory_clear(self):
        """eslam_gpu_trajectory_clear: empties the log, which stays enabled"""
        self._check(self.L.eslam_gpu_trajectory_clear(self.h))

    def trajectory_info(self):
        info = A.TrajectoryInfo()
        self._check(self.L.eslam_gpu_trajectory_info(self.h, C.byref(info)))
        return info

    TRAJECTORY_NODE = np.dtype([("step", "<u8"), ("slot", "<u4"), ("particles", "<u4"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8"),
                                ("yaw", "<f8"), ("zsigma", "<f8")])

    def trajectories(self, indices, capacity=None):
        """eslam_gpu_get_trajectories: the lineages of the current particles `indices` through the
        newest min(entries held, capacity) entries (capacity None: all held).  Returns a structured
        array (len(indices), steps) of TRAJECTORY_NODE, oldest entry first."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        cap = self.trajectory_info().entries if capacity is None else int(capacity)
        assert C.sizeof(A.TrajectoryPose) == self.TRAJECTORY_NODE.itemsize
        out = np.zeros((len(idx), max(cap, 1)), dtype=self.TRAJECTORY_NODE)
        steps = C.c_uint64()
        self._check(self.L.eslam_gpu_get_trajectories(self.h, idx.ctypes.data_as(C.POINTER(C.c_uint64)), len(idx),
                                                      out.ctypes.data_as(C.POINTER(A.TrajectoryPose)), cap, C.byref(steps)))
        return out[:, :steps.value] if cap else out[:, :0]

    def trajectory_smoothed(self, capacity=None):
        """eslam_gpu_trajectory_smoothed: per held entry (the newest `capacity`; None: all), oldest
        first, the pose moments of the current particles' ancestors in it under the current weights
        and the number of distinct ancestors.  Returns a list of TrajectoryEstimate."""
        cap = self.trajectory_info().entries if capacity is None else int(capacity)
        out = (A.TrajectoryEstimate * max(cap, 1))()
        entries = C.c_uint64()
        self._check(self.L.eslam_gpu_trajectory_smoothed(self.h, out, cap, C.byref(entries)))
        return [out[k] for k in range(entries.value)]

    def ancestors(self):
        n = self.count()
        out = np.zeros(n, dtype=np.uint32)
        self._check(self.L.eslam_gpu_get_ancestors(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out

    def rng_state(self):
        s = A.RngState()
        self._check(self.L.eslam_gpu_get_rng_state(self.h, C.byref(s)))
        return s

    def set_rng_state(self, s):
        self._check(self.L.eslam_gpu_set_rng_state(self.h, C.byref(s)))

    # -- snapshots -------------------------------------------------------------
    def snapshot_info(self):
        """eslam_gpu_snapshot_size: the size and counts of the snapshot a save would write now"""
        info = A.SnapshotInfo()
        self._check(self.L.eslam_gpu_snapshot_size(self.h, C.byref(info)))
        return info

    def save_state(self, chunk_bytes=0, file=None):
        """eslam_gpu_save: the whole filter as one blob (np.ndarray[uint8]); with `file` (an
        object with write()) the chunks go to it through eslam_gpu_save_stream instead and the
        SnapshotInfo is returned.  `last_snapshot` holds the call's SnapshotInfo."""
        info = A.SnapshotInfo()
        if file is None:
            size = self.snapshot_info().bytes
            blob = np.zeros(size, np.uint8)
            self._check(self.L.eslam_gpu_save(self.h, blob.ctypes.data_as(C.c_void_p), size, chunk_bytes, C.byref(info)))
            self.last_snapshot = info
            return blob
        failed = []

        def write(_user, data, nbytes):
            try:
                file.write(C.string_at(data, nbytes))
                return 0
            except Exception as e:           # the C side reports ESLAM_ERR_COMM
                failed.append(e)
                return 1

        cb = A.WRITE_FN(write)
        rc = self.L.eslam_gpu_save_stream(self.h, cb, None, chunk_bytes, C.byref(info))
        if rc != 0:
            e = EslamError(rc, self.L.eslam_gpu_last_error(self.h).decode())
            e.__cause__ = failed[0] if failed else None
            raise e
        self.last_snapshot = info
        return info

    def load_state(self, blob=None, chunk_bytes=0, file=None):
        """eslam_gpu_load: replace whatever the filter holds by a snapshot (bytes, bytearray or a
        uint8 array; or `file`, an object with read(), through eslam_gpu_load_stream).  Works on
        a filter that was only created.  Returns the SnapshotInfo."""
        info = A.SnapshotInfo()
        if file is None:
            a = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if not isinstance(blob, np.ndarray) else blob, dtype=np.uint8)
            rc = self.L.eslam_gpu_load(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], chunk_bytes, C.byref(info))
            head = a[:_SNAP_HEADER].tobytes()
        else:
            heads = []

            def read(_user, data, nbytes):
                try:
                    b = file.read(nbytes)
                    if len(b) != nbytes:
                        return 1
                    if not heads:
                        heads.append(b)
                    C.memmove(data, b, nbytes)
                    return 0
                except Exception:
                    return 1

            cb = A.READ_FN(read)
            rc = self.L.eslam_gpu_load_stream(self.h, cb, None, chunk_bytes, C.byref(info))
            head = heads[0] if heads else b""
        if rc != 0:
            self._grid = None
            raise EslamError(rc, self.L.eslam_gpu_last_error(self.h).decode())
        self._grid = _SnapshotGrid(head)     # the geometry get_map() reports
        self.last_snapshot = info
        return info

    def save_state_at(self, path, chunk_bytes=0):
        """eslam_gpu_save_at into the file at `path`, opened without truncation and written with
        os.pwrite: on a sharded filter a collective, every rank writing its part of the one file.
        After a successful save every rank sets the file's size to the blob's (info.bytes), so an
        older, longer file at `path` is cut to it.  Returns the SnapshotInfo."""
        info = A.SnapshotInfo()
        failed = []
        fd = os.open(path, os.O_WRONLY | os.O_CREAT, 0o644)

        def pwrite(_user, offset, data, nbytes):
            try:
                b = C.string_at(data, nbytes)
                done = 0
                while done < nbytes:
                    done += os.pwrite(fd, b[done:], offset + done)
                return 0
            except Exception as e:           # the C side reports ESLAM_ERR_COMM
                failed.append(e)
                return 1

        try:
            rc = self.L.eslam_gpu_save_at(self.h, A.PWRITE_FN(pwrite), None, chunk_bytes, C.byref(info))
            if rc == 0:
                os.ftruncate(fd, info.bytes)     # the file is the blob (any rank may do this, at any time)
        finally:
            os.close(fd)
        if rc != 0:
            e = EslamError(rc, self.L.eslam_gpu_last_error(self.h).decode())
            e.__cause__ = failed[0] if failed else None
            raise e
        self.last_snapshot = info
        return info

    def load_state_at(self, path, chunk_bytes=0):
        """eslam_gpu_load_at from the file at `path`, read with os.pread: on a sharded filter a
        collective, every rank reading the shared parts and its own slice of the rest.  Returns
        the SnapshotInfo."""
        info = A.SnapshotInfo()
        fd = os.open(path, os.O_RDONLY)
        heads = []

        def pread(_user, offset, data, nbytes):
            try:
                b = bytearray()
                while len(b) < nbytes:
                    part = os.pread(fd, nbytes - len(b), offset + len(b))
                    if not part:
                        return 1
                    b += part
                if offset == 0 and not heads:
                    heads.append(bytes(b[:_SNAP_HEADER]))
                C.memmove(data, bytes(b), nbytes)
                return 0
            except Exception:
                return 1

        try:
            rc = self.L.eslam_gpu_load_at(self.h, A.PREAD_FN(pread), None, os.fstat(fd).st_size, chunk_bytes, C.byref(info))
        finally:
            os.close(fd)
        if rc != 0:
            self._grid = None
            raise EslamError(rc, self.L.eslam_gpu_last_error(self.h).decode())
        self._grid = _SnapshotGrid(heads[0])
        self.last_snapshot = info
        return info

    def enable_timing(self, on=True):
        self._check(self.L.eslam_gpu_enable_timing(self.h, 1 if on else 0))

    def kernel_times(self):
        t = A.KernelTimes()
        self._check(self.L.eslam_gpu_get_kernel_times(self.h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in t._fields_}


def selftest_math(fn, x, y=None, device=0):
    L = load_library()
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    yp = None
    if y is not None:
        y = np.ascontiguousarray(y, dtype=np.float64)
        yp = y.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.eslam_gpu_selftest_math(device, fn, x.ctypes.data_as(C.POINTER(C.c_double)), yp,
                                   out.ctypes.data_as(C.POINTER(C.c_double)), x.shape[0])
    if rc != 0:
        raise EslamError(rc, "selftest_math failed")
    return out
