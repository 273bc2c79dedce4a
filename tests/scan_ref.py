"""The CPU reference of the scan MLS build (tests/c/scan_ref.c): built with gcc into
tests/c/_build/ (git-ignored) and bound with ctypes, and the readings the scan tests share --
test infrastructure."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
import eslam_abi as A  # noqa: E402

SRC = os.path.join(ROOT, "tests", "c", "scan_ref.c")
LIB_PATH = os.path.join(ROOT, "tests", "c", "_build", "libscan_ref.so")
# the oracle's flags (oracle/Makefile): the arithmetic rounds as on the device
CFLAGS = ["-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=gnu11", "-Wall", "-Wno-unused-function"]
DEPS = [SRC, os.path.join(ROOT, "include", "eslam_detmath.h"), os.path.join(ROOT, "include", "eslam_gpu.h")]

_lib = None


def build(verbose=False):
    """gcc the reference unless the library is newer than its sources."""
    if os.path.exists(LIB_PATH) and all(os.path.getmtime(d) <= os.path.getmtime(LIB_PATH) for d in DEPS):
        return LIB_PATH
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    cmd = [os.environ.get("CC", "gcc")] + CFLAGS + [f"-I{os.path.join(ROOT, 'include')}", "-shared", "-o", LIB_PATH, SRC, "-lm"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        tail = [C.POINTER(A.ScanParams), C.POINTER(A.ScanPatch), C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(A.ScanInfo)]
        L.scr_from_laser.argtypes = [C.POINTER(A.LaserScan)] + tail
        L.scr_from_depth.argtypes = [C.POINTER(A.DepthImage)] + tail
        L.scr_params_default.argtypes = [C.c_double, C.POINTER(A.ScanParams)]
        L.scr_params_default.restype = None
        L.scr_sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.scr_sincos.restype = None
        _lib = L
    return _lib


def params_default(max_sensor_range=3.0):
    p = A.ScanParams()
    lib().scr_params_default(max_sensor_range, C.byref(p))
    return p


def sincos(x):
    """the contract's dm_sincos"""
    s, c = C.c_double(), C.c_double()
    lib().scr_sincos(float(x), C.byref(s), C.byref(c))
    return s.value, c.value


class Reading:
    """One test input: kind 'laser' (ranges, start_angle, angular_resolution, min_range,
    max_range) or 'depth' (data, scale_x, scale_y, center_x, center_y), with its ScanParams."""

    def __init__(self, name, kind, params, **kw):
        self.name, self.kind, self.params = name, kind, params
        self.__dict__.update(kw)

    def c_reading(self):
        if self.kind == "laser":
            return A.laser_scan(self.ranges, self.start_angle, self.angular_resolution, self.min_range, self.max_range)
        return A.depth_image(self.data, self.scale_x, self.scale_y, self.center_x, self.center_y)

    @property
    def points(self):
        return int(np.asarray(self.ranges).size if self.kind == "laser" else np.asarray(self.data).size)


def patches_array(patches, count=None):
    """a ctypes eslam_scan_patch array as an (n, 4) float64 array: x, y, z, stdev"""
    n = len(patches) if count is None else count
    if not n:
        return np.zeros((0, 4))
    return np.frombuffer(patches, dtype=np.float64, count=4 * n).reshape(n, 4).copy()


def reference(rd):
    """The C reference of a Reading: (patches (n, 4) float64, ScanInfo, points per cluster)."""
    c, _keep = rd.c_reading()
    cap = max(rd.points, 1)
    out = (A.ScanPatch * cap)()
    cl = np.zeros(cap, np.uint32)
    info = A.ScanInfo()
    fn = lib().scr_from_laser if rd.kind == "laser" else lib().scr_from_depth
    rc = fn(C.byref(c), C.byref(rd.params), out, cl.ctypes.data_as(C.POINTER(C.c_uint32)), cap, C.byref(info))
    if rc != 0:
        raise RuntimeError(f"scan reference failed ({rc})")
    n = int(info.patches)
    return patches_array(out, n), info, cl[:n].copy()


def reference_patches(rd):
    """the reference's patches as the ctypes array the map updates take, with the info"""
    arr, info, _ = reference(rd)
    out = (A.ScanPatch * len(arr))()
    for k, row in enumerate(arr):
        out[k].position[0], out[k].position[1], out[k].position[2], out[k].stdev = row
    return out, info


# ---- the shared readings -------------------------------------------------------------------
def quat_rpy(roll, pitch, yaw):
    """(w, x, y, z) of Rz(yaw) Ry(pitch) Rx(roll)"""
    cr, sr, cp, sp, cy, sy = (math.cos(roll / 2), math.sin(roll / 2), math.cos(pitch / 2), math.sin(pitch / 2),
                              math.cos(yaw / 2), math.sin(yaw / 2))
    return (cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy)


def rot_rpy(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def make_params(R=None, t=(0.0, 0.0, 0.0), rpy=(0.0, 0.0, 0.0), **kw):
    p = params_default()
    R = np.eye(3) if R is None else np.asarray(R, float)
    for r in range(3):
        for c in range(3):
            p.sensor2body[4 * r + c] = R[r, c]
        p.sensor2body[4 * r + 3] = t[r]
    for i, v in enumerate(quat_rpy(*rpy)):
        p.orientation[i] = v
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# a camera looking along the body's x: image x to the right (body -y), image y down (body -z)
CAM = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def _laser_floor(name, n, seed, rpy, R, t, start, res):
    """a laser line over a stepped floor (z = -0.5 left of the beam fan's middle, -0.35 right of it,
    in the yaw-free frame), millimetre readings, with error codes, readings outside
    [min_range, max_range] and readings past max_sensor_range"""
    rng = np.random.default_rng(seed)
    p = make_params(R, t, rpy)
    Rw = rot_rpy(rpy[0], rpy[1], 0.0)
    ang = start + np.arange(n) * res
    d = (Rw @ R) @ np.stack([np.cos(ang), np.sin(ang), np.zeros(n)])
    o = Rw @ np.asarray(t)
    floor = np.where(ang < 0, -0.5, -0.35)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d[2] < -1e-3, (floor - o[2]) / d[2], 25.0)
    r = np.clip(r + rng.normal(0, 0.004, n), 0.0, 60.0)
    mm = np.round(r * 1000).astype(np.uint32)
    mm[::97] = (np.arange(len(mm[::97])) % 6).astype(np.uint32)          # 0 and the error codes 1..5
    mm[5::131] = 12                                                     # below min_range
    mm[7::149] = 45000                                                  # above max_range
    return Reading(name, "laser", p, ranges=mm, start_angle=start, angular_resolution=res, min_range=20, max_range=30000)


def depth_floor(name, w, h, seed, rpy=(0.03, -0.05, 0.4), box=True, bad=True):
    """a camera 0.6 m up, pitched down, over a floor with a box on it; NaN, inf, 0 and negative
    pixels when `bad`"""
    rng = np.random.default_rng(seed)
    R = rot_rpy(0.0, 0.6, 0.0) @ CAM
    t = (0.15, -0.02, 0.6)
    p = make_params(R, t, rpy)
    f = 0.9 * w
    sx, sy, cx, cy = 1.0 / f, 1.0 / f, -(w - 1) / 2.0 / f, -(h - 1) / 2.0 / f
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    ray = np.stack([u * sx + cx, v * sy + cy, np.ones_like(u, float)])
    Rw = rot_rpy(rpy[0], rpy[1], 0.0)
    d3 = np.einsum("ij,jhw->ihw", Rw @ R, ray)
    o = Rw @ np.asarray(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(d3[2] < -1e-3, (0.0 - o[2]) / d3[2], 9.0)
    if box:                                                             # a box 0.25 m high in the middle
        top = (0.25 - o[2]) / np.minimum(d3[2], -1e-3)
        m = (abs(u - w / 2) < w / 6) & (abs(v - h / 2) < h / 6)
        d = np.where(m, top, d)
    d = np.clip(d + rng.normal(0, 0.003, d.shape), 0.05, 9.0).astype(np.float32)
    if bad:
        d[3, 5], d[7, 11], d[11, 2], d[13, 17] = np.nan, np.inf, 0.0, -1.5
        d[0, 0] = -np.inf
    return Reading(name, "depth", p, data=d, scale_x=sx, scale_y=sy, center_x=cx, center_y=cy)


def _one_cell():
    """5 000 beams into one cell: a narrow fan of a pitched laser, heights within the thickness"""
    rng = np.random.default_rng(5)
    p = make_params(rot_rpy(0.0, 0.3, 0.0), (0.0, 0.0, 0.0))
    mm = (1020 + rng.integers(-5, 6, 5000)).astype(np.uint32)
    return Reading("one_cell", "laser", p, ranges=mm, start_angle=1e-6, angular_resolution=1e-7, min_range=20, max_range=30000)


def _levels(name, gap):
    """a camera looking straight down from 1.2 m at two surfaces `gap` apart, pixel by pixel"""
    R = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])
    p = make_params(R, (0.013, 0.013, 1.2))
    u, v = np.meshgrid(np.arange(24), np.arange(24))
    d = np.where((u + v) % 2 == 0, 1.0, 1.0 - gap).astype(np.float32)
    return Reading(name, "depth", p, data=d, scale_x=1e-3, scale_y=1e-3, center_x=-0.012, center_y=-0.012)


def _equal_keys():
    """every point at height 0 (an untilted laser on a level body): equal z keys, index order decides"""
    p = make_params()
    mm = np.full(700, 1020, np.uint32)
    return Reading("equal_keys", "laser", p, ranges=mm, start_angle=1e-6, angular_resolution=1e-7, min_range=20, max_range=30000)


_cases = None


def cases():
    """name -> Reading: the inputs of tests/test_gpu_scan.py (and of the CPU tests, which check
    the C reference against the numpy model on every one of them)"""
    global _cases
    if _cases is None:
        tilt = (0.05, -0.08, 0.7)
        Rl = rot_rpy(0.1, 0.5, 0.2)
        tl = (0.2, 0.05, 0.4)
        one = np.array([1, 2, 0, 1500, 3, 5, 45000, 4, 12], np.uint32)
        c = [
            _laser_floor("laser_1081", 1081, 1, tilt, Rl, tl, math.radians(-135.0), math.radians(0.25)),
            _laser_floor("laser_67", 67, 2, tilt, Rl, tl, math.radians(-30.0), math.radians(1.0)),
            depth_floor("depth_61x47", 61, 47, 3),
            depth_floor("depth_301x233", 301, 233, 4),
            _one_cell(),
            _levels("two_levels", 0.2),
            _levels("one_level", 0.05),
            _equal_keys(),
            Reading("one_point", "laser", make_params(Rl, tl, tilt), ranges=one, start_angle=-0.2, angular_resolution=0.05,
                    min_range=20, max_range=30000),
            Reading("no_point", "depth", make_params(CAM, tl, tilt),
                    data=np.array([[np.nan, 0.0, -1.0, np.inf, -np.inf], [0.0] * 5, [np.nan] * 5], np.float32),
                    scale_x=0.01, scale_y=0.01, center_x=-0.02, center_y=-0.01),
        ]
        _cases = {r.name: r for r in c}
    return _cases
