"""Particle clouds for the pose-moment tests (tests/test_moments_ref.py, tests/test_gpu_pose_moments.py,
tests/pose_moments_dist_worker.py) and the independent numpy computation the C restatement is
compared with.  A cloud is a dict of six float64 arrays: x, y, z, theta, zsigma, w."""
import numpy as np

import eslam_abi as A

FIELDS = ("x", "y", "z", "theta", "zsigma", "w")


def blob(n, seed, centre=(1000.0, -2000.0, 0.2), yaw=0.3, yaw_sigma=0.1, sigma=(0.4, 0.25, 0.02), wscale=3e-7):
    """n particles around centre with yaws around `yaw`, weights uniform in [0.2, 1] x wscale"""
    rng = np.random.default_rng(seed)
    return {"x": centre[0] + sigma[0] * rng.standard_normal(n), "y": centre[1] + sigma[1] * rng.standard_normal(n),
            "z": centre[2] + sigma[2] * rng.standard_normal(n), "theta": yaw + yaw_sigma * rng.standard_normal(n),
            "zsigma": rng.uniform(0.005, 0.03, n), "w": rng.uniform(0.2, 1.0, n) * wscale}


def across_the_cut(n, seed):
    """a blob whose yaws have mean pi - 0.05 and sigma 0.3, given in (-pi, pi]: they straddle the cut"""
    c = blob(n, seed, yaw=np.pi - 0.05, yaw_sigma=0.3)
    c["theta"] = np.angle(np.exp(1j * c["theta"]))
    return c


def whole_turns(c, seed):
    """the cloud with 2 pi k, k in [-3, 3], added to every yaw"""
    rng = np.random.default_rng(seed)
    d = {f: c[f].copy() for f in FIELDS}
    d["theta"] = d["theta"] + 2.0 * np.pi * rng.integers(-3, 4, d["theta"].shape[0])
    return d


def correlated(n, seed, rho=0.8):
    """a cloud whose x and yaw deviations have correlation rho"""
    rng = np.random.default_rng(seed)
    c = blob(n, seed + 1)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    c["x"] = 5.0 + 0.5 * a
    c["theta"] = -1.0 + 0.2 * (rho * a + np.sqrt(1.0 - rho * rho) * b)
    return c


def concat(*clouds):
    return {f: np.concatenate([c[f] for c in clouds]) for f in FIELDS}


def shuffled(c, seed):
    p = np.random.default_rng(seed).permutation(c["x"].shape[0])
    return {f: c[f][p].copy() for f in FIELDS}


def two_clusters(n, seed):
    """the gate case: a heavier cluster at (20, -7) and a lighter one 6 m away, shuffled, with the
    gate on the first (4 sigma of its generating covariance: no member of the other is inside).
    Returns (cloud, PoseGate, mask of the first cluster's particles)."""
    n0 = n - n // 3
    a = blob(n0, seed, centre=(20.0, -7.0, 0.2), yaw=3.0, yaw_sigma=0.2)
    b = blob(n - n0, seed + 1, centre=(26.0, -7.5, 0.4), yaw=-2.0, yaw_sigma=0.2, wscale=1e-7)
    c = concat(a, b)
    member = np.concatenate([np.ones(n0, bool), np.zeros(n - n0, bool)])
    p = np.random.default_rng(seed + 2).permutation(n)
    c = {f: c[f][p].copy() for f in FIELDS}
    gate = A.PoseGate((20.0, -7.0), (0.16, 0.0, 0.0625), 16.0)
    return c, gate, member[p]


def cloud(n, seed):
    """the GPU tests' cloud at any n >= 1: the gate case's two clusters"""
    return two_clusters(n, seed)[:2]


SKIP_KINDS = [("x", np.nan), ("theta", np.inf), ("zsigma", np.nan), ("w", 0.0), ("w", -1e-7), ("w", np.nan),
              ("y", -np.inf), ("z", np.nan), ("w", np.inf), ("zsigma", np.inf)]


def with_skipped(c, seed):
    """every kind of skipped particle spread through the cloud; returns the cloud and the count"""
    rng = np.random.default_rng(seed)
    d = {f: c[f].copy() for f in FIELDS}
    n = d["x"].shape[0]
    idx = rng.permutation(n)[:min(n // 2, 2 * len(SKIP_KINDS))]
    for j, i in enumerate(idx):
        f, v = SKIP_KINDS[j % len(SKIP_KINDS)]
        d[f][i] = v
    return d, len(idx)


def particles(c):
    """the cloud as an eslam_abi.ParticleArrays"""
    pa = A.ParticleArrays(c["x"].shape[0])
    pa.x[:], pa.y[:], pa.zpos[:], pa.orientation[:], pa.zsigma[:], pa.weight[:] = (c[f] for f in FIELDS)
    return pa


def inside(c, gate):
    """numpy's own evaluation of the gate's quadratic form"""
    dx, dy = c["x"] - gate.centre[0], c["y"] - gate.centre[1]
    axx, axy, ayy = gate.cov
    return (ayy * dx * dx - 2.0 * axy * dx * dy + axx * dy * dy) / (axx * ayy - axy * axy) <= gate.chi2


def numpy_moments(c, mask=None):
    """The rule of DESIGN.md 5i in numpy float64 with numpy's own sin, cos, arctan2 and plain sums,
    over the valid particles selected by mask.  Returns a dict: mean[4], cov[4, 4], z_within,
    yaw_resultant, effective, weight_share, counted."""
    x, y, z, th, zs, w = (np.asarray(c[f], dtype=np.float64) for f in FIELDS)
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(th) & np.isfinite(zs) & np.isfinite(w) & (w > 0)
    sel = ok if mask is None else ok & mask
    wall = w[ok].sum()
    x, y, z, th, zs, w = (a[sel] for a in (x, y, z, th, zs, w))
    W = w.sum()
    psi = float(np.arctan2((w * np.sin(th)).sum(), (w * np.cos(th)).sum()))
    mean = np.array([(w * x).sum() / W, (w * y).sum() / W, (w * z).sum() / W, psi])
    dev = np.stack([x - mean[0], y - mean[1], z - mean[2], np.angle(np.exp(1j * (th - psi)))])
    cov = np.cov(dev, aweights=w, ddof=0)
    return {"mean": mean, "cov": np.atleast_2d(cov), "z_within": float((w * zs * zs).sum() / W),
            "yaw_resultant": float(np.hypot((w * np.sin(th)).sum(), (w * np.cos(th)).sum()) / W),
            "effective": float(W * W / (w * w).sum()), "weight_share": float(W / wall), "counted": int(sel.sum())}
