"""The inputs of the KLD bin-count tests, shared by the CPU test of the restatement
(tests/test_kld_ref.py) and the GPU test (tests/test_gpu_kld.py), and the independent numpy model
of the count: np.floor, np.unique over the key triples, the bound in Python floats."""
import math

import numpy as np

INV_2PI = float.fromhex("0x1.45f306dc9c883p-3")       # the double nearest 1 / (2 pi)
Z99 = 2.3263478740408408
LIMIT = 2 ** 32 - 2
DEFAULTS = dict(bin_xy=0.1, theta_bins=36, multinomial=0, epsilon=0.05, z_quantile=Z99, n_min=1, n_max=0, min_change=0.0,
                max_bins=0)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4096)
ERR_UNSUPPORTED = -8                # ESLAM_ERR_UNSUPPORTED (include/eslam_gpu.h)


def cloud(n, seed, sigma=0.3, centre=(1.2, -0.7)):
    """a Gaussian cloud with yaw on both sides of 0 and positive weights"""
    r = np.random.default_rng(seed)
    x = centre[0] + sigma * r.standard_normal(n)
    y = centre[1] + sigma * r.standard_normal(n)
    th = 0.3 + 0.5 * r.standard_normal(n)
    w = r.uniform(0.1, 1.0, n) / n
    return x, y, th, w


def one_bin(n):
    return np.full(n, 0.05), np.full(n, -0.05), np.full(n, 0.01), np.full(n, 1.0 / n)


def row_of_cells(m, bin_xy=0.1):
    """m particles in m consecutive cells of one row, one yaw bin: bits 0..m-1 with theta_bins 1"""
    x = (np.arange(m) + 0.5) * bin_xy
    return x, np.full(m, 0.05), np.zeros(m), np.full(m, 1.0 / m)


def yaw_fan(t):
    """t particles in one cell, one per yaw bin of theta_bins = t"""
    th = (np.arange(t) + 0.5) * (2.0 * math.pi / t)
    return np.full(t, 0.05), np.full(t, 0.05), th, np.full(t, 1.0 / t)


def lattice(m, t, bin_xy=0.1):
    """one particle in every bin of an m x m x t lattice (shuffled)"""
    ix, iy, it = np.meshgrid(np.arange(m) - m // 2, np.arange(m) - m // 2, np.arange(t), indexing="ij")
    x = (ix.ravel() + 0.5) * bin_xy
    y = (iy.ravel() + 0.5) * bin_xy
    th = (it.ravel() + 0.5) * (2.0 * math.pi / t)
    p = np.random.default_rng(m * 100 + t).permutation(x.shape[0])
    n = x.shape[0]
    return x[p], y[p], th[p], np.full(n, 1.0 / n)


def edges():
    """negative coordinates and coordinates exactly on bin edges, -0.0 and the smallest doubles
    on either side of 0 among them (bin_xy 0.25: inv is exact, so k * 0.25 sits on an edge)"""
    v = np.array([-0.75, -0.5, -0.25, -0.0, 0.0, 0.25, 0.5, -5e-324, 5e-324, -0.2500000000000001, 0.24999999999999997,
                  -1.0, 1.0, -0.1, -0.3, 0.3])
    x, y = [a.ravel() for a in np.meshgrid(v, v[::-1], indexing="ij")]
    n = x.shape[0]
    return x, y, np.zeros(n), np.full(n, 1.0 / n)


def yaws():
    """negative yaw, yaw at and above 2 pi, -0.0, and tiny negative yaws whose turn fraction rounds to 1.0"""
    tp = 2.0 * math.pi
    th = np.array([-0.0, 0.0, -1e-20, -5e-324, -1e-17, -0.1, -3.0, -tp, -tp - 0.1, tp, tp + 0.1, 3 * tp, 100.5, -100.5, 1e6, -1e6,
                   3.141592653589793, -3.141592653589793, 6.283185307179586, 6.283185307179585, 1e300, -1e300])
    n = th.shape[0]
    return np.full(n, 0.05), np.full(n, 0.05), th, np.full(n, 1.0 / n)


SKIP_KINDS = [(f, v) for f in range(4) for v in (float("nan"), float("inf"), float("-inf"))] + \
             [(3, 0.0), (3, -0.0), (3, -0.25), (0, 2.2e8), (0, -2.2e8), (1, 1e300), (1, -2.147483649e8)]


def with_skipped(x, y, th, w, seed):
    """every kind of skipped particle planted at distinct places (n >= 64); returns the count.
    |x| = 2.2e8 at bin_xy 0.1 is past 2^31 cells; -2.147483649e8 is just past -2^31."""
    arrs = [np.array(a, dtype=np.float64) for a in (x, y, th, w)]
    where = np.random.default_rng(seed).choice(arrs[0].shape[0], len(SKIP_KINDS), replace=False)
    for i, (f, v) in zip(where, SKIP_KINDS):
        arrs[f][i] = v
    return (*arrs, len(SKIP_KINDS))


def cases():
    """[(name, x, y, theta, w, params)]: what both the restatement and the device are checked on"""
    out = []
    for n in SIZES:
        out.append((f"cloud{n}", *cloud(n, seed=n), {}))
    # past the marking pass' first launch (the first 16384 particles): one particle, and a wide
    # cloud most of whose bins only the second launch sees
    out.append(("cloud16385", *cloud(16385, seed=16385), {}))
    out.append(("cloud40000_wide", *cloud(40000, seed=4, sigma=3.0), {}))
    out.append(("one_bin_1000", *one_bin(1000), {}))
    out.append(("one_bin_64", *one_bin(64), dict(theta_bins=1)))
    out.append(("word_row_64", *row_of_cells(64), dict(theta_bins=1)))
    out.append(("word_row_65", *row_of_cells(65), dict(theta_bins=1)))
    out.append(("word_fan_64", *yaw_fan(64), dict(theta_bins=64)))
    out.append(("lattice_5_7", *lattice(5, 7), dict(theta_bins=7)))
    out.append(("edges", *edges(), dict(bin_xy=0.25)))
    out.append(("edges_tenth", *edges(), {}))
    for tb in (1, 36, 4096):
        out.append((f"yaws_{tb}", *yaws(), dict(theta_bins=tb)))
    out.append(("cloud_4096_bins", *cloud(1000, seed=5), dict(theta_bins=4096, bin_xy=0.02)))
    for n in (257, 1000):
        x, y, th, w, _ = with_skipped(*cloud(n, seed=40 + n), seed=n)
        out.append((f"skipped{n}", x, y, th, w, {}))
    x, y, th, w = cloud(300, seed=9)
    out.append(("none_counted", x, y, th, np.zeros(300), dict(n_min=17)))
    out.append(("too_spread", *cloud(500, seed=11, sigma=40.0), dict(max_bins=100000)))
    out.append(("clamps", *cloud(1000, seed=13), dict(n_min=50, n_max=400, min_change=0.0)))
    out.append(("held", *cloud(1000, seed=13), dict(n_min=1, min_change=20.0)))
    return out


def kld_bound(k, epsilon, z):
    if k <= 1:
        return 0.0
    a = 2.0 / (9.0 * (k - 1))
    t = (1.0 - a) + math.sqrt(a) * z
    return ((k - 1) / (2.0 * epsilon)) * t * t * t


def kld_samples(bound, n_min, limit, capacity, n_global, min_change):
    """(samples, clamped): the clamp order of DESIGN.md 5h in Python integers"""
    s = 2 ** 64 - 1 if (not math.isfinite(bound) or bound >= 2.0 ** 63) else math.ceil(bound)
    c = 0
    if s < n_min:
        s, c = n_min, c | 1
    if s > limit:
        s, c = limit, c | 2
    if capacity and s > capacity:
        s, c = capacity, c | 4
    if float(abs(s - n_global)) <= min_change * float(n_global):
        s, c = n_global, c | 8
    return s, c


def model(x, y, th, w, limit=LIMIT, capacity=0, **params):
    """(rc, dict of every eslam_kld_info field) by numpy, independent of the C code"""
    p = dict(DEFAULTS, **params)
    x, y, th, w = [np.asarray(a, dtype=np.float64) for a in (x, y, th, w)]
    n = x.shape[0]
    inv = 1.0 / p["bin_xy"]
    tb = p["theta_bins"]
    with np.errstate(all="ignore"):
        fx, fy = np.floor(x * inv), np.floor(y * inv)
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(th) & np.isfinite(w) & (w > 0.0)
        ok &= (fx >= -2.0 ** 31) & (fx <= 2.0 ** 31 - 1) & (fy >= -2.0 ** 31) & (fy <= 2.0 ** 31 - 1)
        u = th * INV_2PI
        u = u - np.floor(u)
        ft = np.floor(u * float(tb))
    info = dict(particles_counted=int(ok.sum()), particles_skipped=int(n - ok.sum()), bins_occupied=0, origin=[0, 0],
                bins=[0, 0, tb], bound=0.0, samples=0, clamped=0, pad=0)
    if ok.any():
        ix, iy, it = fx[ok].astype(np.int64), fy[ok].astype(np.int64), ft[ok].astype(np.int64)
        it[it == tb] = 0
        info["origin"] = [int(ix.min()), int(iy.min())]
        info["bins"] = [int(ix.max() - ix.min() + 1), int(iy.max() - iy.min() + 1), tb]
        if info["bins"][0] * info["bins"][1] * tb > (p["max_bins"] or 2 ** 27):
            return ERR_UNSUPPORTED, info
        info["bins_occupied"] = int(np.unique(np.stack([ix, iy, it], axis=1), axis=0).shape[0])
    info["bound"] = kld_bound(info["bins_occupied"], p["epsilon"], p["z_quantile"])
    lim = min(limit, p["n_max"]) if p["n_max"] else limit
    info["samples"], info["clamped"] = kld_samples(info["bound"], p["n_min"], lim, capacity, n, p["min_change"])
    return 0, info
