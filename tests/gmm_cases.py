"""Particle clouds for the Gaussian-mixture tests (tests/test_gmm_ref.py, tests/test_gpu_gmm.py) and
the independent numpy EM the C restatement is compared with."""
import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))


def clusters(centres, per, sigma, seed, wscale=3e-7):
    """`per` particles around each centre (isotropic, sigma), weights uniform in [0.2, 1] x wscale,
    order shuffled"""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    for cx, cy in centres:
        xs.append(cx + sigma * rng.standard_normal(per))
        ys.append(cy + sigma * rng.standard_normal(per))
    x, y = np.concatenate(xs), np.concatenate(ys)
    w = rng.uniform(0.2, 1.0, x.shape[0]) * wscale
    p = rng.permutation(x.shape[0])
    return x[p].copy(), y[p].copy(), w[p].copy()


def cloud(n, seed, k=3):
    """n particles in k clusters of unequal size along a slanted line (any n >= 1)"""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, k, n)
    x = 4.0 * which + 0.3 * rng.standard_normal(n) + 20.0
    y = 1.5 * which + 0.2 * rng.standard_normal(n) - 7.0
    w = rng.uniform(0.2, 1.0, n) * 3e-7
    return x, y, w


def with_skipped(x, y, w, seed):
    """every kind of skipped particle spread through the cloud; returns the arrays and the count"""
    rng = np.random.default_rng(seed)
    x, y, w = x.copy(), y.copy(), w.copy()
    n = x.shape[0]
    idx = rng.permutation(n)[:min(n // 2, 12)]
    kinds = [("x", np.nan), ("y", np.inf), ("w", 0.0), ("w", -1e-7), ("w", np.inf), ("w", np.nan), ("x", -np.inf)]
    for j, i in enumerate(idx):
        f, v = kinds[j % len(kinds)]
        {"x": x, "y": y, "w": w}[f][i] = v
    return x, y, w, len(idx)


def numpy_em(x, y, w, K, iterations, min_variance):
    """The rule of DESIGN.md 5g in numpy float64 with numpy's own exp and log and plain sums, run
    for exactly `iterations` passes.  Returns (weights[K], means[K, 2], covs[K, 3], log_likelihood)."""
    x, y, w = (np.asarray(a, dtype=np.float64) for a in (x, y, w))
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(w) & (w > 0)
    x, y, w = x[ok] + 0.0, y[ok] + 0.0, w[ok]
    E = int(np.frexp(w.max())[1])
    wh = np.ldexp(w, -E)
    cx, cy = 0.5 * x.min() + 0.5 * x.max(), 0.5 * y.min() + 0.5 * y.max()
    xp, yp = x - cx, y - cy
    a = x if (x.max() - x.min()) >= (y.max() - y.min()) else y
    h = (a.max() - a.min()) / K
    comp = np.minimum(K - 1, np.floor((a - a.min()) / h)).astype(int) if h > 0 else np.zeros(x.shape[0], int)
    r = np.zeros((K, x.shape[0]))
    r[comp, np.arange(x.shape[0])] = 1.0
    live = np.ones(K, bool)
    P = {}

    def mstep(r):
        S0 = (wh * r).sum(axis=1)
        out = np.zeros((K, 6))
        A = np.zeros((K, 4))
        for k in range(K):
            if not live[k] or S0[k] == 0.0:
                live[k] = False
                continue
            t = wh * r[k]
            mx, my = (t * xp).sum() / S0[k], (t * yp).sum() / S0[k]
            cxx = (t * xp * xp).sum() / S0[k] - mx * mx
            cxy = (t * xp * yp).sum() / S0[k] - mx * my
            cyy = (t * yp * yp).sum() / S0[k] - my * my
            out[k] = (S0[k] / S0.sum(), mx, my, cxx, cxy, cyy)
            axx, ayy = cxx + min_variance, cyy + min_variance
            det = axx * ayy - cxy * cxy
            if not np.isfinite(det) or not det > 0:
                live[k] = False
                continue
            A[k] = (axx, cxy, ayy, det)
        P["out"], P["A"] = out, A

    mstep(r)
    L = float("nan")
    for _ in range(iterations):
        if not live.any():
            break
        out, A = P["out"], P["A"]
        lp = np.full((K, x.shape[0]), -np.inf)
        for k in np.flatnonzero(live):
            dx, dy = xp - out[k, 1], yp - out[k, 2]
            q = (A[k, 2] * dx * dx - 2.0 * A[k, 1] * dx * dy + A[k, 0] * dy * dy) / A[k, 3]
            lp[k] = np.log(out[k, 0]) - 0.5 * np.log(A[k, 3]) - 0.5 * q - LOG_2PI
        M = lp.max(axis=0)
        e = np.exp(lp - M)
        s = e.sum(axis=0)
        r = e / s
        L = float((wh * (M + np.log(s))).sum() / wh.sum())
        mstep(r)
    out = P["out"]
    means = out[:, 1:3] + np.where(out[:, :1] != 0.0, np.array([[cx, cy]]), 0.0)
    return out[:, 0].copy(), means, out[:, 3:6].copy(), L
