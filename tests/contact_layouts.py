"""Foot layouts for the contact-model tests (test infrastructure, no GPU).

k_project_weight is compiled once per way of holding the pushed contact points, and
eslam_launch_project_weight picks the specialisation from the contact count m, the number of
group ends and whether every contact closes its own group.  LAYOUTS names one foot layout (or
more) per specialisation; expected_variant restates the dispatch so that the tests can assert
which one a layout runs."""
import math

import numpy as np

import eslam_abi as A

WINDOW_LDS_CELLS = 1856          # kWindowLds / sizeof(WinCell): the cells the LDS map window holds


def make_feet(m):
    """m distinct feet on a spiral around (0, -0.2): radii 0.3 .. 0.5 m, z in -0.21 .. -0.18."""
    feet = []
    for i in range(m):
        a = 0.1 + 2.0 * math.pi * i / m
        r = 0.3 + 0.2 * ((i * 7) % m) / max(m - 1, 1)
        z = -0.18 - 0.03 * ((i * 5) % 7) / 6.0
        feet.append((r * math.cos(a), -0.2 + r * math.sin(a), z))
    return feet


def _runs(*lengths):
    """group ids for consecutive groups of the given sizes; a size of 1 is an ungrouped contact"""
    out, gid = [], 0
    for k in lengths:
        if k == 1:
            out.append(-1)
        else:
            out += [gid] * k
            gid += 1
    return out


LAYOUTS = {
    "0": (make_feet(0), []),
    "1": (make_feet(1), [-1]),
    "3_ungrouped": (make_feet(3), [-1] * 3),
    "4_in_2": (make_feet(4), [0, 0, 1, 1]),
    "5_mixed": (make_feet(5), [0, 0, -1, 1, 1]),
    "6_ungrouped": (make_feet(6), [-1] * 6),
    "8_ungrouped": (make_feet(8), [-1] * 8),
    "8_in_5": (make_feet(8), _runs(2, 2, 2, 1, 1)),
    "9_ungrouped": (make_feet(9), [-1] * 9),
    "12_in_6": (make_feet(12), _runs(*[2] * 6)),
    "12_in_8": (make_feet(12), _runs(2, 2, 2, 2, 1, 1, 1, 1)),
    "12_ungrouped": (make_feet(12), [-1] * 12),
    "32_ungrouped": (make_feet(32), [-1] * 32),
    "32_in_16": (make_feet(32), _runs(*[2] * 16)),
    "32_in_4": (make_feet(32), _runs(8, 8, 8, 8)),
}


def group_ends(groups):
    """the contacts that close a group (src/ContactModel.cpp:194-197), as a list of 0 / 1"""
    m = len(groups)
    return [1 if (g == -1 or i + 1 == m or g != groups[i + 1]) else 0 for i, g in enumerate(groups)]


def expected_variant(feet, groups, particle_maps=False):
    """(MAXP, BATCH, UNG) of the evaluate_pose the dispatch chooses for this layout
    (eslam_launch_project_weight; DELTA is particle_maps).  UNG is a template argument of the
    <4, true> forms only and False elsewhere."""
    m = min(len(feet), A.MAX_CONTACTS)
    ends = sum(group_ends(list(groups)[:m]))
    ung = ends == m
    if particle_maps:
        return (4, True, ung) if (m <= 4 and ends <= 4) else (A.MAX_CONTACTS, False, False)
    if ends <= 4:
        return (4, True, ung) if m <= 4 else (4, False, False)
    if ends <= 8:
        return (8, m <= 8, False)
    return (A.MAX_CONTACTS, False, False)


# the rows of the dispatch: (MAXP, BATCH, DELTA, UNG)
ROWS = [(4, True, False, True), (4, True, False, False), (4, False, False, False), (8, True, False, False),
        (8, False, False, False), (32, False, False, False), (4, True, True, False), (32, False, True, False)]
MAP_LAYOUTS = ("4_in_2", "6_ungrouped", "12_in_6")           # the ones run with per-particle maps


def row_of(name, particle_maps=False):
    maxp, batch, ung = expected_variant(*LAYOUTS[name], particle_maps=particle_maps)
    return (maxp, batch, particle_maps, ung)


def contact_pattern(s, i):
    """contact probability of contact i at step s: NaN (unknown: evaluated), 0.1 (< 0.2: skipped)
    or 0.9, varying with both"""
    if (s + i) % 3 == 0:
        return float("nan")
    return 0.1 if (s * 7 + i) % 5 == 0 else 0.9


def holey(grid, frac, seed):
    """The grid without the patches of a random share `frac` of its cells (seeded)."""
    w, h = grid.width, grid.height
    keep_cell = np.random.default_rng(seed).random(w * h) >= frac          # cell n * w + m
    counts = np.diff(grid.cell_start.astype(np.int64))
    keep_patch = np.repeat(keep_cell, counts)
    new_counts = np.where(keep_cell, counts, 0)
    cell_start = np.zeros(w * h + 1, dtype=np.uint64)
    np.cumsum(new_counts, out=cell_start[1:])
    ph = None if grid.patch_height is None else grid.patch_height[keep_patch]
    return A.GridArrays(w, h, grid.scale, grid.offset, cell_start.astype(np.uint32), grid.mean[keep_patch],
                        grid.stdev[keep_patch], ph, grid.g2l)


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def yaw_free_feet(step):
    """ContactModel::setContactPoints (src/ContactModel.cpp:21-41): the contact positions
    rotated by the body orientation without its yaw, base::removeYaw(q) = Rz(-yaw(q)) q."""
    R = _rot([float(v) for v in step.body2odometry_rot])
    yaw = math.atan2(R[1, 0], R[0, 0]) if math.hypot(R[2, 2], R[2, 1]) > 1e-12 else 0.0
    c, s = math.cos(-yaw), math.sin(-yaw)
    Rc = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ R
    m = min(int(step.n_contacts), A.MAX_CONTACTS)
    return [Rc @ np.array([float(v) for v in step.contacts[i].position]) for i in range(m)]


def window_cells(particles, step, cfg, grid, max_weight=1.0):
    """rows * cols of the map window that stage_window stages for the weighting of `step`, or 0
    where it stages none: `particles` is the cloud the previous weighting saw (its bounding box,
    of the finite coordinates rounded to float and widened, is what the device keeps) and
    max_weight the update info's max_weight before the step (the spread of project() widens the
    margin by 6 spread_translation_factor spread).  The caller compares with WINDOW_LDS_CELLS.
    It says nothing about the first weighting of a filter (no box yet: no window)."""
    feet = yaw_free_feet(step)
    reach = max([math.hypot(f[0], f[1]) for f in feet], default=0.0)
    mu, cov = step.sample_mean, step.sample_cov
    motion = math.hypot(mu[0], mu[1]) + 6.0 * math.sqrt(cov[0] + cov[4])
    x = max_weight
    beta = cfg.spread_threshold                      # dm_weighting_function(x, 0, beta, 0)
    spread = 1.0 if x < 0.0 else ((1.0 / (0.0 - beta)) * x + 1.0 if x < beta else 0.0)
    mg = (reach + motion + 0.05) + 6.0 * (cfg.spread_translation_factor * spread)

    def box(v):
        v = v[np.isfinite(v)]
        if v.size == 0:
            return None
        lo, hi = float(np.float32(v.min())), float(np.float32(v.max()))
        wide = lambda t: abs(t) * 2.0 ** -22 + 2.0 ** -140
        return lo - wide(lo), hi + wide(hi)

    bx, by = box(particles.x), box(particles.y)
    if bx is None or by is None or grid.patch_height is not None:
        return 0
    g = grid.g2l
    xs, ys = (bx[0] - mg, bx[1] + mg), (by[0] - mg, by[1] + mg)
    lx = [g[0] * wx + g[1] * wy + g[3] for wx in xs for wy in ys]
    ly = [g[4] * wx + g[5] * wy + g[7] for wx in xs for wy in ys]
    inv = (1.0 / grid.scale[0], 1.0 / grid.scale[1])
    clamp = lambda v, top: int(min(max(v, 1.0), float(top)))
    m0 = clamp(math.floor((min(lx) - grid.offset[0]) * inv[0]) - 1.0, grid.width)
    m1 = clamp(math.floor((max(lx) - grid.offset[0]) * inv[0]) + 2.0, grid.width)
    n0 = clamp(math.floor((min(ly) - grid.offset[1]) * inv[1]) - 1.0, grid.height)
    n1 = clamp(math.floor((max(ly) - grid.offset[1]) * inv[1]) + 2.0, grid.height)
    rows, cols = n1 - n0, m1 - m0
    return rows * cols if rows > 0 and cols > 0 else 0


def layout_stream(name, steps=4, pattern=True, feet=None):
    """the step stream of a layout: tilted body, contact_pattern probabilities, ltc = 1"""
    import synthetic as S
    f, groups = LAYOUTS[name]
    f = f if feet is None else feet
    return S.step_stream(steps, tilt=True, feet=f, groups=groups if groups else None,
                         contact=contact_pattern if pattern else 1.0, ltc=1)
