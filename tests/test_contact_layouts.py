"""The oracle's contact model on every foot layout of contact_layouts.LAYOUTS, against a plain
Python restatement of the reference (CPU only).

The GPU tests of test_gpu_contact_layouts.py compare k_project_weight bit for bit with the
oracle's generic loop (or_cm_evaluate_pose) on layouts of up to 32 contacts, grouped and not;
before this file that loop was pinned to the reference's expected values by four-contact
KATs only.  Here it is compared with a model written from the reference source:

* ContactModel::evaluatePose + contactLikelihoodRatio + evaluateWeight
  (src/ContactModel.cpp:104-224, 262-317), updateZPositionEstimate (319-340), the per-particle
  part of PoseEstimator::updateWeights (src/PoseEstimator.cpp:276-319) and GridAccess::get
  (src/PoseEstimator.hpp:97-105: the first patch of the cell within 3 sigma of the query patch),
  in Python floats with math.exp / math.erfc / math.pow, one particle at a time.

Measured (300 particles x 15 layouts, holey rough map): the model and the literal oracle
differ by at most 1.1e-12 relative (layout 6_ungrouped; every count, decision and pushed
point's cell identical); the contract and the literal oracle by at most 1.1e-13 with 0
threshold flips (the cap is 1 % of the particles: 3).  The bound asserted is
test_parity_lineage.REGRESSION_TOL (1e-9).  Run with -s to see the figures per layout."""
import math

import numpy as np
import pytest

import contact_layouts as L
import eslam_abi as A
import oracle_ffi as O
import synthetic as S
from test_parity_lineage import REGRESSION_TOL

N_MODEL = 300
N_ORACLE = 3000
HOLES, HOLE_SEED = 0.12, 11
INIT = dict(mu=[0.0, 0.0, 0.0], sigma=[0.3, 0.3, 0.2], z=0.18, zs=0.3)


@pytest.fixture(scope="module")
def grid():
    return L.holey(S.rough_map(cells=200), HOLES, HOLE_SEED)


def layout_config(name, n):
    cfg = S.bench_config(A.default_config(), n)
    cfg.min_contacts = min(2, len(L.LAYOUTS[name][0]))
    return cfg


# ---- the model ------------------------------------------------------------------------------
class Margin:
    """the smallest relative distance of any threshold decision from its threshold"""

    def __init__(self):
        self.v = math.inf

    def see(self, value, threshold):
        self.v = min(self.v, abs(value - threshold) / abs(threshold))


def cell_of(grid, x, y):
    m = math.floor((x - grid.offset[0]) / grid.scale[0])
    n = math.floor((y - grid.offset[1]) / grid.scale[1])
    if 0 <= m < grid.width and 0 <= n < grid.height:
        return n * grid.width + m
    return None


def model_get(grid, pos, meas_var, margin):
    """GridAccess::get: the query patch is (mean = z, stdev = sqrt(measVar)); the first patch of
    the point's cell whose distance is below 3 sqrt(stdev_p^2 + stdev_q^2)."""
    assert grid.patch_height is None
    g = grid.g2l
    lx = g[0] * pos[0] + g[1] * pos[1] + g[2] * pos[2] + g[3]
    ly = g[4] * pos[0] + g[5] * pos[1] + g[6] * pos[2] + g[7]
    lz = g[8] * pos[0] + g[9] * pos[1] + g[10] * pos[2] + g[11]
    cell = cell_of(grid, lx, ly)
    if cell is None:
        return None
    sd_q = math.sqrt(meas_var)
    for k in range(int(grid.cell_start[cell]), int(grid.cell_start[cell + 1])):
        pm, ps = float(grid.mean[k]), float(grid.stdev[k])
        dist, gate = abs(pm - lz), 3.0 * math.sqrt(ps * ps + sd_q * sd_q)
        margin.see(dist, gate)
        if dist < gate:
            return pm, ps
    return None


def likelihood_ratio(z, sigma, correction):
    """contactLikelihoodRatio: pdf / cdf of boost::math::normal(0, sigma * correction)"""
    sd = sigma * correction
    pdf = math.exp(-(z * z) / (2.0 * sd * sd)) / (sd * math.sqrt(2.0 * math.pi))
    cdf = math.erfc(-(z / (sd * math.sqrt(2.0)))) / 2.0
    return pdf / cdf


def ieee_div(a, b):
    """a / b as C++ doubles divide: x / 0 is an infinity or NaN, not an exception"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def model_particle(grid, cfg, feet, contact, groups, x, y, theta, zpos, zsigma):
    """One particle of updateWeights.  Returns a dict: accepted, points (x, y, mean, zdiff, zvar),
    zdelta, zvar, mprob, zpos, zsigma and the decision margin."""
    margin = Margin()
    meas_var = math.pow(zsigma, 2) + math.pow(cfg.measurement_error, 2)
    assert meas_var != 0
    co, si = math.cos(theta), math.sin(theta)
    points = []
    p = None
    valid, group_valid = False, True
    contact_ratio = pose_var_avg = pose_var_sum = 0.0
    m = len(feet)
    for i in range(m):
        gid = groups[i]
        c = feet[i]
        w = (co * c[0] - si * c[1] + x, si * c[0] + co * c[1] + y, c[2] + zpos - cfg.contact_point_radius)
        prob = float(np.float32(contact[i]))
        if group_valid and not (prob < 0.2):
            patch = model_get(grid, w, meas_var, margin)
            if patch is not None:
                mean, stdev = patch
                zdiff = w[2] - mean
                pose_var = math.pow(stdev, 2)
                zvar = math.pow(stdev, 2) + meas_var
                ratio = likelihood_ratio(zdiff, math.sqrt(zvar), cfg.contact_likelihood_correction)
                if not valid:
                    p = [w[0], w[1], mean, zdiff * ratio, zvar * ratio]
                    contact_ratio = ratio
                    pose_var_avg = pose_var * ratio
                else:
                    p[3] += zdiff * ratio
                    p[4] += zvar * ratio
                    contact_ratio += ratio
                    pose_var_avg += pose_var * ratio
                valid = True
            else:
                group_valid = False
        if valid and (gid == -1 or i + 1 == m or gid != groups[i + 1]):
            margin.see(contact_ratio, 1e-9)
            if group_valid and contact_ratio > 1e-9:
                p[3] /= contact_ratio
                p[4] /= contact_ratio
                pose_var_sum += pose_var_avg / contact_ratio
                points.append(tuple(p))
            group_valid, valid = True, False
            pose_var_avg = contact_ratio = 0.0
    out = dict(points=points, accepted=len(points) >= cfg.min_contacts, zpos=zpos, zsigma=zsigma, mprob=1.0,
               zdelta=0.0, zvar=0.0, margin=margin)
    if not out["accepted"]:
        return out
    # evaluateWeight
    d1 = d2 = 0.0
    for q in points:
        d1 += q[3] / q[4]
        d2 += 1.0 / q[4]
    delta = ieee_div(d1, d2)
    pz = 1.0
    for q in points:
        odiff = (q[3] - delta) / math.sqrt(q[4])
        if cfg.use_shape_update:
            pz *= math.exp(-(odiff * odiff) / 2.0)
    out.update(mprob=pz, zdelta=-delta, zvar=ieee_div(1.0, d2))
    # updateZPositionEstimate (accepted without points, minContacts = 0: 0 / 0 and 1 / 0 as in C++)
    z_var = math.pow(zsigma, 2)
    pose_var = ieee_div(pose_var_sum, float(len(points)))
    a = z_var - pose_var
    delta_var = 1e-9 if a < 1e-9 else a                  # std::max(a, 1e-9)
    gate = abs(out["zdelta"] / math.sqrt(delta_var))
    margin.see(gate, 1.0)
    if not gate > 1.0:
        out["zpos"] = zpos + z_var / (z_var + out["zvar"]) * out["zdelta"]
        var_gain = delta_var / (delta_var + out["zvar"])
        z_var = pose_var + (1.0 - var_gain) * delta_var
    out["zsigma"] = math.sqrt(z_var)
    return out


# ---- the oracle runs ------------------------------------------------------------------------
def rel(a, b):
    """largest relative difference; equal infinities and two NaN count as equal, one NaN as infinite"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(all="ignore"):
        d = np.where(same, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
    d = np.where(np.isnan(d), np.inf, d)
    return float(np.max(d, initial=0.0))


def one_update(cfg, grid, start, st, sum_mode, literal):
    """one update (no resample: min_effective is 0) of the uploaded particles; returns the
    particles after it and the capture (ncp, points, zdelta, zvar)"""
    f = O.OracleFilter(cfg, sum_mode)
    f.set_literal(literal)
    f.set_map(grid)
    f.upload(start)
    f.set_debug(True)
    assert f.update(st) == 0
    assert f.info().resampled == 0
    ncp, cp, zd, zv = f.debug()
    pts = np.ctypeslib.as_array(cp).reshape(start.n, A.MAX_CONTACTS)
    return f.download(), ncp.copy(), pts.copy(), zd.copy(), zv.copy()


WORST = {}


@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_oracle_matches_reference_model(oracle, grid, name):
    feet, groups = L.LAYOUTS[name]
    n = N_MODEL
    cfg = layout_config(name, n)
    cfg.min_effective = 0
    st = L.layout_stream(name, steps=2)[1]
    # the start: a projected cloud (every particle its own pose, z and z sigma)
    f0 = O.OracleFilter(cfg, O.SUM_CONTRACT)
    f0.set_map(grid)
    f0.init_gaussian(n, INIT["mu"], INIT["sigma"], INIT["z"], INIT["zs"])
    f0.project(st)
    start = f0.download()
    start.zsigma[:] = np.linspace(0.05, 0.4, n)          # narrow and wide 3-sigma and 1-sigma gates
    lit, l_ncp, l_pts, l_zd, l_zv = one_update(cfg, grid, start, st, O.SUM_REFERENCE, True)
    con, c_ncp, c_pts, c_zd, c_zv = one_update(cfg, grid, start, st, O.SUM_CONTRACT, False)

    yf = L.yaw_free_feet(st)
    contact = [st.contacts[i].contact for i in range(len(feet))]
    worst = 0.0
    flips = 0
    for i in range(n):
        mo = model_particle(grid, cfg, yf, contact, groups, start.x[i], start.y[i], start.orientation[i],
                            start.zpos[i], start.zsigma[i])
        k = len(mo["points"])
        # the model against the literal oracle: decisions and cells exact, values within the bound
        assert l_ncp[i] == k == lit.n_contact_points[i], (name, i)
        assert bool(lit.floating[i]) == (not mo["accepted"]), (name, i)
        got = l_pts[i, :k]
        for q in range(k):
            want = mo["points"][q]
            assert cell_of(grid, got["point"][q, 0], got["point"][q, 1]) == cell_of(grid, want[0], want[1]), (name, i, q)
            assert got["point"][q, 2] == want[2], (name, i, q, "patch mean")
        cols = [(got["zdiff"], [w[3] for w in mo["points"]]), (got["zvar"], [w[4] for w in mo["points"]]),
                (got["point"][:, 0], [w[0] for w in mo["points"]]), (got["point"][:, 1], [w[1] for w in mo["points"]]),
                ([lit.mprob[i]], [mo["mprob"]]), ([lit.zpos[i]], [mo["zpos"]]), ([lit.zsigma[i]], [mo["zsigma"]])]
        if mo["accepted"]:
            cols += [([l_zd[i]], [mo["zdelta"]]), ([l_zv[i]], [mo["zvar"]])]
        for a, b in cols:
            worst = max(worst, rel(a, b))
        # the contract oracle against the literal one: the same, but for decisions that fall
        # within the bound of their threshold
        same = (c_ncp[i] == k and con.floating[i] == lit.floating[i]
                and rel([con.zpos[i], con.zsigma[i]], [lit.zpos[i], lit.zsigma[i]]) <= REGRESSION_TOL)
        if not same:
            assert mo["margin"].v <= REGRESSION_TOL, (name, i, "contract and literal decide differently", mo["margin"].v)
            flips += 1
            continue
        cg = c_pts[i, :k]
        ccols = [(cg["zdiff"], got["zdiff"]), (cg["zvar"], got["zvar"]), (cg["point"], got["point"]),
                 ([con.mprob[i]], [lit.mprob[i]]), ([c_zd[i]], [l_zd[i]]), ([c_zv[i]], [l_zv[i]])]
        WORST["contract"] = max(WORST.get("contract", 0.0), max(rel(a, b) for a, b in ccols))
        for a, b in ccols:
            assert rel(a, b) <= REGRESSION_TOL, (name, i)
    WORST["model"] = max(WORST.get("model", 0.0), worst)
    WORST["flips"] = max(WORST.get("flips", 0), flips)
    print(f"{name}: model vs literal oracle {worst:.3g}, contract vs literal {WORST.get('contract', 0.0):.3g}, "
          f"threshold flips {flips} of {n}")
    assert worst <= REGRESSION_TOL, (name, worst)
    assert flips <= n // 100, (name, flips)


@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_layout_inputs_spread_counts_and_weights(oracle, grid, name):
    """what makes the GPU comparison on these inputs worth its time: the particles of one step
    differ in their number of contact points, and from the second step on the weights are
    neither reset to uniform nor few"""
    m = len(L.LAYOUTS[name][0])
    cfg = layout_config(name, N_ORACLE)
    f = O.OracleFilter(cfg, O.SUM_CONTRACT)
    f.set_map(grid)
    f.init_gaussian(N_ORACLE, INIT["mu"], INIT["sigma"], INIT["z"], INIT["zs"])
    for k, st in enumerate(L.layout_stream(name)):
        assert f.step(st)
        p, info = f.download(), f.info()
        assert info.resampled == 1
        if m < 3:
            continue
        if k == 0:
            assert len(np.unique(p.n_contact_points)) >= 3, (name, np.unique(p.n_contact_points))
        else:
            assert info.uniform_reset == 0, (name, k)
            assert len(np.unique(p.weight)) > 100, (name, k)


def test_accepted_without_points_stores_the_canonical_nan(oracle, grid):
    """m = 0 with minContacts = 0: the reference's zPos and zSigma are NaN (the model and the
    literal oracle above); the contract oracle stores the canonical quiet NaN, whatever the
    host's processor generates for 0 * inf and 0 / 0"""
    cfg = layout_config("0", N_MODEL)
    f = O.OracleFilter(cfg, O.SUM_CONTRACT)
    f.set_map(grid)
    f.init_gaussian(N_MODEL, INIT["mu"], INIT["sigma"], INIT["z"], INIT["zs"])
    for st in L.layout_stream("0", 2):
        assert f.step(st)
        p = f.download()
        assert not p.floating.any() and not p.n_contact_points.any()
        for v in (p.zpos, p.zsigma):
            assert (np.ascontiguousarray(v).view(np.uint64) == 0x7ff8000000000000).all()


def test_layouts_cover_every_specialisation():
    for name, (feet, groups) in L.LAYOUTS.items():
        assert len(feet) == len(groups) <= A.MAX_CONTACTS
        assert len(set(feet)) == len(feet), name
        for x, y, z in feet:
            assert 0.3 - 1e-12 <= math.hypot(x, y + 0.2) <= 0.5 + 1e-12 and -0.21 <= z <= -0.18, name
    rows = {L.row_of(name) for name in L.LAYOUTS} | {L.row_of(name, True) for name in L.MAP_LAYOUTS}
    assert rows == set(L.ROWS)
    # the named layouts of each row
    assert L.row_of("3_ungrouped") == (4, True, False, True)
    assert L.row_of("4_in_2") == (4, True, False, False)
    assert L.row_of("5_mixed") == L.row_of("32_in_4") == (4, False, False, False)
    assert L.row_of("6_ungrouped") == L.row_of("8_ungrouped") == L.row_of("8_in_5") == (8, True, False, False)
    assert L.row_of("12_in_6") == L.row_of("12_in_8") == (8, False, False, False)
    assert L.row_of("9_ungrouped") == L.row_of("12_ungrouped") == L.row_of("32_in_16") == (32, False, False, False)
    assert L.row_of("4_in_2", True) == (4, True, True, False)
    assert L.row_of("6_ungrouped", True) == L.row_of("12_in_6", True) == (32, False, True, False)
    assert sum(L.group_ends(L.LAYOUTS["5_mixed"][1])) == 3 and sum(L.group_ends(L.LAYOUTS["8_in_5"][1])) == 5
    assert sum(L.group_ends(L.LAYOUTS["12_in_8"][1])) == 8 and sum(L.group_ends(L.LAYOUTS["32_in_4"][1])) == 4


def test_holey_and_window_cells(grid):
    base = S.rough_map(cells=200)
    empty = np.diff(grid.cell_start.astype(np.int64)) == 0
    assert 0.10 < empty.mean() < 0.14
    kept = ~empty
    counts = np.diff(base.cell_start.astype(np.int64))
    assert np.array_equal(np.diff(grid.cell_start.astype(np.int64))[kept], counts[kept])
    assert np.array_equal(grid.mean, base.mean[np.repeat(kept, counts)])
    # a cloud of 0.2 m around the origin, four feet of reach 0.56 m: (0.2 + 0.56 + 0.02 + 6
    # sqrt(2e-4) + 0.05) on either side at 0.1 m cells, -1 / +2 cells of padding
    pa = A.ParticleArrays(3)
    pa.x[:] = [-0.2, 0.2, math.nan]
    pa.y[:] = [-0.2, 0.2, math.inf]
    cfg = A.default_config()
    st = S.step_stream(1)[0]
    side = math.hypot(0.25, 0.5) + 0.02 + 6.0 * math.sqrt(2e-4) + 0.05 + 0.2
    cells = (math.floor(side * 10) + 2 + math.floor(side * 10) + 2) ** 2
    assert L.window_cells(pa, st, cfg, grid, max_weight=1.0) == cells
    assert L.window_cells(pa, st, cfg, grid, max_weight=0.0) > cells         # the spread's margin
    pa.x[0] = -30.0                                                          # off the map: clamped
    assert L.window_cells(pa, st, cfg, grid, max_weight=1.0) < 200 * 200
