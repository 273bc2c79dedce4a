"""The CPU restatement of the KLD bin count (tests/c/kld_ref.c over eslam_detmath.h's dm_kld_*,
DESIGN.md 5h) against an independent numpy model (tests/kld_cases.py: np.floor, np.unique over
the key triples, the bound in Python floats) on every shared case; the closed forms; the clamp
order; the constant DM_INV_2PI; and the layout of the two new structs against their ctypes
mirrors.  No GPU."""
import ctypes as C
import math
import os
import subprocess
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

import eslam_abi as A
import kld_cases as K
import kld_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.cases()


def info_dict(info):
    d = info.as_dict()
    d["bound"] = np.float64(d["bound"]).view(np.uint64).item()
    return d


def model_dict(m):
    d = dict(m)
    d["bound"] = np.float64(d["bound"]).view(np.uint64).item()
    return d


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_numpy_model(case):
    name, x, y, th, w, params = case
    rc, info = R.count(x, y, th, w, **params)
    mrc, m = K.model(x, y, th, w, **params)
    assert rc == mrc, name
    assert info_dict(info) == model_dict(m), name
    assert info.particles_counted + info.particles_skipped == x.shape[0]


def test_cases_cover_what_they_claim():
    by = {c[0]: c for c in CASES}
    info = lambda n: R.count(*by[n][1:5], **by[n][5])      # noqa: E731
    assert info("too_spread")[0] == A.ERR_UNSUPPORTED and info("too_spread")[1].bins[0] > 100
    assert info("none_counted")[0] == 0 and info("none_counted")[1].samples == 17 and info("none_counted")[1].clamped == 1
    assert info("none_counted")[1].particles_counted == 0 and info("none_counted")[1].bins_occupied == 0
    for n in (257, 1000):
        assert info(f"skipped{n}")[1].particles_skipped == len(K.SKIP_KINDS)
    assert info("word_row_64")[1].bins_occupied == 64 and list(info("word_row_64")[1].bins) == [64, 1, 1]
    assert info("word_row_65")[1].bins_occupied == 65 and list(info("word_row_65")[1].bins) == [65, 1, 1]
    assert info("word_fan_64")[1].bins_occupied == 64 and list(info("word_fan_64")[1].bins) == [1, 1, 64]
    assert info("clamps")[1].samples == 400 and info("clamps")[1].clamped == 2
    assert info("held")[1].samples == 1000 and info("held")[1].clamped == 8


def test_one_bin_gives_n_min():
    for n in (1, 64, 1000):
        rc, info = R.count(*K.one_bin(n), n_min=250)
        assert rc == 0 and info.bins_occupied == 1 and info.bound == 0.0
        assert info.samples == 250 and info.clamped & 1
        assert list(info.bins) == [1, 1, 36] and list(info.origin) == [0, -1]


@pytest.mark.parametrize("m,t", [(1, 1), (3, 5), (8, 36), (5, 64)])
def test_full_lattice(m, t):
    rc, info = R.count(*K.lattice(m, t), theta_bins=t)
    assert rc == 0 and info.bins_occupied == m * m * t and list(info.bins) == [m, m, t]
    assert list(info.origin) == [-(m // 2), -(m // 2)] and info.particles_skipped == 0


def test_bound_table():
    """ceil(bound) at epsilon 0.05, z 2.3263478740408408; the raw values lie no closer than 0.03
    to an integer, so the last bits of the bound do not decide them"""
    table = {2: 66, 3: 93, 10: 217, 100: 1347, 1000: 11060, 100000: 1010424}
    for k, want in table.items():
        b = R.bound(k)
        assert math.ceil(b) == want, (k, b)
        assert min(b - math.floor(b), math.ceil(b) - b) >= 0.03, (k, b)
        assert np.float64(b).view(np.uint64) == np.float64(K.kld_bound(k, 0.05, K.Z99)).view(np.uint64)
        assert R.samples(b, 1, K.LIMIT, 0, 7, 0.0) == (want, 0)
    assert R.bound(0) == 0.0 and R.bound(1) == 0.0


def test_clamp_order_and_bits():
    lim = K.LIMIT
    S = R.samples
    assert S(100.5, 1, lim, 0, 5000, 0.0) == (101, 0)
    assert S(100.0, 1, lim, 0, 5000, 0.0) == (100, 0)                # an integral bound is its own ceiling
    assert S(100.5, 250, lim, 0, 5000, 0.0) == (250, 1)              # bit 0: raised to n_min
    assert S(100.5, 1, 80, 0, 5000, 0.0) == (80, 2)                  # bit 1: cut to the limit (n_max)
    assert S(100.5, 1, lim, 64, 5000, 0.0) == (64, 4)                # bit 2: cut to the capacity
    assert S(100.5, 1, lim, 0, 110, 0.1) == (110, 8)                 # bit 3: |101 - 110| = 9 <= 11
    assert S(100.5, 1, lim, 0, 113, 0.1) == (101, 0)                 # 12 > 11.3
    assert S(100.5, 1, lim, 0, 101, 0.0) == (101, 8)                 # at the count: held, trivially
    # in order: n_min first, then the limit wins over n_min, then the capacity, then the hold
    assert S(100.5, 300, 200, 0, 5000, 0.0) == (200, 3)
    assert S(100.5, 300, 200, 150, 5000, 0.0) == (150, 7)
    assert S(100.5, 300, 200, 150, 160, 0.1) == (160, 15)
    assert S(1e6, 1, 1000, 500, 5000, 0.0) == (500, 6)
    # a bound no count can hold is above every limit
    for b in (float("inf"), float("nan"), 2.0 ** 63, 1e300):
        assert S(b, 1, lim, 0, 5000, 0.0) == (lim, 2), b
        assert S(b, 1, 4000, 0, 5000, 0.0) == (4000, 2), b
    assert S(2.0 ** 63 - 1024.0, 1, 2 ** 64 - 1, 0, 5, 0.0) == (2 ** 63 - 1024, 0)
    assert S(-3.0, 1, lim, 0, 5000, 0.0) == (1, 1) and S(0.0, 1, lim, 0, 5000, 0.0) == (1, 1)
    for args in [(100.5, 250, lim, 0, 5000, 0.0), (1e6, 1, 1000, 500, 5000, 0.3), (100.5, 300, 200, 150, 160, 0.1)]:
        assert S(*args) == K.kld_samples(*args)


def test_inv_2pi_is_the_nearest_double():
    c = R.lib().kld_ref_inv_2pi()
    assert c == K.INV_2PI and c.hex() == "0x1.45f306dc9c883p-3"
    getcontext().prec = 60
    pi = Decimal("3.14159265358979323846264338327950288419716939937510582097494")
    exact = Fraction(1 / (2 * pi))
    err = abs(Fraction(c) - exact)
    assert err < abs(Fraction(np.nextafter(c, 1.0).item()) - exact) and err < abs(Fraction(np.nextafter(c, 0.0).item()) - exact)


def test_tiny_negative_yaw_lands_in_bin_zero():
    """theta = -1e-20: u = theta / 2 pi - floor(...) rounds to 1.0, the bin index to theta_bins"""
    u = -1e-20 * K.INV_2PI
    assert u - math.floor(u) == 1.0
    for tb in (1, 36, 4096):
        x, y, th, w = [np.array([v, v]) for v in (0.05, 0.05, 0.0, 0.5)]
        th[1] = -1e-20
        rc, info = R.count(x, y, th, w, theta_bins=tb)
        assert rc == 0 and info.bins_occupied == 1 and info.particles_counted == 2


def test_index_edges():
    """-0.0 and 0.0 share cell 0; the largest counted cell index is 2^31 - 1"""
    one = np.array([0.5])
    for xv, counted in ((2147483647.5, 1), (2147483648.0, 0), (-2147483648.0, 1), (-2147483648.5, 0)):
        rc, info = R.count(np.array([xv]), np.array([0.0]), np.array([0.0]), one, bin_xy=1.0)
        assert rc == 0 and info.particles_counted == counted, xv
        if counted:
            assert info.origin[0] == math.floor(xv)
    rc, info = R.count(np.array([-0.0, 0.0]), np.array([0.0, -0.0]), np.array([-0.0, 0.0]), np.array([0.5, 0.5]))
    assert info.bins_occupied == 1 and list(info.origin) == [0, 0]
    # the two extreme cells in one box: too spread, the box reported
    rc, info = R.count(np.array([-2147483648.0, 2147483647.0]), np.zeros(2), np.zeros(2), np.array([0.5, 0.5]), bin_xy=1.0)
    assert rc == A.ERR_UNSUPPORTED and list(info.bins) == [2 ** 32, 1, 36] and info.origin[0] == -2 ** 31


STRUCTS = {"eslam_kld_params": A.KldParams, "eslam_kld_info": A.KldInfo}


def test_struct_layouts_match_ctypes(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eslam_gpu.h"', "int main(void){"]
    for cname, py in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.split("\n") if l)
    for cname, py in STRUCTS.items():
        assert int(out[cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(py, f).offset, f"{cname}.{f}"
    assert (C.sizeof(A.KldParams), C.sizeof(A.KldInfo)) == (64, 88)


def test_params_default_of_the_library():
    """eslam_kld_params_default (host code of the library; no GPU call)"""
    lib = os.path.join(ROOT, "slam-eslam_amd", "lib", "libeslam_gpu.so")
    if not os.path.exists(lib):
        import sys
        sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
        import build_lib
        build_lib.build(verbose=False)
    L = C.CDLL(lib)
    cfg = A.default_config()
    cfg.particle_count = 1234
    p = A.KldParams(n_min=7, n_max=9, min_change=3.0, max_bins=5, multinomial=1)
    L.eslam_kld_params_default(C.byref(cfg), C.byref(p))
    got = tuple(getattr(p, f) for f, _ in A.KldParams._fields_)
    assert got == (0.1, 36, 0, 0.05, 2.3263478740408408, 1234, 0, 0.0, 0)
    L.eslam_kld_params_default(None, C.byref(p))
    assert p.n_min == 1
    d = A.KldParams()
    assert tuple(getattr(d, f) for f, _ in A.KldParams._fields_) == (0.1, 36, 0, 0.05, 2.3263478740408408, 1, 0, 0.0, 0)
