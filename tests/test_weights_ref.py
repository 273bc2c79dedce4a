"""Weight sums and normalisation at any weight scale, on the CPU oracle in contract mode (which the
device equals bit for bit: test_gpu_weight_scales.py) against weights_ref.py, the reference's
definitions in exact rational arithmetic.

(a) multiplying every weight by 2^k is exact on normal doubles, so it may move the weight sum by
    2^k and nothing else: no tolerance.
(b) at every scale, power of two or decimal, the sum, the normalised weights, the effective count
    and the centroid lie within the bounds derived in weight_scale_cases.py from the contract's
    rounding steps.  Bound and measured worst case over the whole table (CPU oracle, units of
    u = 2^-53), per J:

        quantity            bound                  J = 1    J = 3    J = 31
        sum                 (J + 6) u              1.99     1.99     1.99
        normalised weight   (J + 7) u              2.82     2.82     2.82
        effective count     (3 J + 22) u           4.90     4.88     4.88
        centroid (per A)    (4 J + 26 + 2 L) u     2.60     2.60     2.60
        mean yaw            the same + 8 u (trig)  within the 8 u

    (the worst cases sit at the small sizes, where every J sums the same single chunk; the
    J = 1 figures, 2e-16 to 5e-16, are those measured before on weights of natural scale)

(c) weights outside (0, finite): the declared rule of DESIGN.md 2 (weights_ref.declared_rule).

Before the statistics' exponent followed the largest weight below 1 (dm_stat_exp) and the squares
were taken of the scaled weights, (a) failed for every k <= -56 of the table (the chunk totals were
truncated at 2^-111 whatever the scale; k = -1 passed, the base weights being >= 2^-30) and for k >= 511 (w w and S S overflowed), and (b) from 1e-20 down (an
infinite effective count, then a sum off by up to 3e-3, then the uniform reset of a filter whose
weights were all positive) and from 1e153 up (effective NaN)."""
import numpy as np
import pytest

import oracle_ffi as O
import weight_scale_cases as W
import weights_ref as R


def oracle_filter(n, rows):
    return O.OracleFilter(W.config(n, rows), O.SUM_CONTRACT)


def info(f):
    return f.info()


@pytest.fixture(scope="module")
def base_runs(oracle):
    """the k = 0 run of every (n, rows), computed once"""
    return {(n, rows): W.run_case(oracle_filter(n, rows), info, n, W.scaled(n, ("p", 0))) for n in W.SIZES for rows in W.ROWS}


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    for J in sorted(w):
        print(f"J = {J}: worst errors in u: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(w[J].items())))


def test_table_is_what_it_says():
    for n in W.SIZES:
        w = W.base_weights(n)
        for k in W.POW2:
            s = W.scaled(n, ("p", k))                                # asserts normal and exact itself
            assert W.is_normal([float(W.reference(n, ("p", k)).S)]) and W.is_normal(s * s if abs(k) < 400 else s)
        x = W.poses(n)
        for c in (x.x, x.y, x.orientation, x.zpos):
            assert n < 8 or (np.any(c < 0) and np.any(c > 0))
        for rows in W.ROWS:
            J = W.rows_of(rows, n)
            chunks = [w[c:c + 64 * J] for c in range(0, n, 64 * J)]
            if len(chunks) > 1:
                assert any(np.all(c < 2.0 ** -20) for c in chunks), (n, rows)
    assert W.rows_of(31, 4097) == 31 and -(-4097 // (64 * 31)) == 3      # three chunks, the last ragged


@pytest.mark.parametrize("rows", W.ROWS)
@pytest.mark.parametrize("n", W.SIZES)
def test_power_of_two_scale_moves_only_the_sum(oracle, base_runs, n, rows):
    """(a)"""
    f = oracle_filter(n, rows)
    for k in W.POW2:
        got = W.run_case(f, info, n, W.scaled(n, ("p", k)))
        W.assert_same_run(got, base_runs[(n, rows)], f"n={n} rows={rows} k={k}", k=k)


@pytest.mark.parametrize("rows", W.ROWS)
@pytest.mark.parametrize("n", W.SIZES)
def test_accuracy_at_every_scale(oracle, worst, n, rows):
    """(b)"""
    f, J = oracle_filter(n, rows), W.rows_of(rows, n)
    for scale in W.SCALES:
        got = W.run_case(f, info, n, W.scaled(n, scale))
        W.check_accuracy(got, W.reference(n, scale), n, J, f"n={n} rows={rows} scale={W.scale_id(scale)}",
                         worst.setdefault(J, {}))


@pytest.mark.parametrize("rows", W.OUTSIDE_ROWS)
@pytest.mark.parametrize("n", W.OUTSIDE_SIZES)
def test_outside_the_domain(oracle, n, rows):
    """(c)"""
    f, J = oracle_filter(n, rows), W.rows_of(rows, n)
    names = []
    for name, w in W.outside_cases(n, rows):
        got = W.run_case(f, info, n, w, full=False)
        W.check_rule(got, R.declared_rule(w.tolist(), J), n, J, f"n={n} rows={rows} {name}")
        names.append(name)
    assert {"pos_inf", "neg_inf", "1e200_among_ones", "all_negative", "all_neg_zero", "all_pos_zero", "nan_at_0"} <= set(names)
    assert n == 65 and rows == 3 or {"nan_then_inf", "inf_then_nan", "negative_chunk"} <= set(names)


def test_reference_mode_agrees(oracle):
    """the oracle's reference mode (the reference's sequential sums) at the scales where the
    contract used to fail: within n u of the exact values"""
    n = 193
    for scale in (("d", 1e-300), ("d", 1e-33), ("d", 1e200), ("p", -960), ("p", 960)):
        f = O.OracleFilter(W.config(n, 0), O.SUM_REFERENCE)
        f.upload(W.particles(n, W.scaled(n, scale)))
        ref = W.reference(n, scale)
        assert W.rel_err(f.weights_sum(), ref.S) <= n * W.U
        assert W.rel_err(f.normalize(), ref.effective) <= 3 * n * W.U


@pytest.mark.parametrize("n,rows", W.STEP_SIZES)
def test_upload_then_step_is_scale_invariant(oracle, n, rows):
    """the update's S and Q with a moved exponent (the weighting squares w mprob unscaled, which
    is exact for |k| <= 400: DESIGN.md 2): every step equals the k = 0 run's"""
    runs = {k: W.run_steps(O.OracleFilter(W.step_config(n, rows), O.SUM_CONTRACT), info, n, k) for k in W.STEP_K}
    for k in W.STEP_K:
        W.assert_same_steps(runs[k], runs[0], f"n={n} k={k}", k=k)
