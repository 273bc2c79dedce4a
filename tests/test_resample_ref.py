"""The CPU reference of the resample to a count (tests/c/resample_ref.c) pinned to what already
exists: the oracle's or_resample (contract mode) and or_resample_multinomial at samples == n,
and cases small enough to check by hand.  tests/test_gpu_resample_counts.py compares the device
with this reference."""
import numpy as np
import pytest

import eslam_abi as A
import resample_ref as R


def particles(weights, seed=5):
    """distinct, recognisable fields around the given weights"""
    n = len(weights)
    rng = np.random.default_rng(seed)
    pa = A.ParticleArrays(n)
    pa.x[:] = rng.normal(size=n)
    pa.y[:] = rng.normal(size=n)
    pa.orientation[:] = rng.uniform(-3, 3, size=n)
    pa.zpos[:] = rng.normal(size=n)
    pa.zsigma[:] = rng.uniform(0.01, 1, size=n)
    pa.weight[:] = weights
    pa.mprob[:] = rng.uniform(size=n)
    pa.floating[:] = rng.integers(0, 2, size=n)
    pa.n_contact_points[:] = rng.integers(0, 21, size=n)
    return pa


def gather(pa, anc, weight=None):
    """the particle set a resample with these ancestors leaves (weights carried, or all `weight`)"""
    out = A.ParticleArrays(len(anc))
    for f in A.ParticleArrays.FIELDS:
        getattr(out, f)[:] = getattr(pa, f)[anc]
    if weight is not None:
        out.weight[:] = weight
    return out


def weight_sets(n, rng):
    uniform = np.full(n, 1.0 / n)
    conc = rng.uniform(size=n) ** 12
    conc /= conc.sum()
    unnorm = rng.uniform(size=n) * (5.3 / (0.5 * n))
    short = rng.uniform(size=n) * (0.37 / (0.5 * n))          # sum about 0.37: stratified draws overrun it
    return {"uniform": uniform, "concentrated": conc, "unnormalised": unnorm, "short": short}


@pytest.mark.parametrize("n", [1, 77, 2049, 9000])
@pytest.mark.parametrize("kind", ["uniform", "concentrated", "unnormalised", "short"])
def test_stratified_at_n_is_the_oracles_resample(oracle, n, kind):
    """ancestors, overruns and the RNG state of or_resample in contract mode; the shift rule too:
    the reference is given 61 - (dm_weight_exp(sum) + 1), the oracle derives its own"""
    from parity_util import assert_bit_identical
    w = weight_sets(n, np.random.default_rng(n))[kind]
    pa = particles(w)
    orc = oracle.OracleFilter(A.default_config(), oracle.SUM_CONTRACT)
    orc.upload(pa)
    x0 = orc.rng_state().minstd_x
    assert x0 == R.minstd_seed(A.default_config().seed)
    S = orc.weights_sum()
    anc, over, x1 = R.stratified(w, n, x0, R.shift_of(S))
    orc.resample()
    assert np.array_equal(anc, orc.ancestors())
    assert x1 == orc.rng_state().minstd_x
    assert_bit_identical(orc.download(), gather(pa, anc), "stratified")
    assert over == orc.info().resample_overruns
    assert (over > 0) == (kind == "short" and n > 1) or n == 1


@pytest.mark.parametrize("n", [1, 64, 1000, 4099])
def test_multinomial_at_n_is_the_oracles_on_dyadic_weights(oracle, n):
    """dyadic weights (multiples of 2^-20 summing to exactly 1, zeros among them): the oracle's
    sequential double sums and the fixed-point sums are both exact, so the particles, the
    weights (1 / m = 1 / n: nothing is dropped) and the RNG state agree"""
    from parity_util import assert_bit_identical
    rng = np.random.default_rng(100 + n)
    units = rng.multinomial(1 << 20, rng.dirichlet(np.full(n, 0.3)))
    if n > 3:
        units[0] += units[1]; units[1] = 0               # zeros among them: a run, and the last one
        units[n // 2] += units[-1]; units[-1] = 0
    assert units.sum() == 1 << 20
    w = units.astype(np.float64) / (1 << 20)
    assert (w == 0).any() or n <= 3
    pa = particles(w)
    orc = oracle.OracleFilter(A.default_config(), oracle.SUM_CONTRACT)
    orc.upload(pa)
    x0 = orc.rng_state().minstd_x
    anc, dropped, x1 = R.multinomial(w, n, x0, R.shift_of(1.0))
    orc.L.or_resample_multinomial(orc.h, n)
    assert dropped == 0 and len(anc) == n
    assert orc.count() == n
    assert x1 == orc.rng_state().minstd_x
    assert_bit_identical(orc.download(), gather(pa, anc, 1.0 / n), "multinomial")
    assert not (w[anc] == 0).any()                       # a zero-weight particle is never drawn (U > 0 here)


def test_one_particle():
    for samples in (1, 5, 130):
        anc, over, x1 = R.stratified([1.0], samples, 42, R.shift_of(1.0))
        assert anc.tolist() == [0] * samples and over == 0
        anc, dropped, x2 = R.multinomial([1.0], samples, 42, R.shift_of(1.0))
        assert anc.tolist() == [0] * samples and dropped == 0
        assert x1 == x2                                  # both consumed `samples` draws
    # a sum below 1: the stratified draws beyond it are clamped to the only particle
    anc, over, _ = R.stratified([0.5], 100, 42, R.shift_of(0.5))
    assert anc.tolist() == [0] * 100 and 45 <= over <= 55


@pytest.mark.parametrize("where", ["first", "last"])
def test_all_mass_in_one_particle(where):
    n, samples = 50, 200
    w = np.zeros(n)
    i = 0 if where == "first" else n - 1
    w[i] = 1.0
    for fn in (R.stratified, R.multinomial):
        anc, beyond, _ = fn(w, samples, 7, R.shift_of(1.0))
        # U = 0 (minstd value 1) would pick particle 0 whatever its weight: not among these draws
        assert anc.tolist() == [i] * samples and beyond == 0


def test_weight_sum_a_quarter_keeps_the_draws_below_it():
    """weights summing to exactly 0.25: multinomial keeps the draws with U <= 0.25 (fx is
    monotone and 0.25 is exact in fixed point), counted here with the minstd stream alone"""
    n, samples, x0 = 64, 5000, 123457
    w = np.full(n, 0.25 / n)
    assert w.sum() == 0.25
    shift = R.shift_of(0.25)
    anc, dropped, x1 = R.multinomial(w, samples, x0, shift)
    u = R.uniforms(x0, samples)
    keep = u <= 0.25
    assert 0 < keep.sum() < samples
    assert len(anc) == int(keep.sum()) and dropped == samples - int(keep.sum())
    # the kept draws, in draw order, land on particle ceil(U / (0.25 / n)) - 1
    want = np.maximum(np.ceil(u[keep] * (n / 0.25)) - 1, 0).astype(np.uint32)
    assert np.array_equal(anc, want)
    # the stream moved on by `samples` draws
    a, m = 48271, 2147483647
    assert x1 == (pow(a, samples, m) * x0) % m


def test_multinomial_takes_the_first_of_an_equal_run():
    """zero weights have C_i = C_(i-1): a draw equal to that sum takes the first index of the run"""
    w = [0.0, 0.0, 0.5, 0.0, 0.0, 0.5, 0.0]
    anc, dropped, _ = R.multinomial(w, 4000, 99, R.shift_of(1.0))
    assert dropped == 0
    assert set(anc.tolist()) == {2, 5}
    anc, over, _ = R.stratified(w, 4000, 99, R.shift_of(1.0))
    assert over == 0 and set(anc.tolist()) == {2, 5} and np.all(np.diff(anc.astype(np.int64)) >= 0)
