"""Weight sums and normalisation at any weight scale on the device: the table of
weight_scale_cases.py through eslam_gpu_upload_particles, get_weights_sum, normalize_weights,
get_centroid, get_best_particle_index and resample, compared with the CPU oracle bit for bit, with
the k = 0 run of the device itself (a power-of-two scale moves only the sum), with weights_ref.py
within the derived bounds, and, for weights outside (0, finite), with the declared rule.  The
non-finite flags of k_weight_stats and the finalize's acc_value, and the update's S and Q with a
moved exponent, are device-only code: the outside-the-domain cases and the upload-then-step test
aim at them."""
import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import weight_scale_cases as W
import weights_ref as R

pytestmark = pytest.mark.gpu


def gpu_info(f):
    return f.sync()


def oracle_info(f):
    return f.info()


@pytest.mark.parametrize("rows", W.ROWS)
@pytest.mark.parametrize("n", W.SIZES)
def test_device_at_every_scale(gpu_mod, oracle, n, rows):
    cfg, J = W.config(n, rows), W.rows_of(rows, n)
    gpu, orc = gpu_mod.GpuFilter(cfg), O.OracleFilter(cfg, O.SUM_CONTRACT)
    base = W.run_case(gpu, gpu_info, n, W.scaled(n, ("p", 0)))
    for scale in W.SCALES:
        label = f"n={n} rows={rows} scale={W.scale_id(scale)}"
        w = W.scaled(n, scale)
        got = W.run_case(gpu, gpu_info, n, w)
        W.assert_same_run(got, W.run_case(orc, oracle_info, n, w), label + " (device, oracle)")
        if scale[0] == "p":
            W.assert_same_run(got, base, label + " (device, its k = 0 run)", k=scale[1])
        W.check_accuracy(got, W.reference(n, scale), n, J, label)
    gpu.close()


@pytest.mark.parametrize("rows", W.OUTSIDE_ROWS)
@pytest.mark.parametrize("n", W.OUTSIDE_SIZES)
def test_device_outside_the_domain(gpu_mod, oracle, n, rows):
    """bit for bit against the oracle (a NaN equals any NaN: which payload a division by NaN
    returns belongs to the processor), and against the declared rule"""
    cfg, J = W.config(n, rows), W.rows_of(rows, n)
    gpu, orc = gpu_mod.GpuFilter(cfg), O.OracleFilter(cfg, O.SUM_CONTRACT)
    for name, w in W.outside_cases(n, rows):
        label = f"n={n} rows={rows} {name}"
        got = W.run_case(gpu, gpu_info, n, w, full=False)
        W.assert_same_run(got, W.run_case(orc, oracle_info, n, w, full=False), label, nan_equal=True)
        W.check_rule(got, R.declared_rule(w.tolist(), J), n, J, label)
    gpu.close()


@pytest.mark.parametrize("n,rows", W.STEP_SIZES)
def test_upload_then_step(gpu_mod, oracle, n, rows):
    """upload base weights 2^k, three forced updates: K1's sa / sb and the finalize with a moved
    exponent.  Every field, effective, resampled and uniform_reset equal the k = 0 run's and the
    oracle's; weight_sum is 2^k times the k = 0 value at the first step and equal afterwards."""
    cfg = W.step_config(n, rows)
    runs = {}
    for k in W.STEP_K:
        gpu = gpu_mod.GpuFilter(cfg)
        runs[k] = W.run_steps(gpu, gpu_info, n, k)
        gpu.close()
        want = W.run_steps(O.OracleFilter(cfg, O.SUM_CONTRACT), oracle_info, n, k)
        W.assert_same_steps(runs[k], want, f"n={n} k={k} (device, oracle)")
    for k in W.STEP_K:
        W.assert_same_steps(runs[k], runs[0], f"n={n} k={k} (device, its k = 0 run)", k=k)


@pytest.mark.parametrize("first,stop", [(64, 129), (0, 193)])
def test_write_particles_rescales(gpu_mod, oracle, first, stop):
    """eslam_gpu_write_particles of weights 2^-200 into [first, stop) of a normalised filter sets
    the statistics' exponent from the whole set again (the oracle: download, edit, upload); the
    following normalize_weights equals the oracle's and lies within the bounds of weights_ref"""
    n, rows = 193, 0
    cfg, J = W.config(n, rows), W.rows_of(rows, n)
    gpu, orc = gpu_mod.GpuFilter(cfg), O.OracleFilter(cfg, O.SUM_CONTRACT)
    for f in (gpu, orc):
        f.upload(W.particles(n, W.scaled(n, ("p", 0))))
        f.normalize()
    pa = orc.download()
    assert W.same_bits(gpu.download().weight, pa.weight)
    pa.weight[first:stop] = np.ldexp(pa.weight[first:stop], -200)
    part = A.ParticleArrays(stop - first)
    for fld in W.FIELDS:
        getattr(part, fld)[:] = getattr(pa, fld)[first:stop]
    gpu.write(first, part)
    orc.upload(pa)
    w_in = np.array(pa.weight)
    out = []
    for f in (gpu, orc):
        total = f.weights_sum()
        eff = f.normalize()
        out.append((total, eff, np.array(f.download().weight)))
    assert W.same_bits(out[0][0], out[1][0]) and W.same_bits(out[0][1], out[1][1]), (out[0][:2], out[1][:2])
    assert W.same_bits(out[0][2], out[1][2])
    W.check_normalized(w_in, out[0][0], out[0][1], out[0][2], J, f"write [{first}, {stop})")
    gpu.close()
