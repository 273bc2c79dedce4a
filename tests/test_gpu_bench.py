"""bench.py on the GPU: a plain run times the steps and prints the headline line only, --full
adds the per-kernel pass and the CPU baseline, and --dump-outputs writes the particle set the
last timed step left (compared with the same steps run through GpuFilter here)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 300000                    # above bench.DUMP_SAMPLE: the dump is the seeded sample
CELLS = 200
STEPS, WARMUP = 3, 2
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernel_ms", "kernel_ms_note", "cpu_baseline")


def run_bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
                        str(WARMUP), "--particles", str(N), "--map-cells", str(CELLS)] + extra, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(gpu_mod, tmp_path):
    import eslam_abi as A
    import synthetic as S
    sys.path.insert(0, ROOT)
    import bench
    out = tmp_path / "dump"
    d = run_bench(["--dump-outputs", str(out)])
    for k in HEADLINE:
        assert k in d, k
    for k in FULL_ONLY:
        assert k not in d, k
    assert d["steps"] == STEPS and d["warmup"] == WARMUP
    # ms_per_step is rounded to 1e-4 ms: half a unit on a step of 0.01 ms or more is 0.5 %
    assert d["ms_per_step"] >= 0.01 and d["value"] == pytest.approx(N / d["ms_per_step"] / 1e3, rel=1e-2)

    f = gpu_mod.GpuFilter(S.bench_config(A.default_config(), N), device=0)
    f.set_map(S.flat_map(cells=CELLS))
    f.init_gaussian(N, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)
    for st in S.step_stream(WARMUP + STEPS):
        updated = f.step(st)
    info = f.sync()
    pa = f.download()
    f.close()

    got = {p.name[:-4]: np.load(p) for p in out.iterdir()}
    assert sorted(got) == sorted(list(A.ParticleArrays.FIELDS) + ["sample_index", "step_updated", "update_info"])
    assert sum(a.nbytes for a in got.values()) <= 64e6
    idx = got["sample_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < N
    for name, a in pa.as_dict().items():
        assert got[name].dtype == (np.float64 if a.dtype == np.float64 else np.float32), name
        assert np.array_equal(got[name], a[idx].astype(got[name].dtype)), name
    assert got["step_updated"][0] == float(updated)
    assert got["update_info"][0] == info.effective and got["update_info"][1] == info.weight_sum
    assert d["last_update"]["effective"] == info.effective


@pytest.mark.gpu
def test_full_run_adds_kernel_pass_and_cpu_baseline(gpu_mod, oracle):
    d = run_bench(["--full", "--cpu-sample", "4096", "--cpu-steps", "2"])
    for k in HEADLINE + FULL_ONLY:
        assert k in d, k
    assert d["kernel_ms"]["project_weight_ms"] > 0
    assert d["roofline"]["kernel"] in ("k_project_weight", "k_normalize_segments")
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["aos"]["value"] > 0
