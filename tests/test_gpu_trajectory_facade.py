"""The C++ façade's trajectory log (include/eslam_gpu.hpp over eslam_gpu_trajectory_*,
eslam_gpu_get_trajectories and eslam_gpu_trajectory_smoothed) on the GPU:
tests/cpp/test_facade_trajectory.cpp."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_trajectory_facade_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "test_facade_trajectory.cpp")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                    f"-I{os.path.join(ROOT, 'include')}", src], check=True)


@pytest.mark.gpu
def test_cpp_trajectory_facade():
    sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
    import build_lib
    exe = build_lib.build_facade_test(verbose=False, name="test_facade_trajectory")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trajectory facade OK" in r.stdout
