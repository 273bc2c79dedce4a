"""The C++ façade's trajectory log on a sharded estimator (include/eslam_gpu.hpp over
eslam_gpu_trajectory_enable_sharded, one rank over the library's RCCL) on the GPU:
tests/cpp/test_facade_trajectory_sharded.cpp."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_trajectory_sharded_facade_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "test_facade_trajectory_sharded.cpp")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                    f"-I{os.path.join(ROOT, 'include')}", src], check=True)


@pytest.mark.gpu
def test_cpp_trajectory_sharded_facade():
    sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
    import build_lib
    exe = build_lib.build_facade_test(verbose=False, name="test_facade_trajectory_sharded")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade trajectory sharded OK" in r.stdout
