"""The C++ façade's saveState(path) / loadState(path) (include/eslam_gpu.hpp over eslam_gpu_save_at /
eslam_gpu_load_at) on the GPU: tests/cpp/test_snapshot_facade_file.cpp."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_snapshot_facade_file_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "test_snapshot_facade_file.cpp")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                    f"-I{os.path.join(ROOT, 'include')}", src], check=True)


@pytest.mark.gpu
def test_cpp_snapshot_facade_file(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
    import build_lib
    exe = build_lib.build_facade_test(verbose=False, name="test_snapshot_facade_file")
    r = subprocess.run([exe, str(tmp_path / "state.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "snapshot facade file OK" in r.stdout
