"""The trajectory log's ABI (CPU-side checks, no GPU calls): the three new structs have the C
layouts in ctypes, the library exports the six entry points, the ABI version and eslam_config have
not moved, and null arguments are refused before anything touches a device."""
import ctypes as C
import os
import subprocess

import pytest

import eslam_abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "slam-eslam_amd", "lib", "libeslam_gpu.so")
STRUCTS = {"eslam_trajectory_info": A.TrajectoryInfo, "eslam_trajectory_pose": A.TrajectoryPose,
           "eslam_trajectory_estimate": A.TrajectoryEstimate}
SYMBOLS = ["eslam_gpu_trajectory_enable", "eslam_gpu_trajectory_disable", "eslam_gpu_trajectory_clear", "eslam_gpu_trajectory_info",
           "eslam_gpu_get_trajectories", "eslam_gpu_trajectory_smoothed"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import sys
        sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
        import build_lib
        build_lib.build(verbose=False)
    return C.CDLL(LIB)


def test_struct_layouts_match_ctypes(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eslam_gpu.h"', "int main(void){",
             'printf("eslam_config %zu\\n", sizeof(eslam_config));']
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
    assert C.sizeof(A.TrajectoryInfo) == 56 and C.sizeof(A.TrajectoryPose) == 56
    assert C.sizeof(A.TrajectoryEstimate) == 16 + C.sizeof(A.PoseMoments) == 240
    # the log is created by a call, not by a config field
    assert int(out["eslam_config"]) == C.sizeof(A.Config)


def test_symbols_exist(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def test_abi_version_is_still_8(lib):
    lib.eslam_gpu_abi_version.restype = C.c_int
    assert lib.eslam_gpu_abi_version() == 8


def test_null_arguments_are_refused_without_a_device(lib):
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    lib.eslam_gpu_trajectory_enable.argtypes = [vp, C.c_uint32, C.c_uint64]
    lib.eslam_gpu_trajectory_disable.argtypes = [vp]
    lib.eslam_gpu_trajectory_clear.argtypes = [vp]
    lib.eslam_gpu_trajectory_info.argtypes = [vp, C.POINTER(A.TrajectoryInfo)]
    lib.eslam_gpu_get_trajectories.argtypes = [vp, u64p, C.c_uint64, C.POINTER(A.TrajectoryPose), C.c_uint64, u64p]
    lib.eslam_gpu_trajectory_smoothed.argtypes = [vp, C.POINTER(A.TrajectoryEstimate), C.c_uint64, u64p]
    assert lib.eslam_gpu_trajectory_enable(None, 4, 16) == A.ERR_INVALID_ARG
    assert lib.eslam_gpu_trajectory_disable(None) == A.ERR_INVALID_ARG
    assert lib.eslam_gpu_trajectory_clear(None) == A.ERR_INVALID_ARG
    info = A.TrajectoryInfo()
    assert lib.eslam_gpu_trajectory_info(None, C.byref(info)) == A.ERR_INVALID_ARG
    idx, steps = C.c_uint64(0), C.c_uint64(7)
    node, est = A.TrajectoryPose(), A.TrajectoryEstimate()
    assert lib.eslam_gpu_get_trajectories(None, C.byref(idx), 1, C.byref(node), 1, C.byref(steps)) == A.ERR_INVALID_ARG
    assert steps.value == 0
    steps.value = 7
    assert lib.eslam_gpu_trajectory_smoothed(None, C.byref(est), 1, C.byref(steps)) == A.ERR_INVALID_ARG
    assert steps.value == 0
