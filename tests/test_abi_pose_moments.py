"""The pose-moment entry point's ABI (CPU-side checks, no GPU calls): the two new structs have the C
layouts in ctypes, the library exports the symbols, and the ABI version has not moved."""
import ctypes as C
import os
import subprocess

import pytest

import eslam_abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "slam-eslam_amd", "lib", "libeslam_gpu.so")
STRUCTS = {"eslam_pose_gate": A.PoseGate, "eslam_pose_moments": A.PoseMoments}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import sys
        sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
        import build_lib
        build_lib.build(verbose=False)
    return C.CDLL(LIB)


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
    assert C.sizeof(A.PoseGate) == 48 and C.sizeof(A.PoseMoments) == 224


def test_restatement_sees_the_same_sizes():
    import moments_ref as R
    assert R.lib().moments_ref_sizeof(0) == C.sizeof(A.PoseGate)
    assert R.lib().moments_ref_sizeof(1) == C.sizeof(A.PoseMoments)


def test_symbols_exist(lib):
    assert hasattr(lib, "eslam_gpu_pose_moments") and hasattr(lib, "eslam_gpu_get_z_compensated_orientation")


def test_abi_version_is_still_8(lib):
    lib.eslam_gpu_abi_version.restype = C.c_int
    assert lib.eslam_gpu_abi_version() == 8


def test_null_arguments_are_refused_without_a_device(lib):
    lib.eslam_gpu_pose_moments.argtypes = [C.c_void_p, C.POINTER(A.PoseGate), C.POINTER(A.PoseMoments)]
    out = A.PoseMoments()
    assert lib.eslam_gpu_pose_moments(None, None, C.byref(out)) == A.ERR_INVALID_ARG
