"""The owning buffer, event and event-ring types and the Carver of csrc/eslam_buf.h, and the scratch
layouts of csrc/eslam_scratch.h (CPU only): tests/cpp/test_buf.cpp
supplies counting, malloc-backed stand-ins for the HIP calls they make and is built with ASan and
UBSan into tests/cpp/_build/ (git-ignored), so a double free, a leak or a use after free in the
owners fails here, with no HIP library linked and no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_buf.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "test_buf")
CSRC = os.path.join(ROOT, "slam-eslam_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "eslam_buf.h"), os.path.join(CSRC, "eslam_scratch.h"), os.path.join(CSRC, "eslam_internal.h"),
        os.path.join(ROOT, "include", "eslam_gpu.h"), os.path.join(ROOT, "include", "eslam_detmath.h")]
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
CXXFLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM_INCLUDE}", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined", "-g", "-O1", "-Wall", "-Wextra"]


def build(verbose=False):
    """g++ the program unless it is newer than its sources."""
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in DEPS):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + [SRC, "-o", EXE]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return EXE


def test_owners_free_grow_and_move_as_the_context_needs():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_buf ok" in r.stdout, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
