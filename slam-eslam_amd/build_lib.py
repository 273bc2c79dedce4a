"""Build libeslam_gpu.so (gfx950) in-tree with hipcc -- no cmake, no JIT cache.

    python slam-eslam_amd/build_lib.py            # rebuild unless the library's build id matches
    python slam-eslam_amd/build_lib.py --force

The library is the product: HIP kernels + the C ABI of include/eslam_gpu.h.
-ffp-contract=off keeps device and host arithmetic bit-identical to the CPU oracle.
Machine-LICM is disabled for the step kernels' translation units only (PER_SOURCE): in
eslam_kernels.hip it hoists the ~150 fp64 polynomial constants of the contact model out of the
particle loop and drives k_project_weight to 256 VGPRs / occupancy 1.

Provenance: the SHA-256 of every source, of every header they include (HEADERS: the seven in
csrc/ -- device-visible layouts, launcher declarations, buffer owners, scratch layouts, the host
side's context, the wave primitives, the diagnostic stamps -- and the two public ones)
and of every flag is compiled into the library (eslam_gpu_build_id()).  A build is skipped only when the existing library reports the hash
of the current sources, so a run never loads a binary that was not built from them
(tests/test_abi.py checks the shipped library the same way).
"""
import ctypes
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "lib")
LIB = os.path.join(OUT_DIR, "libeslam_gpu.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("ESLAM_OFFLOAD_ARCH", "gfx950")

SOURCES = ["eslam_kernels.hip", "eslam_particle_maps.hip", "eslam_selftest.hip",
           "eslam_resample.hip", "eslam_hash.hip", "eslam_shared_map.hip", "eslam_snapshot.hip",
           "eslam_scan.hip", "eslam_particle_grid.hip", "eslam_gmm.hip", "eslam_moments.hip", "eslam_kld.hip", "eslam_trajectory.hip", "eslam_ctx.hip", "eslam_host_comm.hip",
           "eslam_host_map.hip", "eslam_host_stats.hip", "eslam_host_trajectory.hip", "eslam_host_snapshot.hip"]
HEADERS = [os.path.join(CSRC, "eslam_internal.h"), os.path.join(CSRC, "eslam_launch.h"), os.path.join(CSRC, "eslam_buf.h"),
           os.path.join(CSRC, "eslam_scratch.h"), os.path.join(CSRC, "eslam_ctx.h"),
           os.path.join(CSRC, "eslam_wave.h"), os.path.join(CSRC, "eslam_stamps.h"),
           os.path.join(ROOT, "include", "eslam_gpu.h"), os.path.join(ROOT, "include", "eslam_detmath.h")]
FLAGS = ["-O3", f"--offload-arch={ARCH}", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-mfma", "-Wall", "-Wno-unused-result", "-Wno-unused-function", f"-I{os.path.join(ROOT, 'include')}"]
# Only eslam_kernels.hip (k_project_weight) is known to need the flag.  The other two were one
# translation unit with it and have always been compiled this way: dropping it from any of them
# is a separate, measured change.  tests/test_build_lists.py checks the keys against SOURCES.
NO_LICM = ["-mllvm", "-disable-machine-licm"]
PER_SOURCE = {"eslam_kernels.hip": NO_LICM, "eslam_particle_maps.hip": NO_LICM, "eslam_selftest.hip": NO_LICM}


def source_hash(defines=(), extra=()):
    """SHA-256 over the build inputs: every source and header, the flags, the defines."""
    h = hashlib.sha256()
    for path in [os.path.join(CSRC, s) for s in SOURCES] + HEADERS:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as fh:
            h.update(fh.read())
    flags = [f.replace(ROOT, "<root>") for f in FLAGS]      # location-independent (the GPU box's copy)
    h.update(repr((flags, PER_SOURCE, list(defines), list(extra), ARCH)).encode())
    return h.hexdigest()


def library_build_id(lib=LIB):
    """The build id compiled into a built library (None if it cannot be loaded)."""
    if not os.path.exists(lib):
        return None
    try:
        L = ctypes.CDLL(lib)
        L.eslam_gpu_build_id.restype = ctypes.c_char_p
        return L.eslam_gpu_build_id().decode()
    except (OSError, AttributeError):
        return None


def build(force=False, verbose=True, defines=(), lib=None, tag=""):
    """defines: extra -D macros (ablation builds only); lib/tag: alternative output names."""
    os.makedirs(OUT_DIR, exist_ok=True)
    lib = lib or LIB
    extra = os.environ.get("ESLAM_EXTRA_FLAGS", "").split()     # experiment builds only
    bid = source_hash(defines, extra)
    if not force and library_build_id(lib) == bid:
        return lib
    objs = []
    for src in SOURCES:
        path = os.path.join(CSRC, src)
        obj = os.path.join(OUT_DIR, src + tag + ".o")
        objs.append(obj)
        cmd = [HIPCC] + FLAGS + PER_SOURCE.get(src, []) + extra + ["-D" + d for d in defines]
        if src == "eslam_ctx.hip":
            cmd.append(f'-DESLAM_BUILD_ID="{bid}"')
        cmd += ["-c", path, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", lib] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return lib


FACADE_SRC = os.path.join(ROOT, "tests", "cpp", "test_facade.cpp")
FACADE_BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_facade")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_facade_test(verbose=True, name="test_facade"):
    """g++ a C++ façade test (include/eslam_gpu.hpp over the C ABI) against the library:
    tests/cpp/<name>.cpp -> tests/cpp/_build/<name> (test_facade, test_facade_shared_map,
    test_snapshot_facade, test_snapshot_facade_file, test_facade_scan, test_facade_resample,
    test_facade_resample_sharded, test_facade_particle_grid, test_facade_gmm, test_facade_kld, test_facade_moments, test_facade_trajectory,
    test_facade_trajectory_sharded)."""
    src = os.path.join(os.path.dirname(FACADE_SRC), name + ".cpp")
    exe = os.path.join(os.path.dirname(FACADE_BIN), name)
    deps = [src, LIB, os.path.join(ROOT, "include", "eslam_gpu.hpp"), os.path.join(ROOT, "include", "eslam_gpu.h")]
    if not _stale(exe, deps):
        return exe
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", f"-I{os.path.join(ROOT, 'include')}", src,
           f"-L{OUT_DIR}", "-leslam_gpu", "-Wl,-rpath,$ORIGIN/../../../slam-eslam_amd/lib", "-o", exe]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return exe


if __name__ == "__main__":
    defs = [a[2:] for a in sys.argv[1:] if a.startswith("-D")]
    tag = "_" + "_".join(d.lower() for d in defs) if defs else ""
    build(force="--force" in sys.argv, defines=defs, tag=tag,
          lib=os.path.join(OUT_DIR, f"libeslam_gpu{tag}.so") if defs else None)
