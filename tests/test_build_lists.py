"""The build lists of slam-eslam_amd/build_lib.py against the files in csrc/ (CPU only, no build):
a source missing from SOURCES is not compiled, a header missing from HEADERS leaves the build id
stale, and a PER_SOURCE key that matches no source is ignored without a word -- which would compile
k_project_weight without -disable-machine-licm (256 VGPRs, occupancy 1)."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-eslam_amd"))
import build_lib  # noqa: E402


def in_csrc(pattern):
    return {os.path.basename(p) for p in glob.glob(os.path.join(build_lib.CSRC, pattern))}


def test_sources_are_the_hip_files():
    assert len(build_lib.SOURCES) == len(set(build_lib.SOURCES))
    assert set(build_lib.SOURCES) == in_csrc("*.hip")


def test_every_header_is_hashed():
    hashed = {os.path.basename(h) for h in build_lib.HEADERS if os.path.dirname(h) == build_lib.CSRC}
    assert in_csrc("*.h") <= hashed
    assert all(os.path.exists(h) for h in build_lib.HEADERS)


def test_per_source_keys_are_sources():
    assert set(build_lib.PER_SOURCE) <= set(build_lib.SOURCES)


def test_k1_source_is_built_without_machine_licm():
    definition = re.compile(r"__global__[^;{]*\bk_project_weight\s*\(")
    defining = [s for s in build_lib.SOURCES if definition.search(open(os.path.join(build_lib.CSRC, s)).read())]
    assert len(defining) == 1, defining
    assert "-disable-machine-licm" in build_lib.PER_SOURCE.get(defining[0], [])
