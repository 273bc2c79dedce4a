"""The model of a sharded filter's snapshot (snapshot_shard_ref.py) on hand-built blobs, no GPU:
the ranks' byte ranges tile the blob exactly once, one rank holding everything writes the blob
it loaded, and no slicing changes what a particle's own map shows."""
import os
import re
import struct

import numpy as np
import pytest

import eslam_abi as A
import snapshot_format as F
import snapshot_shard_ref as R

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eslam_gpu.h")

N = 7
SLICINGS = {1: [0, 7], 2: [0, 3, 7], 3: [0, 2, 5, 7]}


def hand_built(maps=True):
    """seven particles, five tables, seven pages (neither a multiple of 32):
      table 0 (particles 0, 2) and table 1 (particles 1, 4) are named from both sides of a boundary;
      page 0 is shared by tables 0, 1 and 3 and page 1 by tables 0 and 2, which fall on different sides;
      page 1's owner is table 0, outside every slice that holds table 2 only;
      tables 1 and 3 keep pages in trail entries."""
    width = height = 40
    v, wx = 2, 3
    w = wx * wx
    rw = F.row_words(w, v)
    sections = F.SEC_GRID | F.SEC_PARTICLES | F.SEC_SCALARS | (F.SEC_MAPS if maps else 0)
    h = {"sections": sections, "n": N, "particle_maps": int(maps), "local_map_trail": v if maps else 0,
         "hx": int(maps), "hy": int(maps), "max_sensor_range": 0.8, "width": width, "height": height, "scale_x": 0.1, "scale_y": 0.1,
         "offset_x": -2.0, "offset_y": -2.0, "global2local": [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], "n_patches": 3,
         "has_height": 1, "hash_bins": 0, "hash_n": 0, "tables": 5 if maps else 0, "pages": 7 if maps else 0,
         "wx": wx if maps else 0, "wy": wx if maps else 0, "row_words": rw if maps else 0}
    cells = np.zeros(width * height + 1, np.uint32)
    cells[5:] = 1
    cells[9:] = 3
    grid = {"cell_start": cells, "mean": np.array([0.1, 0.2, 0.3], np.float32), "stdev": np.array([0.01, 0.02, 0.03], np.float32),
            "patch_height": np.array([0.0, 0.1, 0.0], np.float32)}
    particles = {f: np.arange(N) * 0.5 + k for k, f in enumerate(F.PARTICLE_FIELDS)}
    particles["flags"] = np.array([0x84, 0x02, 0, 1, 0x80, 3, 4], np.uint8)
    scalars = struct.pack("<IIQQQd12d34III", 12345, 0, 7, 1, 3, 0.75, *range(12), *range(100, 134), 5, 0) + bytes(8) + \
        struct.pack("<iIdQd", 3, 12345, 0.75, 9, 1.0 / N)
    if not maps:
        return F.build(h, grid, particles, scalars)
    sid = [0, 1, 0, 2, 1, 3, 4]
    tables = np.zeros((5, rw), np.uint32)
    tables[:, 4:4 + w] = F.NONE
    tables[:, 4 + w + 2:4 + w + 3 * v:3] = F.NONE
    tr = 4 + w
    tables[0, :4] = [2, 2, 0, 0]
    tables[0, 4 + 7], tables[0, 4 + 8] = 0, 1
    tables[1, :4] = [3, 2, 1, 1]
    tables[1, 4 + 6] = 0
    tables[1, tr:tr + 3] = [0, 1, 2]
    tables[2, :4] = [1, 1, 0, 0]
    tables[2, 4 + 0], tables[2, 4 + 4] = 3, 1
    tables[3, :4] = [2, 3, 0, 2]
    tables[3, 4 + 1] = 4
    tables[3, tr:tr + 6] = [4, 4, 5, 0, 3, 0]
    tables[4, :4] = [np.uint32(-1 & 0xFFFFFFFF), 2, 0, 0]
    tables[4, 4 + 2] = 6
    pages = np.zeros((7, F.PAGE_CELLS, 2), np.float32)
    pages[:, :, 1] = -1.0
    for p in range(7):
        pages[p, (5 * p) % 64] = (0.5 + p, 0.05 + p)
        pages[p, 63 - p] = (0.25 + p, 0.01 * (p + 1))
    owner = np.array([F.NONE, 0, 1, 2, 3, F.NONE, 4], np.uint32)
    return F.build(h, grid, particles, scalars, sid=sid, tables=tables, owner=owner, pages=pages)


def parts_of(blob, bounds):
    return [R.reshard(blob, lo, hi) for lo, hi in zip(bounds, bounds[1:])]


def test_the_hand_built_blob_has_the_cases():
    s = F.read(hand_built())
    assert s.header["tables"] % 32 and s.header["pages"] % 32
    for ranks in (2, 3):
        b = SLICINGS[ranks]
        sides = [set(int(t) for t in s.sid[lo:hi]) for lo, hi in zip(b, b[1:])]
        assert any(sides[k] & sides[k + 1] for k in range(ranks - 1)), "a table named from both sides of a boundary"
    p2 = R.reshard(s, 3, 7)                       # holds tables 1, 2, 3, 4: not table 0
    assert 0 not in set(int(t) for t in s.sid[3:7])
    assert len(p2["pages"]) == 7 and list(p2["owner"]).count(F.NONE) == 3     # page 1's owner (table 0) is outside
    assert any(int(s.tables[t][3]) for t in set(int(t) for t in s.sid[3:7]))  # trail entries


@pytest.mark.parametrize("maps", [True, False])
@pytest.mark.parametrize("ranks", [1, 2, 3])
def test_rank_ranges_tile_the_blob_once(ranks, maps):
    blob = hand_built(maps)
    bounds = SLICINGS[ranks]
    parts = parts_of(blob, bounds)
    joined = R.join(parts)
    h = F.read(joined).header
    T = [len(p["tables"]) if maps else 0 for p in parts]
    P = [len(p["pages"]) if maps else 0 for p in parts]
    ranges = R.rank_ranges(h, bounds, T, P)
    assert len(ranges) == ranks
    hits = np.zeros(h["bytes"], np.uint8)
    for rr in ranges:
        for off, nbytes in rr:
            assert nbytes > 0 and off + nbytes <= h["bytes"]
            hits[off:off + nbytes] += 1
    assert hits.min() == 1 and hits.max() == 1
    assert ranges[0][0] == (0, F.HEADER_BYTES)
    for r in range(1, ranks):                    # the replicated pieces are rank 0's alone
        assert all(off >= F.HEADER_BYTES for off, _ in ranges[r])


@pytest.mark.parametrize("maps", [True, False])
def test_one_rank_holding_everything_writes_the_blob(maps):
    blob = hand_built(maps)
    assert R.join([R.reshard(blob, 0, N)]) == blob


@pytest.mark.parametrize("ranks", [2, 3])
def test_no_slicing_changes_a_particles_map(ranks):
    blob = hand_built()
    whole = F.read(blob)
    joined = R.join(parts_of(blob, SLICINGS[ranks]))
    s = F.read(joined)
    assert joined != blob and s.header["tables"] > whole.header["tables"]      # one copy per rank of the straddling tables
    for sec in ("grid", "particles", "scalars"):
        (a, n), (b, m) = s.sections[sec], whole.sections[sec]
        assert n == m and bytes(s.blob[a:a + n]) == bytes(whole.blob[b:b + m]), sec
    for i in range(N):
        for x, y in zip(s.particle_map(i), whole.particle_map(i)):
            assert np.array_equal(x, y), i
        assert len(whole.particle_map(i)[0]) > 0
    # loading the joined blob on the same layout and saving reproduces it
    assert R.join(parts_of(joined, SLICINGS[ranks])) == joined
    # and one rank loading it folds the copies' tables but not their pages: the maps are still the same
    one = F.read(R.join([R.reshard(joined, 0, N)]))
    for i in range(N):
        for x, y in zip(one.particle_map(i), whole.particle_map(i)):
            assert np.array_equal(x, y), i


def test_positional_forms_mirror_the_header():
    """the ctypes mirror of the positional forms names what include/eslam_gpu.h declares"""
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\bint (eslam_gpu_(?:save|load)_at)\s*\(", text))
    assert declared == set(A.SNAPSHOT_AT_PROTOTYPES) and len(declared) == 2
    assert "typedef int (*eslam_pwrite_fn)(void* user, uint64_t offset, const void* data, uint64_t bytes);" in text
    assert "typedef int (*eslam_pread_fn)(void* user, uint64_t offset, void* data, uint64_t bytes);" in text
