"""The snapshot format on the CPU: the pure-Python reader of DESIGN.md 5e's layout round-trips
a hand-built blob, and the ctypes mirror names what include/eslam_gpu.h declares."""
import ctypes as C
import os
import re
import struct

import numpy as np

import eslam_abi as A
import snapshot_format as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eslam_gpu.h")


def hand_built():
    """two particles, two tables, three pages: page 1 is shared by both tables, table 1 keeps
    page 2 in a trail entry and holds copies of grid cells (the shadow flag)"""
    width = height = 40
    v, wx = 2, 3                                       # trail entries; a 3 x 3 window (hx = hy = 1)
    w = wx * wx
    rw = F.row_words(w, v)
    h = {"sections": F.SEC_GRID | F.SEC_PARTICLES | F.SEC_SCALARS | F.SEC_MAPS, "n": 2, "particle_maps": 1, "local_map_trail": v,
         "hx": 1, "hy": 1, "max_sensor_range": 0.8, "width": width, "height": height, "scale_x": 0.1, "scale_y": 0.1,
         "offset_x": -2.0, "offset_y": -2.0, "global2local": [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], "n_patches": 3,
         "has_height": 0, "hash_bins": 0, "hash_n": 0, "tables": 2, "pages": 3, "wx": wx, "wy": wx, "row_words": rw}
    cells = np.zeros(width * height + 1, np.uint32)
    cells[5:] = 1
    cells[9:] = 3
    grid = {"cell_start": cells, "mean": np.array([0.1, 0.2, 0.3], np.float32), "stdev": np.array([0.01, 0.02, 0.03], np.float32)}
    particles = {f: np.array([k + 0.25, -(k + 0.5)]) for k, f in enumerate(F.PARTICLE_FIELDS)}
    particles["flags"] = np.array([0x84, 0x02], np.uint8)
    scalars = struct.pack("<IIQQQd12d34III", 12345, 0, 7, 1, 3, 0.75, *range(12), *range(100, 134), 5, 0) + bytes(8) + \
        struct.pack("<iIdQd", 3, 12345, 0.75, 9, 0.5)
    tables = np.full((2, rw), 0, np.uint32)
    tables[:, 4:4 + w] = F.NONE
    tables[:, 4 + w + 2:4 + w + 3 * v:3] = F.NONE
    # table 0: centre tile (2, 2); tile (2, 2) -> slot (2 % 3) + 3 (2 % 3) = 8 is page 0, tile (1, 2) -> slot 7 is page 1
    tables[0, :4] = [2, 2, 0, 0]
    tables[0, 4 + 8], tables[0, 4 + 7] = 0, 1
    # table 1: centre (3, 2), shadow; tile (3, 2) -> slot 0 + 3 * 2 = 6 is the shared page 1; trail entry 0: tile (0, 1), page 2
    tables[1, :4] = [3, 2, 1, 1]
    tables[1, 4 + 6] = 1
    tables[1, 4 + w:4 + w + 3] = [0, 1, 2]
    pages = np.zeros((3, F.PAGE_CELLS, 2), np.float32)
    pages[:, :, 1] = -1.0                              # stdev < 0: the cell holds no patch
    pages[0, 0], pages[0, 63] = (0.5, 0.05), (0.6, 0.06)
    pages[1, 9] = (0.7, 0.07)
    pages[2, 10] = (0.8, 0.08)
    owner = np.array([0, F.NONE, 1], np.uint32)
    blob = F.build(h, grid, particles, scalars, sid=[0, 1], tables=tables, owner=owner, pages=pages)
    return blob, h, grid, particles, tables, owner, pages


def test_reader_round_trips_a_hand_built_blob():
    blob, h, grid, particles, tables, owner, pages = hand_built()
    assert len(blob) % 16 == 0
    s = F.read(blob)
    for k, v in h.items():
        assert s.header[k] == v, k
    assert s.header["bytes"] == len(blob)
    for name, (off, size) in s.sections.items():
        assert off % 16 == 0 and size % 16 == 0, name
    assert s.sections["hash"] == (0, 0) and s.sections["grid"][0] == F.HEADER_BYTES
    assert np.array_equal(s.grid["cell_start"], grid["cell_start"]) and np.array_equal(s.grid["stdev"], grid["stdev"])
    for f in F.PARTICLE_FIELDS:
        assert np.array_equal(s.particles[f], particles[f])
    assert list(s.particles["floating"]) == [1, 0] and list(s.particles["n_contact_points"]) == [4, 2]
    assert s.scalars["minstd_x"] == s.scalars["minstd"] == 12345 and s.scalars["update_count"] == 9
    assert s.scalars["libc_rand"][33] == 133 and s.scalars["libc_rand_pos"] == 5 and s.scalars["wexp"] == 3
    assert np.array_equal(s.tables, tables) and np.array_equal(s.owner, owner) and np.array_equal(s.pages, pages)
    t1 = s.table(1)
    assert t1["shadow"] == 1 and t1["hw"] == 1 and t1["trail"] == [(0, 1, 2)] and t1["centre"] == (3, 2)
    # particle 0: slot 7 (tile (1, 2), page 1: cell 9 = (1, 1)) before slot 8 (tile (2, 2), page 0: cells 0 and 63)
    c, m, sd = s.particle_map(0)
    w = h["width"]
    assert list(c) == [(16 + 1) * w + 8 + 1, 16 * w + 16, (16 + 7) * w + 16 + 7]
    assert list(m) == [np.float32(0.7), np.float32(0.5), np.float32(0.6)]
    # particle 1: slot 6 is the shared page at tile (3, 2), then the trail's tile (0, 1), page 2: cell 10 = (2, 1)
    c, m, sd = s.particle_map(1)
    assert list(c) == [(16 + 1) * w + 24 + 1, (8 + 1) * w + 2]
    assert list(sd) == [np.float32(0.07), np.float32(0.08)]
    # the same bytes again from what the reader returned
    again = F.build(s.header, s.grid, s.particles, bytes(s.blob[s.sections["scalars"][0]:][:F.SCALARS_BYTES]), sid=s.sid,
                    tables=s.tables, owner=s.owner, pages=s.pages)
    assert again == blob


def test_abi_mirror_names_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"^int (eslam_gpu_(?:snapshot_size|save\w*|load\w*))\s*\(", text, flags=re.M))
    assert declared == set(A.SNAPSHOT_PROTOTYPES) and len(declared) == 5
    m = re.search(r"typedef struct eslam_snapshot_info \{(.*?)\} eslam_snapshot_info;", text, flags=re.S)
    fields = [f.strip() for decl in re.findall(r"uint(?:64|32)_t ([^;]+);", m.group(1)) for f in decl.split(",")]
    assert fields == [f for f, _ in A.SnapshotInfo._fields_]
    assert C.sizeof(A.SnapshotInfo) == 64
    assert int(re.search(r"#define ESLAM_SNAPSHOT_VERSION (\d+)", text).group(1)) == A.SNAPSHOT_VERSION == F.VERSION
    assert int(re.search(r"#define ESLAM_ABI_VERSION (\d+)", text).group(1)) == 8
    for name, bit in (("GRID", F.SEC_GRID), ("HASH", F.SEC_HASH), ("PARTICLES", F.SEC_PARTICLES), ("SCALARS", F.SEC_SCALARS),
                      ("MAPS", F.SEC_MAPS)):
        assert int(re.search(rf"#define ESLAM_SNAPSHOT_{name} (0x[0-9a-f]+)u", text).group(1), 16) == bit == getattr(A, "SNAPSHOT_" + name)
    assert "typedef int (*eslam_write_fn)(void* user, const void* data, uint64_t bytes);" in text
    assert "typedef int (*eslam_read_fn)(void* user, void* data, uint64_t bytes);" in text
