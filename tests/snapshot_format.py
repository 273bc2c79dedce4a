"""A pure-Python reader (and, for the format test, writer) of the snapshot layout that
DESIGN.md 5e documents -- written from that description, not from the C++, so that the tests
which use it check the document (test infrastructure).

    snap = read(blob)
    snap.header["n"], snap.particles["x"], snap.grid["cell_start"], snap.particle_map(i)
"""
import struct

import numpy as np

MAGIC = b"ESLAMSNP"
VERSION = 1
HEADER_BYTES = 336
SEC_GRID, SEC_HASH, SEC_PARTICLES, SEC_SCALARS, SEC_MAPS = 1, 2, 4, 8, 16
SECTIONS = ("grid", "hash", "particles", "scalars", "maps")
NONE = 0xFFFFFFFF
PAGE_CELLS = 64
PAGE_BYTES = 512
SCALARS_BYTES = 320

# DESIGN.md 5e, "Header": name, struct code -- in file order, little-endian, no implicit padding
HEADER_FIELDS = [
    ("magic", "8s"), ("version", "I"), ("sections", "I"), ("bytes", "Q"), ("n", "Q"),
    ("particle_maps", "I"), ("local_map_trail", "I"), ("hx", "I"), ("hy", "I"), ("max_sensor_range", "d"),
    ("width", "I"), ("height", "I"), ("scale_x", "d"), ("scale_y", "d"), ("offset_x", "d"), ("offset_y", "d"),
    ("global2local", "12d"), ("n_patches", "Q"), ("has_height", "I"), ("hash_bins", "I"), ("hash_n", "Q"),
    ("tables", "Q"), ("pages", "Q"), ("wx", "I"), ("wy", "I"), ("row_words", "I"), ("pad", "I"),
    ("sections_off_size", "10Q"), ("reserved", "Q"),
]
HEADER_STRUCT = struct.Struct("<" + "".join(c for _, c in HEADER_FIELDS))
assert HEADER_STRUCT.size == HEADER_BYTES

PARTICLE_FIELDS = ("x", "y", "orientation", "zpos", "zsigma", "weight", "mprob")


def pad16(b):
    return (b + 15) & ~15


def row_words(w, v):
    """words of a table row: centre x, y, shadow, trail mark, the window's slots, 3 per trail entry; whole 16 bytes"""
    return (4 + w + 3 * v + 3) & ~3


def pack_header(h):
    vals = []
    for name, code in HEADER_FIELDS:
        v = h[name]
        if code in ("12d", "10Q"):
            vals.extend(v)
        else:
            vals.append(v)
    return HEADER_STRUCT.pack(*vals)


def unpack_header(blob):
    raw = HEADER_STRUCT.unpack_from(bytes(blob[:HEADER_BYTES]))
    h, k = {}, 0
    for name, code in HEADER_FIELDS:
        if code in ("12d", "10Q"):
            cnt = int(code[:-1])
            h[name] = list(raw[k:k + cnt])
            k += cnt
        else:
            h[name] = raw[k]
            k += 1
    return h


def section_sizes(h):
    """the size of every section as the header's counts give it (0: not present)"""
    ncell, np_, n = h["width"] * h["height"], h["n_patches"], h["n"]
    size = {
        "grid": pad16((ncell + 1) * 4) + pad16(np_ * 8) + (pad16(np_ * 4) if h["has_height"] else 0),
        "hash": 4 * pad16(h["hash_n"] * 8) + pad16(h["hash_n"] * 4) + pad16(h["hash_bins"] ** 2 * 4),
        "particles": 7 * pad16(n * 8) + pad16(n),
        "scalars": SCALARS_BYTES,
        "maps": pad16(n * 4) + pad16(h["tables"] * h["row_words"] * 4) + pad16(h["pages"] * 4) + h["pages"] * PAGE_BYTES,
    }
    return {s: (size[s] if h["sections"] & (1 << k) else 0) for k, s in enumerate(SECTIONS)}


def layout(h):
    """{section: (offset, size)} in file order behind the header, and the total size"""
    at, out = HEADER_BYTES, {}
    for k, (s, size) in enumerate(section_sizes(h).items()):
        out[s] = (0, 0)
        if h["sections"] & (1 << k):
            out[s] = (at, size)
            at += size
    return out, at


class Snapshot:
    def __init__(self, blob):
        self.blob = np.frombuffer(bytes(blob), np.uint8)
        h = self.header = unpack_header(self.blob)
        assert h["magic"] == MAGIC and h["version"] == VERSION
        want, total = layout(h)
        self.sections = {s: (h["sections_off_size"][2 * k], h["sections_off_size"][2 * k + 1]) for k, s in enumerate(SECTIONS)}
        assert self.sections == want and total == h["bytes"] == self.blob.shape[0]
        self._at = 0
        n, ncell, np_ = h["n"], h["width"] * h["height"], h["n_patches"]
        # grid: cell_start, patches {mean, stdev}, heights
        self._seek("grid")
        patch = None
        self.grid = {"cell_start": self._take("<u4", ncell + 1)}
        patch = self._take("<f4", 2 * np_).reshape(np_, 2)
        self.grid["mean"], self.grid["stdev"] = patch[:, 0].copy(), patch[:, 1].copy()
        self.grid["patch_height"] = self._take("<f4", np_) if h["has_height"] else None
        # pose hash: x, y, theta, z, the poses' buckets, the bucket sizes
        self.hash = None
        if h["sections"] & SEC_HASH:
            self._seek("hash")
            self.hash = {f: self._take("<f8", h["hash_n"]) for f in ("x", "y", "theta", "z")}
            self.hash["bucket"] = self._take("<i4", h["hash_n"])
            self.hash["bucket_sizes"] = self._take("<u4", h["hash_bins"] ** 2)
        # particles: seven fp64 arrays and the flags byte (contact points | floating << 7)
        self._seek("particles")
        self.particles = {f: self._take("<f8", n) for f in PARTICLE_FIELDS}
        flags = self._take("u1", n)
        self.particles["flags"] = flags
        self.particles["floating"] = flags >> 7
        self.particles["n_contact_points"] = flags & 0x7F
        # scalars: eslam_rng_state (280 bytes), 8 bytes of padding, wexp, minstd, max_weight, update_count, inv_n
        self._seek("scalars")
        raw = self._take("u1", SCALARS_BYTES).tobytes()
        r = struct.unpack_from("<IIQQQd12d34III", raw, 0)
        self.scalars = {"minstd_x": r[0], "project_count": r[2], "init_count": r[3], "hash_count": r[4], "rng_max_weight": r[5],
                        "ud_pose": list(r[6:18]), "libc_rand": list(r[18:52]), "libc_rand_pos": r[52]}
        w = struct.unpack_from("<iIdQd", raw, 288)
        self.scalars.update({"wexp": w[0], "minstd": w[1], "max_weight": w[2], "update_count": w[3], "inv_n": w[4]})
        # per-particle maps: sid, table rows, owner words, pages
        self.sid = self.tables = self.owner = self.pages = None
        if h["sections"] & SEC_MAPS:
            self._seek("maps")
            self.sid = self._take("<u4", n)
            self.tables = self._take("<u4", h["tables"] * h["row_words"]).reshape(h["tables"], h["row_words"])
            self.owner = self._take("<u4", h["pages"])
            self.pages = self._take("<f4", h["pages"] * PAGE_CELLS * 2).reshape(h["pages"], PAGE_CELLS, 2)
            assert self._at == self.sections["maps"][0] + self.sections["maps"][1]

    def _seek(self, s):
        self._at = self.sections[s][0]

    def _take(self, dtype, count):
        nbytes = np.dtype(dtype).itemsize * count
        a = np.frombuffer(self.blob[self._at:self._at + nbytes].tobytes(), dtype)
        self._at += pad16(nbytes)
        return a

    def table(self, k):
        """table k as a dict: centre, shadow, hw, slots (W), trail [(a, b, page)] (hw entries)"""
        h = self.header
        w = h["wx"] * h["wy"]
        r = self.tables[k]
        tr = r[4 + w:4 + w + 3 * h["local_map_trail"]].reshape(-1, 3)
        return {"centre": (int(np.int32(r[0])), int(np.int32(r[1]))), "shadow": int(r[2]), "hw": int(r[3]),
                "slots": r[4:4 + w], "trail": [(int(np.int32(a)), int(np.int32(b)), int(p)) for a, b, p in tr[:int(r[3])]]}

    def particle_map(self, i):
        """particle i's own patches (cells, mean, stdev): the window's tiles in slot order, then the
        trail's in entry order, each tile's cells row by row (as eslam_gpu_get_particle_map)"""
        h = self.header
        t = self.table(int(self.sid[i]))
        wx, wy, hx, hy = h["wx"], h["wy"], h["hx"], h["hy"]
        tiles = []
        for s, pg in enumerate(t["slots"]):
            if pg == NONE:
                continue
            lo_a, lo_b = t["centre"][0] - hx, t["centre"][1] - hy
            a = lo_a + ((s % wx) - lo_a) % wx          # the tile of slot column s % wx inside [c - h, c + h]
            b = lo_b + ((s // wx) - lo_b) % wy
            tiles.append((a, b, int(pg)))
        tiles += [(a, b, pg) for a, b, pg in t["trail"] if pg != NONE]
        cells, mean, stdev = [], [], []
        for a, b, pg in tiles:
            page = self.pages[pg]
            for j in range(PAGE_CELLS):
                if not page[j, 1] >= 0.0:
                    continue
                cells.append((8 * b + (j >> 3)) * h["width"] + 8 * a + (j & 7))
                mean.append(page[j, 0])
                stdev.append(page[j, 1])
        return np.array(cells, np.uint32), np.array(mean, np.float32), np.array(stdev, np.float32)


def read(blob):
    return Snapshot(blob)


def build(h, grid, particles, scalars_raw, sid=None, tables=None, owner=None, pages=None, hash_=None):
    """A blob from its parts (the format test's hand-built snapshots): h holds the header's counts
    (sections, offsets and the size are filled in here)."""
    h = dict(h)
    h.setdefault("magic", MAGIC)
    h.setdefault("version", VERSION)
    h.setdefault("pad", 0)
    h.setdefault("reserved", 0)
    h["sections_off_size"] = [0] * 10
    h["bytes"] = 0
    lay, total = layout(h)
    h["bytes"] = total
    h["sections_off_size"] = [v for s in SECTIONS for v in lay[s]]
    out = bytearray(pack_header(h))

    def put(a, dtype):
        b = np.ascontiguousarray(a, dtype=dtype).tobytes()
        out.extend(b + bytes(pad16(len(b)) - len(b)))

    put(grid["cell_start"], "<u4")
    put(np.stack([grid["mean"], grid["stdev"]], axis=1), "<f4")
    if h["has_height"]:
        put(grid["patch_height"], "<f4")
    if h["sections"] & SEC_HASH:
        for f in ("x", "y", "theta", "z"):
            put(hash_[f], "<f8")
        put(hash_["bucket"], "<i4")
        put(hash_["bucket_sizes"], "<u4")
    for f in PARTICLE_FIELDS:
        put(particles[f], "<f8")
    put(particles["flags"], "u1")
    assert len(scalars_raw) == SCALARS_BYTES
    out.extend(scalars_raw)
    if h["sections"] & SEC_MAPS:
        put(sid, "<u4")
        put(tables, "<u4")
        put(owner, "<u4")
        put(pages, "<f4")
    assert len(out) == total
    return bytes(out)
