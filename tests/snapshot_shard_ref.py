"""A pure-Python model of a sharded filter's snapshot ("Sharded filters"), written
from that description on top of snapshot_format.py (test infrastructure).

    rank_ranges(header, bounds, T, P)   the byte ranges of the one blob that each rank writes
    reshard(blob, lo, hi)               what the rank holding particles [lo, hi) holds after a load
    join(parts)                         the blob a sharded save of those ranks writes

The blob of a sharded filter is the version-1 blob: rank 0 writes what every rank holds alike,
every rank its shard of the particle arrays and its tables and pages behind those of the ranks
below it.  A rank's tables and pages are its own (a table named from both sides of a shard
boundary is one copy per rank), each rank's in canonical order: tables by the lowest particle
of the rank naming them, pages by first reference.
"""
import numpy as np

import snapshot_format as F


def _arrays(h):
    """every array of the blob in file order: (name, units, unit bytes, how it is split)"""
    ncell, np_, n = h["width"] * h["height"], h["n_patches"], h["n"]
    out = [("header", F.HEADER_BYTES, 1, "lead")]
    out += [("cell_start", ncell + 1, 4, "lead"), ("patch", np_, 8, "lead")]
    if h["has_height"]:
        out.append(("patch_height", np_, 4, "lead"))
    if h["sections"] & F.SEC_HASH:
        out += [(f"hash_{f}", h["hash_n"], 8, "lead") for f in ("x", "y", "theta", "z")]
        out += [("hash_bucket", h["hash_n"], 4, "lead"), ("hash_sizes", h["hash_bins"] ** 2, 4, "lead")]
    out += [(f, n, 8, "shard") for f in F.PARTICLE_FIELDS] + [("flags", n, 1, "shard")]
    out.append(("scalars", F.SCALARS_BYTES, 1, "lead"))
    if h["sections"] & F.SEC_MAPS:
        out += [("sid", n, 4, "shard"), ("tables", h["tables"], h["row_words"] * 4, "tables"), ("owner", h["pages"], 4, "pages"),
                ("pages", h["pages"], F.PAGE_BYTES, "pages")]
    return out


def rank_ranges(header, bounds, T, P):
    """[[(offset, bytes), ...] per rank]: rank r writes particles [bounds[r], bounds[r + 1]), table
    rows [sum(T[:r]), +T[r]) and pages [sum(P[:r]), +P[r]); rank 0 the replicated pieces; the zero
    padding behind an array goes with the rank that holds the array's last element"""
    ranks = len(bounds) - 1
    assert bounds[0] == 0 and bounds[-1] == header["n"]
    if header["sections"] & F.SEC_MAPS:
        assert sum(T) == header["tables"] and sum(P) == header["pages"]
    out = [[] for _ in range(ranks)]
    at = 0
    for _, total, unit, split in _arrays(header):
        for r in range(ranks):
            if split == "lead":
                first, count = 0, (total if r == 0 else 0)
            elif split == "shard":
                first, count = bounds[r], bounds[r + 1] - bounds[r]
            elif split == "tables":
                first, count = sum(T[:r]), T[r]
            else:
                first, count = sum(P[:r]), P[r]
            if not count:
                continue
            nbytes = count * unit
            if first + count == total:
                nbytes += F.pad16(total * unit) - total * unit
            out[r].append((at + first * unit, nbytes))
        at += F.pad16(total * unit)
    assert at == header["bytes"]
    return out


def _page_words(h):
    """the words of a table row that name pages: the window's slots, then every trail entry's third word"""
    w, v = h["wx"] * h["wy"], h["local_map_trail"]
    return list(range(4, 4 + w)), [4 + w + 3 * e + 2 for e in range(v)]


def reshard(blob, lo, hi):
    """the slice [lo, hi) of a snapshot as its own filter: sid, tables, owner and pages under the
    slice's own compact ids (and the slice's particle arrays, for join)"""
    s = blob if isinstance(blob, F.Snapshot) else F.read(blob)
    h = s.header
    part = {"snap": s, "lo": lo, "hi": hi,
            "particles": {f: s.particles[f][lo:hi] for f in F.PARTICLE_FIELDS + ("flags",)}}
    if not h["sections"] & F.SEC_MAPS:
        part.update(sid=None, tables=None, owner=None, pages=None)
        return part
    slots, trail = _page_words(h)
    tmap, tlist = {}, []
    for i in range(lo, hi):                      # tables: by the lowest particle of the slice naming them
        t = int(s.sid[i])
        if t not in tmap:
            tmap[t] = len(tlist)
            tlist.append(t)
    pmap, plist = {}, []
    for t in tlist:                              # pages: by first reference (slots, then the used trail entries)
        row = s.tables[t]
        hw = int(row[3])
        for q in slots + trail[:hw]:
            p = int(row[q])
            if p != F.NONE and p not in pmap:
                pmap[p] = len(plist)
                plist.append(p)
    tables = s.tables[tlist].copy() if tlist else np.zeros((0, h["row_words"]), np.uint32)
    for k, t in enumerate(tlist):
        hw = int(tables[k, 3])
        for q in slots + trail[:hw]:
            if tables[k, q] != F.NONE:
                tables[k, q] = pmap[int(tables[k, q])]
    owner = np.array([tmap.get(int(s.owner[p]), F.NONE) if s.owner[p] != F.NONE else F.NONE for p in plist], np.uint32)
    part.update(sid=np.array([tmap[int(s.sid[i])] for i in range(lo, hi)], np.uint32), tables=tables, owner=owner,
                pages=s.pages[plist].copy() if plist else np.zeros((0, F.PAGE_CELLS, 2), np.float32))
    return part


def join(parts):
    """the blob the ranks holding `parts` (in rank order, adjacent slices from 0 to n) save together"""
    s = parts[0]["snap"]
    h = dict(s.header)
    assert parts[0]["lo"] == 0 and parts[-1]["hi"] == h["n"]
    assert all(a["hi"] == b["lo"] for a, b in zip(parts, parts[1:]))
    particles = {f: np.concatenate([p["particles"][f] for p in parts]) for f in F.PARTICLE_FIELDS + ("flags",)}
    scalars = bytes(s.blob[s.sections["scalars"][0]:][:F.SCALARS_BYTES])
    hash_ = None
    if s.hash is not None:
        hash_ = s.hash
    if not h["sections"] & F.SEC_MAPS:
        return F.build(h, s.grid, particles, scalars, hash_=hash_)
    slots, trail = _page_words(h)
    sid, tables, owner, pages = [], [], [], []
    tbase = pbase = 0
    for p in parts:
        sid.append(p["sid"] + np.uint32(tbase))
        t = p["tables"].copy()
        for q in slots + trail:                  # entries past the trail's mark hold none
            col = t[:, q]
            t[:, q] = np.where(col != F.NONE, col + np.uint32(pbase), col)
        tables.append(t)
        owner.append(np.where(p["owner"] != F.NONE, p["owner"] + np.uint32(tbase), p["owner"]).astype(np.uint32))
        pages.append(p["pages"])
        tbase += len(p["tables"])
        pbase += len(p["pages"])
    h["tables"], h["pages"] = tbase, pbase
    return F.build(h, s.grid, particles, scalars, sid=np.concatenate(sid), tables=np.concatenate(tables),
                   owner=np.concatenate(owner), pages=np.concatenate(pages), hash_=hash_)
