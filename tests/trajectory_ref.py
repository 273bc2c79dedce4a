"""The numpy restatement of the trajectory log's algebra -- test infrastructure.

A log is a ring of entries; an entry holds the particles' five columns as they stood at the end of
a step and `parent`, the slot of each particle's ancestor in the previous held entry.  `link[i]` is
the slot, in the newest entry, of the ancestor of the current particle i: the identity after a
record, composed with the ancestors of every resample since."""
import numpy as np

import moments_ref

COLUMNS = ("x", "y", "z", "yaw", "zsigma")
NODE = np.dtype([("step", "<u8"), ("slot", "<u4"), ("particles", "<u4"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("yaw", "<f8"),
                 ("zsigma", "<f8")])


class TrajectoryLog:
    def __init__(self, capacity, n):
        self.capacity = int(capacity)
        self.entries = []                      # oldest first: dicts of step, the five columns, parent
        self.link = np.arange(n, dtype=np.uint32)
        self.next_step = 0

    def clear(self, n):
        """a new particle set (upload, init, load) or trajectory_clear: empty, the link the identity"""
        self.entries = []
        self.link = np.arange(n, dtype=np.uint32)

    def compose(self, anc):
        """a resample: output i is a copy of particle anc[i]"""
        self.link = self.link[np.asarray(anc, dtype=np.int64)]

    def record(self, x, y, z, yaw, zsigma, anc=None):
        """the end of a step; anc: this step's resample's ancestors, None when it did not resample"""
        if anc is not None:
            self.compose(anc)
        cols = [np.array(c, dtype=np.float64) for c in (x, y, z, yaw, zsigma)]
        assert all(c.shape == self.link.shape for c in cols)
        e = dict(zip(COLUMNS, cols))
        e["step"] = self.next_step
        e["parent"] = self.link.copy()
        self.next_step += 1
        self.entries.append(e)
        if len(self.entries) > self.capacity:
            self.entries.pop(0)
        self.link = np.arange(len(cols[0]), dtype=np.uint32)

    def record_particles(self, pa, anc=None):
        """record() of an eslam_abi.ParticleArrays"""
        self.record(pa.x, pa.y, pa.zpos, pa.orientation, pa.zsigma, anc)

    def ancestor_maps(self, capacity=None):
        """a_k for the newest min(held, capacity) entries, oldest first: a_newest = link,
        a_{k-1} = parent_k[a_k]"""
        held = self.entries if capacity is None else self.entries[len(self.entries) - min(len(self.entries), capacity):]
        maps, a = [], self.link
        for e in reversed(held):
            maps.append(a)
            a = e["parent"][a.astype(np.int64)]
        return list(reversed(maps)), held

    def trace(self, indices, capacity=None):
        """the lineages of the current particles `indices`: a NODE array (len(indices), steps)"""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        maps, held = self.ancestor_maps(capacity)
        out = np.zeros((len(idx), len(held)), dtype=NODE)
        for k, (a, e) in enumerate(zip(maps, held)):
            slot = a[idx]
            out["step"][:, k] = e["step"]
            out["slot"][:, k] = slot
            out["particles"][:, k] = len(e["parent"])
            for c in COLUMNS:
                out[c][:, k] = e[c][slot.astype(np.int64)]
        return out

    def smoothed(self, w, capacity=None, sum_chunk_rows=0):
        """per held entry, oldest first: (step, distinct ancestors, PoseMoments) of the current
        particles' ancestors in it under the current weights w"""
        maps, held = self.ancestor_maps(capacity)
        out = []
        for a, e in zip(maps, held):
            s = a.astype(np.int64)
            rc, m = moments_ref.moments(e["x"][s], e["y"][s], e["z"][s], e["yaw"][s], e["zsigma"][s], w, None, sum_chunk_rows)
            assert rc == 0
            out.append((e["step"], len(np.unique(a)), m))
        return out
