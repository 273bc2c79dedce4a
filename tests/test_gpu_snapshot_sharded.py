"""Snapshots of a sharded filter ("Sharded filters"): the ranks write one version-1
blob between them through eslam_gpu_save_at, and any layout -- other ranks, one GPU -- loads
its part of it through eslam_gpu_load_at and continues bit for bit.

The ranks are gloo processes sharing the one GPU (tests/snapshot_dist_worker.py); what a
sharded save must write is modelled in tests/snapshot_shard_ref.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eslam_abi as A
import snapshot_format as F
import snapshot_shard_ref as R
import snapshot_shard_scenarios as SC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = 4096                                     # chunk_bytes: runs and rows split across many chunks


def launch(name, n_global, world, tmp, program, tag, timeout=240, mem="host"):
    """Run the ranks on `program`; they meet through a FileStore in `tmp`.  Every rank is under a
    time limit, and its expiry kills all of them.  mem: the worker's exchange ('host', 'device' or 'rccl')."""
    store = os.path.join(tmp, f"store_{tag}")
    if os.path.exists(store):
        os.remove(store)
    procs, outs = [], []
    for r in range(world):
        out = os.path.join(tmp, f"{tag}_{r}.npz")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), ESLAM_DIST_STORE=store, OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "snapshot_dist_worker.py"), name, str(n_global), out,
                                       json.dumps(program), mem], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        outs.append(out)
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    bad = [f"--- rank {r} (exit {p.returncode}) ---\n{log[-2500:]}" for r, (p, log) in enumerate(zip(procs, logs)) if p.returncode != 0]
    assert not bad, "\n".join(bad)
    return [dict(np.load(o)) for o in outs]


def blob_of(path):
    return open(path, "rb").read()


_single = {}


def single(gpu_mod, name, n_global):
    """the one-GPU filter: snapshot B at the scenario's save point, E three steps later, and the
    update infos of those steps (computed once per scenario and size)"""
    key = (name, n_global)
    if key not in _single:
        f = gpu_mod.GpuFilter(SC.config(name, n_global))
        SC.prepare(f, name, n_global, 0, n_global)
        k = SC.SAVE_AT[name]
        SC.advance(f, name, 0, k, {})
        b = f.save_state().tobytes()
        rec = {}
        SC.advance(f, name, k, k + SC.MORE, rec)
        e = f.save_state().tobytes()
        f.close()
        _single[key] = (b, e, rec)
    return _single[key]


def table_maps(s):
    """every table's map as particle_map() gives it for a particle naming the table"""
    h = s.header
    out = []
    for k in range(h["tables"]):
        t = s.table(k)
        wx, wy, hx, hy = h["wx"], h["wy"], h["hx"], h["hy"]
        lo_a, lo_b = t["centre"][0] - hx, t["centre"][1] - hy
        tiles = [(lo_a + ((q % wx) - lo_a) % wx, lo_b + ((q // wx) - lo_b) % wy, int(pg)) for q, pg in enumerate(t["slots"]) if pg != F.NONE]
        tiles += [(a, b, pg) for a, b, pg in t["trail"] if pg != F.NONE]
        cells, mean, stdev = [], [], []
        for a, b, pg in tiles:
            page = s.pages[pg]
            j = np.nonzero(page[:, 1] >= 0.0)[0]
            cells.append(((8 * b + (j >> 3)) * h["width"] + 8 * a + (j & 7)).astype(np.uint32))
            mean.append(page[j, 0])
            stdev.append(page[j, 1])
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
        out.append((cat(cells, np.uint32), cat(mean, np.float32), cat(stdev, np.float32)))
    return out


def assert_same_filter(got, want, label):
    """two snapshots of one filter under different layouts: the particle and scalar sections byte
    for byte (and the grid and hash), and every particle's own map"""
    g, w = F.read(got), F.read(want)
    for sec in ("grid", "hash", "particles", "scalars"):
        (a, n), (b, m) = g.sections[sec], w.sections[sec]
        assert n == m and bytes(g.blob[a:a + n]) == bytes(w.blob[b:b + m]), f"{label}: section {sec} differs"
    if w.sid is None:
        assert got == want, label
        return
    gm, wm = table_maps(g), table_maps(w)
    n = w.header["n"]
    for i in range(0, n, max(n // 16, 1)):       # the fast form against the reader's own, on a sample
        for x, y in zip(g.particle_map(i), gm[int(g.sid[i])]):
            assert np.array_equal(x, y), (label, i)
    some = 0
    for i in range(n):
        a, b = gm[int(g.sid[i])], wm[int(w.sid[i])]
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{label}: particle {i}'s map differs"
        some += len(a[0])
    assert some > 0, label


def assert_infos(parts, rec, label):
    assert rec
    for r, p in enumerate(parts):
        for key, v in rec.items():
            assert np.array_equal(p[key].view(np.uint64), v.view(np.uint64)), f"{label}: rank {r} {key}"


@pytest.mark.parametrize("n_global,world", [(3000, 2), (1500, 3)])
def test_shared_map_bytes_equal_one_gpu(gpu_mod, tmp_path, n_global, world):
    """pose hash on, shared map: the ranks' file is the one-GPU filter's blob byte for byte, saved
    after a run from init and after a load of the one-GPU blob and three more steps"""
    b, b1, rec = single(gpu_mod, "hash", n_global)
    tmp = str(tmp_path)
    fb, f0, f1 = (os.path.join(tmp, x) for x in ("B.snap", "F0.snap", "F1.snap"))
    open(fb, "wb").write(b)
    k = SC.SAVE_AT["hash"]
    parts = launch("hash", n_global, world, tmp, [["prepare"], ["steps", 0, k], ["save", f0, 0], ["load", fb, 0],
                                                  ["steps", k, k + SC.MORE], ["save", f1, SMALL]], f"hash{world}")
    assert blob_of(f0) == b, "the ranks' run from init"
    assert blob_of(f1) == b1, "the ranks' run continued from the one-GPU blob"
    bounds = SC.bounds("hash", n_global, world)
    for r, p in enumerate(parts):
        save = [v for key, v in sorted(p.items()) if key.endswith("/save")][0]
        assert list(save[:4]) == [len(b), n_global, 0, 0]                 # the filter's, on every rank
        assert int(p["op3/count"][0]) == bounds[r + 1] - bounds[r]
    assert_infos(parts, {key: v for key, v in rec.items()}, "hash")


@pytest.mark.parametrize("name,world", [("maps", 2), ("maps", 3), ("heirloom", 2), ("heirloom", 3)])
def test_particle_maps_against_the_model(gpu_mod, tmp_path, name, world):
    """per-particle maps: the ranks load the one-GPU blob and save at once what the model says
    (whole and in 4 KiB chunks), and then continue as the one-GPU filter does"""
    n_global = 1500
    b, e, rec = single(gpu_mod, name, n_global)
    bounds = SC.bounds(name, n_global, world)
    sb = F.read(b)
    if name == "heirloom":                       # one table under particles on both sides of a boundary
        assert any(set(sb.sid[bounds[r]:bounds[r + 1]].tolist()) & set(sb.sid[bounds[r + 1]:bounds[r + 2]].tolist()) for r in range(world - 1))
    tmp = str(tmp_path)
    fb, fs, fs4, fe = (os.path.join(tmp, x) for x in ("B.snap", "S.snap", "S4.snap", "E.snap"))
    open(fb, "wb").write(b)
    k = SC.SAVE_AT[name]
    parts = launch(name, n_global, world, tmp, [["load", fb, 0], ["save", fs, 0], ["load", fb, SMALL], ["save", fs4, SMALL],
                                                ["steps", k, k + SC.MORE], ["save", fe, 0]], f"{name}{world}")
    want = R.join([R.reshard(sb, lo, hi) for lo, hi in zip(bounds, bounds[1:])])
    assert blob_of(fs) == want, "load_at + save_at against the model"
    assert blob_of(fs4) == want, "the same in 4 KiB chunks"
    hs = F.read(want).header
    for p in parts:
        assert list(p["op1/save"][:4]) == [len(want), n_global, hs["tables"], hs["pages"]]
        assert int(p["op3/save"][4]) > int(p["op1/save"][4])             # many more chunks
    assert_same_filter(blob_of(fe), e, f"{name} world {world}")
    assert_infos(parts, rec, name)


def test_resharding(gpu_mod, tmp_path):
    """a file written by 2 ranks loads on 3 ranks and on one GPU, and both continue as the
    uninterrupted one-GPU filter; the same 2 ranks loading it write its bytes again"""
    name, n_global = "maps", 1500
    _, e, rec = single(gpu_mod, name, n_global)
    tmp = str(tmp_path)
    f2, f2b, f2c, e3 = (os.path.join(tmp, x) for x in ("F2.snap", "F2b.snap", "F2c.snap", "E3.snap"))
    k = SC.SAVE_AT[name]
    launch(name, n_global, 2, tmp, [["prepare"], ["steps", 0, k], ["save", f2, 0], ["load", f2, SMALL], ["save", f2b, 0],
                                    ["load_mem", f2], ["save", f2c, SMALL]], "reshard2")
    two = blob_of(f2)
    assert blob_of(f2b) == two and blob_of(f2c) == two
    parts = launch(name, n_global, 3, tmp, [["load", f2, SMALL], ["steps", k, k + SC.MORE], ["save", e3, 0]], "reshard3")
    assert_same_filter(blob_of(e3), e, "2 ranks' file on 3 ranks")
    assert_infos(parts, rec, "reshard3")
    for chunk in (0, SMALL):
        f = gpu_mod.GpuFilter(SC.config(name, n_global))
        f.load_state_at(f2, chunk_bytes=chunk)
        got = {}
        SC.advance(f, name, k, k + SC.MORE, got)
        assert_same_filter(f.save_state().tobytes(), e, "2 ranks' file on one GPU")
        assert_infos([got], rec, "reshard1")
        f.close()


class LoopComm:
    """a communicator of one rank, in process: every exchange is a copy"""
    rank, nranks, device_memory, error = 0, 1, False, None

    def __init__(self):
        self._ag = A.ALLGATHER_FN(lambda user, send, recv, n, stream: C.memmove(recv, send, n) and 0)
        self._a2a = A.ALLTOALLV_FN(lambda user, send, sb, recv, rb, stream: C.memmove(recv, send, int(sb[0])) and 0)
        self.struct = A.Comm(None, 0, 1, 0, 0, self._ag, self._a2a)


def save_at_bytes(f, size, chunk=0):
    """eslam_gpu_save_at into memory: the blob, and how often each byte was written"""
    blob, hits = np.zeros(size, np.uint8), np.zeros(size, np.uint8)

    def pwrite(_user, off, data, n):
        if off + n > size:
            return 1
        blob[off:off + n] = np.frombuffer(C.string_at(data, n), np.uint8)
        hits[off:off + n] += 1
        return 0

    info = A.SnapshotInfo()
    f._check(f.L.eslam_gpu_save_at(f.h, A.PWRITE_FN(pwrite), None, chunk, C.byref(info)))
    assert info.bytes == size
    return blob.tobytes(), hits


@pytest.mark.parametrize("name", ["maps", "hash"])
def test_one_context(gpu_mod, tmp_path, name):
    """in process: on an unsharded filter save_at writes save_stream's bytes, each once, and
    load_at restores them; the same on a filter sharded over one rank, which still refuses the
    sequential forms"""
    import io
    import eslam_dist
    n_global = 1536
    b = single(gpu_mod, name, n_global)[0]
    path = os.path.join(str(tmp_path), "B.snap")
    f = gpu_mod.GpuFilter(SC.config(name, n_global))
    f.load_state(b)
    out = io.BytesIO()
    f.save_state(file=out)
    assert out.getvalue() == b
    for chunk in (0, SMALL):
        got, hits = save_at_bytes(f, len(b), chunk)
        assert got == b and hits.min() == 1 and hits.max() == 1
    f.save_state_at(path)
    assert blob_of(path) == b
    f.close()
    f = gpu_mod.GpuFilter(SC.config(name, n_global))
    f.load_state_at(path, chunk_bytes=SMALL)
    assert f.save_state().tobytes() == b
    f.close()
    # sharded over one rank: every bit of both bitmaps is set, table k is pool entry k
    g = eslam_dist.ShardedGpuFilter(SC.config(name, n_global), n_global, LoopComm())
    g.load_state_at(path)
    assert g.snapshot_info().bytes == len(b)
    got, hits = save_at_bytes(g, len(b), SMALL)
    assert got == b and hits.min() == 1 and hits.max() == 1
    g.load_state(b)                              # eslam_gpu_load: the whole blob in memory
    assert save_at_bytes(g, len(b))[0] == b
    info = A.SnapshotInfo()
    buf = np.zeros(len(b), np.uint8)
    assert g.L.eslam_gpu_save(g.h, buf.ctypes.data_as(C.c_void_p), len(b), 0, C.byref(info)) == A.ERR_UNSUPPORTED
    assert "eslam_gpu_save_at" in g.L.eslam_gpu_last_error(g.h).decode()
    assert g.L.eslam_gpu_save_stream(g.h, A.WRITE_FN(lambda u, d, n: 0), None, 0, C.byref(info)) == A.ERR_UNSUPPORTED
    assert g.L.eslam_gpu_load_stream(g.h, A.READ_FN(lambda u, d, n: 1), None, 0, C.byref(info)) == A.ERR_UNSUPPORTED
    rec, want = {}, single(gpu_mod, name, n_global)
    k = SC.SAVE_AT[name]
    SC.advance(g, name, k, k + SC.MORE, rec)     # the refusals changed nothing
    assert save_at_bytes(g, len(want[1]))[0] == want[1]
    assert_infos([rec], want[2], "one rank")
    g.close()


def test_one_rank_device_memory_and_rccl(gpu_mod, tmp_path):
    """the host-word collectives' device-memory branch (the plan's counts and the agreements go
    through the context's small device buffer): one rank loads the one-GPU blob and saves it in
    4 KiB chunks, continues and saves again, with device-memory callbacks and over the library's
    own RCCL communicator.  Both write the host-memory run's bytes, and end where the one-GPU
    filter does.  The three one-rank groups run one after another: a worker that fails ends the
    test before the next one starts."""
    name, n_global = "maps", 1500
    b, e, rec = single(gpu_mod, name, n_global)
    tmp = str(tmp_path)
    fb = os.path.join(tmp, "B.snap")
    open(fb, "wb").write(b)
    k = SC.SAVE_AT[name]
    mems = ("host", "device", "rccl")
    files = {m: (os.path.join(tmp, f"S_{m}.snap"), os.path.join(tmp, f"E_{m}.snap")) for m in mems}

    def run(m):
        fs, fe = files[m]
        return launch(name, n_global, 1, tmp, [["load", fb, SMALL], ["save", fs, SMALL], ["steps", k, k + SC.MORE],
                                               ["save", fe, SMALL]], f"one_{m}", mem=m)

    parts = {m: run(m) for m in mems}            # launch() asserts every worker's exit status
    host_s, host_e = (blob_of(p) for p in files["host"])
    assert_same_filter(host_e, e, "host, one rank")
    for m in ("device", "rccl"):
        assert blob_of(files[m][0]) == host_s, f"{m}: the blob saved after the load"
        assert blob_of(files[m][1]) == host_e, f"{m}: the blob saved after three more steps"
        assert_same_filter(blob_of(files[m][1]), e, f"{m}, one rank")
        assert_infos(parts[m], rec, m)
        assert list(parts[m][0]["op1/save"][:2]) == [len(host_s), n_global]


def test_refusals_and_agreement(gpu_mod, tmp_path):
    """2 ranks: a blob of another particle count is refused before any collective; a callback
    failing on one rank and a page pool too small on one rank fail the call on both, and after a
    failed load neither rank holds particles.  Return codes on a healthy device throughout."""
    name, n_global = "maps", 1500
    tmp = str(tmp_path)
    good, other = os.path.join(tmp, "B.snap"), os.path.join(tmp, "other.snap")
    open(good, "wb").write(single(gpu_mod, name, n_global)[0])
    open(other, "wb").write(single(gpu_mod, name, 1536)[0])
    parts = launch(name, n_global, 2, tmp, [["refusals", good, other]], "refusals")
    for r, p in enumerate(parts):
        assert int(p["other_n"][0]) == A.ERR_INVALID_ARG, r
        assert int(p["bad_read_step"][0]) == A.ERR_NOT_INITIALISED and int(p["small_pool_step"][0]) == A.ERR_NOT_INITIALISED, r
        assert int(p["still_saves"][0]) == 0, r
    assert [int(p["bad_read"][0]) for p in parts] == [A.ERR_COMM, A.ERR_COMM]          # rank 1's callback; rank 0 told
    assert [int(p["bad_write"][0]) for p in parts] == [A.ERR_COMM, A.ERR_COMM]
    assert [int(p["small_pool"][0]) for p in parts] == [A.ERR_COMM, A.ERR_OUT_OF_MEMORY]

