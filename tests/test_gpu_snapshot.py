"""Snapshots on the GPU (eslam_gpu_save / eslam_gpu_load): one filter (`orig`)
saves at step K, a freshly created second one (`rest`) loads, and both continue next to the
oracle, which needs no snapshot and simply keeps running.  "Bit-exact" means: the downloads bit
for bit, the map-update counters of every update, the ancestors, and the maps of sampled
particles (0 and n - 1 among them).  The saved filter, continued, equals the oracle too: a save
changes nothing a later call can see."""
import io

import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import shared_map_ref as R
import snapshot_format as F
import synthetic as S
from hash_util import hash_config, hash_grid, slope_stream
from parity_util import assert_bit_identical, info_tuple

pytestmark = pytest.mark.gpu

MAP_INFO = ("map_patches_dropped", "map_stores_copied", "map_stores_changed", "map_patches_covered", "map_tiles_evicted")


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def map_info(i):
    return tuple(int(getattr(i, f)) for f in MAP_INFO)


def assert_maps_equal(gpu, orc, idx, label):
    for i in idx:
        gc, gm, gs = gpu.particle_map(i)
        oc, om, os_ = orc.particle_map(i)
        go, oo = np.argsort(gc), np.argsort(oc)
        assert np.array_equal(gc[go], oc[oo]), (label, i)
        assert np.array_equal(u32(gm[go]), u32(om[oo])) and np.array_equal(u32(gs[go]), u32(os_[oo])), (label, i)


def sample(n, count=8):
    return sorted(set(np.linspace(0, n - 1, count).astype(np.int64).tolist() + [0, n - 1]))


def assert_same_grid(got, want, label):
    assert np.array_equal(got.cell_start, want.cell_start), label
    assert np.array_equal(u32(got.mean), u32(want.mean)) and np.array_equal(u32(got.stdev), u32(want.stdev)), label
    assert (got.patch_height is None) == (want.patch_height is None), label
    if want.patch_height is not None:
        assert np.array_equal(u32(got.patch_height), u32(want.patch_height)), label


def updated(filters, orc, scan, label, maps=None, ancestors=True):
    """after a step + map update on every filter: each GPU filter bit-exact with the oracle"""
    oi, op = map_info(orc.info()), orc.download()
    for name, f in filters:
        assert map_info(f.sync()) == oi, (label, name, oi)
        assert_bit_identical(f.download(), op, f"{label} {name}")
        if ancestors:
            assert np.array_equal(f.ancestors(), orc.ancestors()), (label, name)
        if maps:
            assert_maps_equal(f, orc, maps, f"{label} {name}")


def pm_config(n, trail=None, pages=None):
    cfg = S.bench_config(A.default_config(), n)
    cfg.flags |= A.FLAG_PARTICLE_MAPS | A.FLAG_RECORD_ANCESTORS
    if trail is not None:
        cfg.local_map_trail = trail
    if pages is not None:
        cfg.local_map_pages = pages
    return cfg


def pm_pair(gpu_mod, cfg, grid, n, sigma=(0.05, 0.05, 0.02), zs=0.05, threads=1):
    gpu = gpu_mod.GpuFilter(cfg)
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    orc.set_threads(threads)
    for f in (gpu, orc):
        f.set_map(grid)
        f.init_gaussian(n, [0.0, 0.0, 0.0], list(sigma), 0.18, zs)
    return gpu, orc


def run_to_save(gpu_mod, n, steps=12):
    """the per-particle-map scenario of tests 1-3 and 8 up to the save: `steps` steps, a map update
    after each but the last; the last step's resample gather is still pending (no sync, no download)"""
    cfg = pm_config(n)
    grid = S.unmapped_beyond(S.rough_map(cells=80), 0.3)
    orig, orc = pm_pair(gpu_mod, cfg, grid, n)
    scan = S.scan_patches()
    stream = S.step_stream(24, tilt=True)
    for k in range(steps):
        assert orig.step(stream[k]) == orc.step(stream[k])
        if k < steps - 1:
            orig.map_update(scan)
            orc.map_update(scan)
    return cfg, orig, orc, scan, stream


def continue_from(orig, rest, orc, scan, stream, first, last, label):
    """the map update of step `first`, then steps first + 1 .. last, on all three"""
    n = orig.count()
    both = [("orig", orig), ("rest", rest)]
    for f in (orig, rest, orc):
        f.map_update(scan)
    updated(both, orc, scan, f"{label} step {first}", ancestors=False)     # a load carries no ancestors
    for k in range(first + 1, last + 1):
        st = stream[k - 1]
        assert orig.step(st) == rest.step(st) == orc.step(st)
        for f in (orig, rest, orc):
            f.map_update(scan)
        updated(both, orc, scan, f"{label} step {k}", maps=sample(n) if k % 6 == 0 or k == last else None)


def test_continue_particle_maps(gpu_mod, oracle):
    """1 + 2: save after step 12 with the gather pending; orig, rest and the oracle bit-exact for
    steps 13-24; canonical bytes (a save right after the load returns the loaded blob; after step 24
    orig and rest, whose pools differ, save the same bytes); the Python reader of the documented
    layout agrees with download() and particle_map()"""
    n = 2048
    cfg, orig, orc, scan, stream = run_to_save(gpu_mod, n)
    blob = orig.save_state()
    info = orig.last_snapshot
    assert info.bytes == blob.shape[0] and info.particles == n and info.version == A.SNAPSHOT_VERSION
    assert info.sections == A.SNAPSHOT_GRID | A.SNAPSHOT_PARTICLES | A.SNAPSHOT_SCALARS | A.SNAPSHOT_MAPS
    assert 0 < info.tables < n and info.pages > 0            # resamples have happened: tables are shared
    # the reader: the particles and 40 particles' maps, in eslam_gpu_get_particle_map's order
    snap = F.read(blob)
    assert snap.header["tables"] == info.tables and snap.header["pages"] == info.pages
    p = orig.download()
    for f in F.PARTICLE_FIELDS + ("floating", "n_contact_points"):
        assert np.array_equal(np.ascontiguousarray(snap.particles[f]).view(np.uint8), np.ascontiguousarray(getattr(p, f)).view(np.uint8)), f
    for i in sample(n, 40):
        for got, want in zip(snap.particle_map(i), orig.particle_map(i)):
            assert np.array_equal(u32(got), u32(want)), i
    rest = gpu_mod.GpuFilter(cfg)
    linfo = rest.load_state(blob)
    assert (linfo.bytes, linfo.tables, linfo.pages) == (info.bytes, info.tables, info.pages)
    assert np.array_equal(rest.save_state(), blob)
    continue_from(orig, rest, orc, scan, stream, 12, 24, "continue")
    a, b = orig.save_state(), rest.save_state()
    assert orig.last_snapshot.tables <= n
    assert np.array_equal(a, b)
    rest.close()
    orig.close()


def test_chunking(gpu_mod, oracle):
    """3: any chunk size gives the same bytes in another number of chunks; a load in 4 KiB chunks
    continues bit-exact; the file-object forms carry the same bytes"""
    n = 600
    cfg, orig, orc, scan, stream = run_to_save(gpu_mod, n)
    blobs, chunks = [], []
    for cb in (4096, 65536, 0):
        blobs.append(orig.save_state(chunk_bytes=cb))
        chunks.append(orig.last_snapshot.chunks)
    assert np.array_equal(blobs[0], blobs[1]) and np.array_equal(blobs[0], blobs[2])
    assert chunks[0] > chunks[1] > chunks[2] > 0, chunks
    buf = io.BytesIO()
    finfo = orig.save_state(chunk_bytes=8192, file=buf)
    assert buf.getvalue() == blobs[0].tobytes() and finfo.bytes == blobs[0].shape[0]
    rest = gpu_mod.GpuFilter(cfg)
    rest.load_state(file=io.BytesIO(buf.getvalue()), chunk_bytes=65536)
    assert np.array_equal(rest.save_state(), blobs[0])
    rest.load_state(blobs[0], chunk_bytes=4096)              # replaces what the filter holds
    continue_from(orig, rest, orc, scan, stream, 12, 18, "chunked load")
    rest.close()
    orig.close()


# test_particle_maps_loop_trail's walk, shortened: straight out, then back, on the empty prior.
# TRAIL_OUT / TRAIL_BACK are the shortest out-and-back for which the CPU oracle alone shows a
# 3-entry trail forgetting a tile on the way out (map_tiles_evicted first rises at step 203) and a
# tile of particle 0's trail inside its window again on the way back (the window's centre returns
# one tile at step 203 + 34); found by running the oracle over longer walks, checked again below.
TRAIL_OUT, TRAIL_BACK = 203, 40


def test_trail_and_eviction(gpu_mod, oracle):
    """4a: a save at the turn-around of an out-and-back walk with a 3-entry trail: trails, their
    high-water marks and the evictions continue bit-exact"""
    n = 1024
    cfg = pm_config(n, trail=3, pages=32)
    grid = S.unmapped_beyond(S.flat_map(cells=200), -1e9)
    orig, orc = pm_pair(gpu_mod, cfg, grid, n, threads=16)
    scan = S.scan_patches()
    stream = S.step_stream(TRAIL_OUT, dx=0.02, dyaw=0.0) + S.step_stream(TRAIL_BACK, dx=-0.02, dyaw=0.0)
    half = 4                                                 # dm_lm_half(3.0 m, 0.1 m cells): a 9 x 9-tile window

    def tiles(i):
        c = orc.particle_map(i)[0].astype(np.int64)
        return set(zip(((c % grid.width) // 8).tolist(), ((c // grid.width) // 8).tolist()))

    def outside(i):
        p = orc.download()
        ca = int(np.floor((p.x[i] - grid.offset[0]) / grid.scale[0])) >> 3
        cb = int(np.floor((p.y[i] - grid.offset[1]) / grid.scale[1])) >> 3
        return {t for t in tiles(i) if abs(t[0] - ca) > half or abs(t[1] - cb) > half}

    evicted = 0
    rest = None
    for k, st in enumerate(stream):
        fs = [("orig", orig)] + ([("rest", rest)] if rest else [])
        assert len({f.step(st) for _, f in fs} | {orc.step(st)}) == 1
        for f in [f for _, f in fs] + [orc]:
            f.map_update(scan)
        last = k == len(stream) - 1
        updated(fs, orc, scan, f"trail step {k}", maps=sample(n, 4) if last or k == TRAIL_OUT else None)
        if k < TRAIL_OUT:
            evicted += orc.info().map_tiles_evicted
        if k == TRAIL_OUT - 1:                               # the turn-around
            assert evicted > 0
            trail0 = outside(0)
            assert trail0
            rest = gpu_mod.GpuFilter(cfg)
            rest.load_state(orig.save_state())
            assert_maps_equal(rest, orc, sample(n, 4), "trail after load")
    assert trail0 & (tiles(0) - outside(0))                  # a tile came back from the trail
    assert np.array_equal(orig.save_state(), rest.save_state())
    rest.close()
    orig.close()


def test_shadow_tables(gpu_mod, oracle):
    """4b: scan patches on cells the shared grid covers (tables holding copies of grid cells,
    kLmShadow): saved after 6 updates, bit-exact for 6 more"""
    n = 1500
    cfg = pm_config(n, pages=48)
    grid = S.unmapped_beyond(S.rough_map(cells=120), 0.3)
    orig, orc = pm_pair(gpu_mod, cfg, grid, n, sigma=(0.1, 0.1, 0.05))
    scan = S.scan_patches(nx=10, ny=6, x0=-0.9, x1=0.95)
    rest, covered = None, 0
    for k, st in enumerate(S.step_stream(12, tilt=True)):
        fs = [("orig", orig)] + ([("rest", rest)] if rest else [])
        assert len({f.step(st) for _, f in fs} | {orc.step(st)}) == 1
        for f in [f for _, f in fs] + [orc]:
            f.map_update(scan)
        updated(fs, orc, scan, f"shadow step {k}", maps=sample(n) if k in (5, 11) else None)
        covered += orc.info().map_patches_covered
        if k == 5:
            assert covered > 0
            blob = orig.save_state()
            assert F.read(blob).tables[:, 2].max() == 1      # shadow tables are in the snapshot
            rest = gpu_mod.GpuFilter(cfg)
            rest.load_state(blob)
    assert np.array_equal(orig.save_state(), rest.save_state())
    rest.close()
    orig.close()


def test_restored_pool(gpu_mod, oracle):
    """5: a pool of 10 pages per particle saved at step 30: the collection runs on the restored
    pool (10 pages) and on a larger one (16) alike, bit-exact to step 60; a pool of 1 page per
    particle refuses the blob with ESLAM_ERR_OUT_OF_MEMORY and is usable afterwards"""
    n = 8192
    cfg = pm_config(n, pages=10)
    grid = S.unmapped_beyond(S.rough_map(cells=200), -1e9)
    orig, orc = pm_pair(gpu_mod, cfg, grid, n, sigma=(0.1, 0.1, 0.1), zs=1.001, threads=16)
    scan = S.scan_patches()
    stream = S.step_stream(60, tilt=True)
    rest, blob, want = None, None, []
    for k, st in enumerate(stream):
        fs = [("orig", orig)] + ([("rest10", rest)] if rest else [])
        assert len({f.step(st) for _, f in fs} | {orc.step(st)}) == 1
        for f in [f for _, f in fs] + [orc]:
            f.map_update(scan)
        updated(fs, orc, scan, f"pool step {k}", maps=sample(n, 4) if k == 59 else None)
        if k >= 30:
            want.append((map_info(orc.info()), orc.download(), orc.ancestors()))
        if k == 29:
            blob = orig.save_state()
            assert orig.last_snapshot.pages > n              # more live pages than a pool of 1 per particle holds
            rest = gpu_mod.GpuFilter(cfg)
            rest.load_state(blob)
    rest.close()
    cfg16 = pm_config(n, pages=16)
    r16 = gpu_mod.GpuFilter(cfg16)
    r16.load_state(blob)
    for k in range(30, 60):
        r16.step(stream[k])
        r16.map_update(scan)
        wi, wp, wa = want[k - 30]
        assert map_info(r16.sync()) == wi, k
        assert_bit_identical(r16.download(), wp, f"pool of 16, step {k}")
        assert np.array_equal(r16.ancestors(), wa), k
    assert_maps_equal(r16, orc, sample(n, 4), "pool of 16")
    r16.close()
    small = gpu_mod.GpuFilter(pm_config(n, pages=1))
    with pytest.raises(gpu_mod.EslamError) as ei:
        small.load_state(blob)
    assert ei.value.code == A.ERR_OUT_OF_MEMORY and "local_map_pages" in str(ei.value)
    assert small.count() == 0
    small.set_map(grid)
    small.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1], 0.18, 1.001)
    small.step(stream[0])
    small.sync()
    small.close()
    orig.close()


def heights_grid(cells=120):
    grid = S.rough_map(cells=cells)
    rng = np.random.default_rng(3)
    grid.patch_height = np.where(rng.random(grid.mean.shape[0]) < 0.3, rng.uniform(0.05, 0.5, grid.mean.shape[0]), 0.0).astype(np.float32)
    return grid


def test_shared_map_filter(gpu_mod, oracle):
    """6: a shared-map filter after a shared_map_update: the grid as the device holds it travels
    (heights included), and steps and a further merge continue identically"""
    n = 512
    cfg = S.bench_config(A.default_config(), n)
    cfg.flags |= A.FLAG_RECORD_ANCESTORS
    grid = heights_grid()
    orig = gpu_mod.GpuFilter(cfg)
    orig.set_map(grid)
    orig.init_gaussian(n, [0.0, 0.0, 0.0], [0.1, 0.1, 0.05], 0.18, 0.05)
    scan = S.scan_patches()
    assert len(scan) == 48
    stream = S.step_stream(20, tilt=True)
    for k in range(10):
        orig.step(stream[k])
        if k == 4:
            merge = orig.shared_map_update(scan)
            assert merge.inserted + merge.fused > 0
            assert not np.array_equal(u32(orig.get_map().mean), u32(grid.mean))      # the grid has been merged into
    blob = orig.save_state()
    assert orig.last_snapshot.sections == A.SNAPSHOT_GRID | A.SNAPSHOT_PARTICLES | A.SNAPSHOT_SCALARS
    assert orig.last_snapshot.grid_patches == orig.get_map().mean.shape[0] >= grid.mean.shape[0]
    rest = gpu_mod.GpuFilter(cfg)
    rest.load_state(blob)
    assert_same_grid(rest.get_map(), orig.get_map(), "after the load")
    got = rest.get_map()
    assert (got.width, got.height, got.scale, got.offset, got.g2l) == (grid.width, grid.height, grid.scale, grid.offset, grid.g2l)
    for k in range(10, 20):
        assert orig.step(stream[k]) == rest.step(stream[k])
        assert_bit_identical(rest.download(), orig.download(), f"shared step {k}")
        assert np.array_equal(rest.ancestors(), orig.ancestors()), k
        if k == 14:
            a, b = orig.shared_map_update(scan), rest.shared_map_update(scan)
            assert all(getattr(a, f) == getattr(b, f) for f, _ in A.SharedMergeInfo._fields_)
            assert_same_grid(rest.get_map(), orig.get_map(), "after the second merge")
    assert np.array_equal(orig.save_state(), rest.save_state())
    rest.close()
    orig.close()


def test_pose_hash(gpu_mod, oracle):
    """7: the pose hash built once in init travels as it is: a shared merge at step 3 has changed
    the grid since, so a hash rebuilt at load would hold other poses (checked on the CPU oracle);
    steps 16-35 cross two respawns (the respawn counter and rand())"""
    n = 2048
    cfg = hash_config(n, steps=8, bins=20, period=10)
    grid = hash_grid(cells=60)
    orig = gpu_mod.GpuFilter(cfg)
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    for f in (orig, orc):
        f.set_map(grid)
        f.init_pose([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])
    scan = S.scan_patches()
    stream = slope_stream(35)
    for k in range(15):
        orig.step(stream[k])
        if k < 3:
            orc.step(stream[k])
        if k == 2:                                           # after step 3
            assert_bit_identical(orig.download(), orc.download(), "before the merge")
            merged, _ = R.merge(grid, orc.download(), scan)
            orig.shared_map_update(scan)
            assert_same_grid(orig.get_map(), merged, "merge")
            rebuilt = O.OracleFilter(cfg, O.SUM_CONTRACT)
            rebuilt.set_map(merged)
            rebuilt.hash_create()
            before, after = orc.hash_poses(), rebuilt.hash_poses()
            assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(before, after))
    blob = orig.save_state()
    assert orig.last_snapshot.sections & A.SNAPSHOT_HASH and orig.last_snapshot.hash_poses == orig.hash_info()[0] > 0
    rest = gpu_mod.GpuFilter(cfg)
    rest.load_state(blob)
    (no, so), (nr, sr) = orig.hash_info(), rest.hash_info()
    assert no == nr and np.array_equal(so, sr)
    for a, b in zip(orig.hash_poses(), rest.hash_poses()):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    for a, b in zip(orig.hash_poses(), orc.hash_poses()):    # still the hash of the grid before the merge
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    h0 = orig.rng_state().hash_count
    resamples = 0
    for k in range(15, 35):
        assert orig.step(stream[k]) == rest.step(stream[k])
        assert_bit_identical(rest.download(), orig.download(), f"hash step {k}")
        oi, ri = orig.sync(), rest.sync()
        assert info_tuple(oi) == info_tuple(ri), k
        if oi.resampled:                                     # the ancestors are the last resample's; a load carries none
            resamples += 1
            assert np.array_equal(rest.ancestors(), orig.ancestors()), k
    assert resamples > 0
    so, sr = orig.rng_state(), rest.rng_state()
    assert so.hash_count == sr.hash_count == h0 + 20 and so.libc_rand_pos == sr.libc_rand_pos
    assert list(so.libc_rand) == list(sr.libc_rand) and so.minstd_x == sr.minstd_x
    rest.close()
    orig.close()


def test_refusals(gpu_mod, oracle):
    """8: blobs that fail validation are refused on the host with ESLAM_ERR_INVALID_ARG and a
    message, the context reads as "no particles" and stays usable; a failing write callback ends the
    save with ESLAM_ERR_COMM and the saved filter steps on, bit-exact with the oracle"""
    n = 600
    cfg, orig, orc, scan, stream = run_to_save(gpu_mod, n)
    good = orig.save_state()
    snap = F.read(good)
    maps_off = snap.sections["maps"][0]
    tables_off = maps_off + F.pad16(4 * n)

    def patched(off, value, dtype="<u4"):
        b = good.copy()
        b[off:off + np.dtype(dtype).itemsize] = np.frombuffer(np.array([value], dtype).tobytes(), np.uint8)
        return b

    cases = {
        "truncated by one byte": good[:-1],
        "truncated to the header": good[:F.HEADER_BYTES],
        "bad magic": patched(0, good[0] ^ 1, "u1"),
        "version 2": patched(8, 2),
        "local_map_trail": patched(36, cfg.local_map_trail + 1),
        "PARTICLE_MAPS": patched(32, 0),
        "a sid past the tables": patched(maps_off + 4 * 5, snap.header["tables"]),
        "a slot past the pages": patched(tables_off + 4 * 4, snap.header["pages"]),
        "a section past the end": patched(248 + 16 * 4 + 8, snap.sections["maps"][1] + 16, "<u8"),
    }
    victim = gpu_mod.GpuFilter(cfg)
    for k, (label, blob) in enumerate(cases.items()):
        if k % 3 == 0:
            victim.load_state(good)                          # a live context is replaced, then refuses
        with pytest.raises(gpu_mod.EslamError) as ei:
            victim.load_state(blob)
        assert ei.value.code == A.ERR_INVALID_ARG and str(ei.value), label
        assert victim.count() == 0, label
        with pytest.raises(gpu_mod.EslamError) as ei:
            victim.step(stream[0])
        assert ei.value.code == A.ERR_NOT_INITIALISED, label
    # a context with another layout refuses the good blob
    other = pm_config(n)
    other.max_sensor_range = 1.0
    victim.close()
    victim = gpu_mod.GpuFilter(other)
    with pytest.raises(gpu_mod.EslamError) as ei:
        victim.load_state(good)
    assert ei.value.code == A.ERR_INVALID_ARG and "max_sensor_range" in str(ei.value)
    victim.close()

    class Failing:
        calls = 0

        def write(self, b):
            self.calls += 1
            if self.calls == 2:
                raise IOError("disk full")

    sink = Failing()
    with pytest.raises(gpu_mod.EslamError) as ei:
        orig.save_state(chunk_bytes=4096, file=sink)
    assert ei.value.code == A.ERR_COMM and sink.calls == 2
    victim = gpu_mod.GpuFilter(cfg)
    victim.load_state(good)
    continue_from(orig, victim, orc, scan, stream, 12, 15, "after the refusals")
    victim.close()
    orig.close()
