"""Every map path on grids that are square in neither sense (tests/rect_grids.py: 150 x 110
cells, scale_x != scale_y, one cell size per parity class of the window's half widths), bit for
bit against the oracle.  A table row's two bookkeeping words (the shadow flag and the trail's
high-water mark) sit behind its (2 hx + 1)(2 hy + 1) window slots; on the windows whose hx and hy
differ in parity (9 x 11, 11 x 9, 9 x 15 tiles) padding the slots alone left one word for the
two, and the flag landed on the window's last slot.  The per-axis rules themselves are pinned on
the CPU (tests/test_rect_grids.py)."""
import math

import numpy as np
import pytest

import eslam_abi as A
import oracle_ffi as O
import particle_grid_ref as PG
import rect_grids as G
import snapshot_format as F
import synthetic as S
from parity_util import assert_bit_identical, run_pair

pytestmark = pytest.mark.gpu

MAP_INFO = ("map_patches_dropped", "map_stores_copied", "map_stores_changed", "map_patches_covered", "map_tiles_evicted")
SCALE = G.RECT_CASES["9x11"][0]               # 0.10 x 0.08 m cells: a 9 x 11-tile window, W = 99


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


def sample(n, count=12):
    return sorted(set(np.linspace(0, n - 1, count).astype(np.int64).tolist() + [0, 1, n - 1]))


def maps_config(n, pages=48, trail=None):
    cfg = S.bench_config(A.default_config(), n)
    cfg.flags |= A.FLAG_PARTICLE_MAPS | A.FLAG_RECORD_ANCESTORS
    cfg.local_map_pages = pages
    if trail is not None:
        cfg.local_map_trail = trail
    return cfg


def pair(gpu_mod, cfg, grid, n, sigma=(0.1, 0.1, 0.05), zs=0.05, threads=4):
    gpu = gpu_mod.GpuFilter(cfg)
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    orc.set_threads(threads)
    for f in (gpu, orc):
        f.set_map(grid)
        f.init_gaussian(n, [0.0, 0.0, 0.0], list(sigma), 0.18, zs)
    return gpu, orc


def mapped_cells_scan():
    """reaching back over the cells the shared grid covers (x < 0.3): the shadow flag"""
    return S.scan_patches(nx=10, ny=6, x0=-0.9, x1=0.95)


# ---- a. steps without maps --------------------------------------------------------------------
@pytest.mark.parametrize("yaw", [None, 0.3])
def test_step_parity(gpu_mod, oracle, yaw):
    """K1's staged window and K3 on the 150 x 110 grid of 0.10 x 0.08 m cells, identity and rotated
    global2local: particles and info after every step, the ancestors of every resample"""
    n = 1500
    grid = G.rect_rough_map(scale=SCALE)
    if yaw is not None:
        grid = G.rotated(grid, yaw=yaw)
    cfg = S.bench_config(A.default_config(), n)
    gpu, orc = run_pair(cfg, grid, S.step_stream(10, tilt=True), n, gpu_factory=lambda c: gpu_mod.GpuFilter(c),
                        label=f"rect steps yaw={yaw}")
    assert orc.info().data_particles > 0
    gpu.close()


def test_particles_leaving_the_short_edge(gpu_mod, oracle):
    """the cloud walks off the grid's short side (y = +-4.4 m; the long side reaches +-7.5 m): feet
    that pass the height but would still be inside a square grid of the width must miss"""
    n = 1500
    grid = G.rect_rough_map(scale=SCALE)
    assert grid.height * grid.scale[1] < grid.width * grid.scale[0]
    cfg = S.bench_config(A.default_config(), n)
    stream = S.step_stream(12, dx=0.12, dyaw=0.0, tilt=True)
    gpu, orc = run_pair(cfg, grid, stream, n, init=dict(mu=[0.0, 3.6, math.pi / 2], sigma=[0.4, 0.4, 0.1], z=0.18, zs=0.5),
                        gpu_factory=lambda c: gpu_mod.GpuFilter(c), label="short edge")
    p = orc.download()
    half = grid.height * grid.scale[1] / 2
    assert np.mean(p.y > half) > 0.3 and np.all(np.abs(p.x) < grid.width * grid.scale[0] / 2 - 1.0)
    assert 0 < orc.info().data_particles < n
    gpu.close()


# ---- b. per-particle maps on every window shape ----------------------------------------------
SHAPES = [(name, scan, yaw) for name in G.RECT_CASES for scan in ("forward", "mapped_cells") for yaw in (None,)]
SHAPES += [(name, scan, 0.7) for name in ("9x11", "11x9") for scan in ("forward", "mapped_cells")]


@pytest.mark.parametrize("name,scan_kind,yaw", SHAPES)
def test_particle_maps_shapes(gpu_mod, oracle, name, scan_kind, yaw):
    """test_gpu_particle_maps.py's test_particle_maps_shapes on every row of rect_grids.RECT_CASES:
    the default forward scan and the scan reaching back over mapped cells (tables that carry the
    shadow flag); the two windows with one padding word also on a grid rotated by 0.7 rad, where
    both window axes move as the robot walks in +x"""
    scale, (hx, hy) = G.RECT_CASES[name]
    n = 1500
    cfg = maps_config(n)
    grid = G.rect_prior("beyond", scale, yaw=yaw)
    gpu, orc = pair(gpu_mod, cfg, grid, n)
    scan = S.scan_patches() if scan_kind == "forward" else mapped_cells_scan()
    dropped = written = covered = 0
    for k, st in enumerate(S.step_stream(12, tilt=True)):
        assert gpu.step(st) == orc.step(st)
        gpu.map_update(scan)
        orc.map_update(scan)
        gi = gpu.sync()
        assert_bit_identical(gpu.download(), orc.download(), f"{name} {scan_kind} yaw={yaw} step {k}")
        assert map_info(gi) == map_info(orc.info()), (name, scan_kind, k, map_info(gi), map_info(orc.info()))
        dropped += gi.map_patches_dropped
        written += gi.map_cells_written
        covered += gi.map_patches_covered
    assert np.array_equal(gpu.ancestors(), orc.ancestors())
    assert_maps_equal(gpu, orc, list(range(0, n, 97)) + [n - 1], name)
    assert written > 0 and dropped == 0
    if scan_kind == "mapped_cells":
        assert covered > 0
    gpu.close()


# ---- c. the trail on a window with one padding word ---------------------------------------------
TRAIL_YAW, TRAIL_DX = 0.7, 0.05
TRAIL_OUT, TRAIL_BACK = 48, 44


def trail_scan():
    """reaching back and sideways to the window's edges (every patch within 3 m): the tiles the
    window leaves behind hold pages, so they go to the trail"""
    return S.scan_patches(nx=12, ny=8, x0=-2.6, x1=0.95, y0=-1.4, y1=1.4)


def trail_walk():
    return S.step_stream(TRAIL_OUT, dx=TRAIL_DX, dyaw=0.0) + S.step_stream(TRAIL_BACK, dx=-TRAIL_DX, dyaw=0.0)


def check_trail_walk_geometry():
    """each leg moves the window's centre by more than two tile columns and two tile rows of the
    rotated grid: a tile is 8 cells, 0.8 m x 0.64 m"""
    assert all(math.hypot(s.position[0], s.position[1]) < G.RANGE for s in trail_scan())
    for steps in (TRAIL_OUT, TRAIL_BACK):
        assert steps * TRAIL_DX * math.cos(TRAIL_YAW) > 2 * 8 * SCALE[0]
        assert steps * TRAIL_DX * math.sin(TRAIL_YAW) > 2 * 8 * SCALE[1]


@pytest.mark.parametrize("trail", [16, 2])
def test_trail_on_a_one_padding_word_window(gpu_mod, oracle, trail):
    """an empty prior on the rotated 9 x 11 window, out 2.4 m and 2.2 m back with a scan that maps
    the window's rear: tiles go to the trail on the way out and come back on the return.
    Counters on every step, particles and sampled maps at the turn and at the end; a trail of 2
    overflows.  On the way back the feet find the cells mapped on the way out."""
    check_trail_walk_geometry()
    n = 1024
    cfg = maps_config(n, pages=160, trail=trail)
    grid = G.rect_prior("empty", SCALE, yaw=TRAIL_YAW)
    gpu, orc = pair(gpu_mod, cfg, grid, n, sigma=(0.05, 0.05, 0.02))
    scan = trail_scan()
    stream = trail_walk()
    evicted, moved, out, back = 0, 0, [], []
    for k, st in enumerate(stream):
        assert gpu.step(st) == orc.step(st)
        gpu.map_update(scan)
        orc.map_update(scan)
        gi, oi = gpu.sync(), orc.info()
        assert map_info(gi) == map_info(oi), (k, map_info(gi), map_info(oi))
        assert gi.data_particles == oi.data_particles
        evicted += oi.map_tiles_evicted
        (out if k < TRAIL_OUT else back).append(oi.data_particles / n)
        if k in (TRAIL_OUT - 1, len(stream) - 1):
            assert_bit_identical(gpu.download(), orc.download(), f"trail {trail} step {k}")
            assert_maps_equal(gpu, orc, sample(n, 6), f"trail {trail} step {k}")
            moved += sum(outside_window(orc, grid, i) for i in sample(n, 6))
    assert np.array_equal(gpu.ancestors(), orc.ancestors())
    assert moved > 0                                   # sampled maps hold tiles outside their window: trail entries
    if trail == 16:
        assert evicted == 0
    else:
        assert evicted > 0
    # over ground mapped on the way out more particles find data than over unmapped ground
    assert np.mean(back) > np.mean(out), (np.mean(out), np.mean(back))
    gpu.close()


def outside_window(f, grid, i):
    """the tiles of particle i's map outside the window around its pose: its trail's tiles (the
    window's centre is the tile at the last map update, which the pose has not left since)"""
    hx, hy = half_widths(grid)
    c = f.particle_map(i)[0].astype(np.int64)
    p = f.download()
    lx, ly = G.to_local(grid, p.x[i], p.y[i], p.zpos[i])
    m, n = G.cell_coords(grid, lx, ly)
    ca, cb = int(math.floor(m)) >> 3, int(math.floor(n)) >> 3
    ta, tb = (c % grid.width) >> 3, (c // grid.width) >> 3
    return len(set(zip(ta[(np.abs(ta - ca) > hx) | (np.abs(tb - cb) > hy)].tolist(),
                       tb[(np.abs(ta - ca) > hx) | (np.abs(tb - cb) > hy)].tolist())))


def half_widths(grid):
    return tuple(min(max(math.ceil(G.RANGE / (8.0 * s)), 1), 15) for s in grid.scale)


# ---- d. map_match -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["identity", "mapped_cells"])
def test_map_match(gpu_mod, oracle, case):
    """test_particle_maps_match_bit_exact's identity and mapped_cells cases on the 9 x 11 window:
    the match weighting against the particle's own map and against the shared grid's cells"""
    n = 2000
    cfg = maps_config(n)
    grid = G.rect_prior("beyond", SCALE)
    gpu, orc = pair(gpu_mod, cfg, grid, n)
    back = dict(x0=-0.9, x1=0.95) if case == "mapped_cells" else {}
    scan = S.scan_patches(nx=12, ny=9, **back)
    probe = S.scan_patches(nx=12, ny=9, z=-0.15, **back)
    lowered = 0
    for k, st in enumerate(S.step_stream(12, tilt=True)):
        assert gpu.step(st) == orc.step(st)
        w0 = gpu.download().weight.copy()
        if k % 4 != 2:
            gpu.map_match(probe)
            orc.map_match(probe)
            assert_bit_identical(gpu.download(), orc.download(), f"{case} match step {k}")
            lowered += int(np.sum(gpu.download().weight < w0))
        if k % 4 != 1:
            gpu.map_update(scan)
            orc.map_update(scan)
            assert map_info(gpu.sync()) == map_info(orc.info()), (case, k)
        assert_bit_identical(gpu.download(), orc.download(), f"{case} step {k}")
    assert np.array_equal(gpu.ancestors(), orc.ancestors())
    assert lowered > n
    gpu.close()


# ---- e. the page collection with the bookkeeping words in play -----------------------------------
COLLECT_STEPS, COLLECT_DX = 40, 0.1
COLLECT_PAGES = 17


def collect_run(filters, orc, n, steps=COLLECT_STEPS, on_step=None, before_update=None):
    """the 9 x 11 window, the scan over mapped cells (shadow tables) and a walk of 4 m, which moves
    the tiles mapped at the start out of the window and into the trail"""
    scan = mapped_cells_scan()
    for k, st in enumerate(S.step_stream(steps, dx=COLLECT_DX, dyaw=0.0, tilt=True)):
        assert len({f.step(st) for f in filters} | {orc.step(st)}) == 1
        if before_update:
            before_update(k)
        for f in filters + [orc]:
            f.map_update(scan)
        for f in filters:
            gi = f.sync()
            assert map_info(gi) == map_info(orc.info()), (k, map_info(gi), map_info(orc.info()))
        if on_step:
            on_step(k)


def test_page_collection(gpu_mod, oracle):
    """A pool of COLLECT_PAGES pages per particle: twice what the oracle's maps hold per particle
    at the end of this run (8.36 pages per particle: or_pages_in_use / n after step 40, measured on
    the CPU, 10.3 at its peak after step 5; the assertion below keeps the figure honest).  The
    collection runs several times --
    it marks the pages of the window's slots and of the trail's used entries, and must take
    neither bookkeeping word for a page id -- and 40 steps stay bit-exact.

    The marks' invariant, through the public info alone: eslam_gpu_snapshot_size reports `pages`,
    the distinct pages the particles' tables name.  Asked between a step and its map update, that
    is the set a collection inside the update marks (no tile is forgotten here: the trail never
    overflows), so after an update that collected, the pages in use are exactly those plus the
    pages the update took: n * local_map_pages - map_pages_free == pages + map_pages_taken.  A
    walk that takes a bookkeeping word for a page id marks a page no table names."""
    n = 1500
    cfg = maps_config(n, pages=COLLECT_PAGES, trail=16)
    grid = G.rect_prior("beyond", SCALE)
    gpu, orc = pair(gpu_mod, cfg, grid, n)
    free, live, collections, covered = [n * COLLECT_PAGES], [0], [0], [0]

    def before(k):
        live[0] = int(gpu.snapshot_info().pages)

    def each(k):
        gi = gpu.sync()
        assert gi.map_tiles_evicted == 0
        if gi.map_pages_free + gi.map_pages_taken > free[-1]:                # the free list was rebuilt
            collections[0] += 1
            print("collection at step", k, "live", live[0], "taken", gi.map_pages_taken, "free", gi.map_pages_free)
            assert n * COLLECT_PAGES - gi.map_pages_free == live[0] + gi.map_pages_taken, k
        free.append(int(gi.map_pages_free))
        covered[0] += gi.map_patches_covered
        if k % 10 == 9:
            assert_bit_identical(gpu.download(), orc.download(), f"collection step {k}")

    collect_run([gpu], orc, n, on_step=each, before_update=before)
    assert np.array_equal(gpu.ancestors(), orc.ancestors())
    assert_maps_equal(gpu, orc, sample(n), "collection")
    assert collections[0] >= 3 and covered[0] > 0, (collections, free)
    assert sum(outside_window(orc, grid, i) for i in sample(n)) > 0        # trail entries in use
    per = orc.pages_in_use() / n
    assert COLLECT_PAGES / 2.5 < per <= COLLECT_PAGES / 2, per
    gpu.close()


def test_loaded_pool_holds_the_live_pages_only(gpu_mod, oracle):
    """The page walks' invariant, through the public info alone: a snapshot reports `pages`, the
    distinct pages live tables name.  A fresh context that loads it holds exactly those, so after
    one map update n * local_map_pages - map_pages_free == pages + map_pages_taken.  A walk that
    took a bookkeeping word for a page id would count one page more or fewer."""
    n = 1500
    cfg = maps_config(n, pages=COLLECT_PAGES, trail=16)
    grid = G.rect_prior("beyond", SCALE)
    gpu, orc = pair(gpu_mod, cfg, grid, n)
    collect_run([gpu], orc, n, steps=34)
    blob = gpu.save_state()
    pages = gpu.last_snapshot.pages
    rest = gpu_mod.GpuFilter(cfg)
    rest.load_state(blob)
    st = S.step_stream(35, dx=COLLECT_DX, dyaw=0.0, tilt=True)[34]
    scan = mapped_cells_scan()
    for f in (gpu, rest, orc):
        f.step(st)
        f.map_update(scan)
    ri = rest.sync()
    assert map_info(ri) == map_info(orc.info())
    assert n * COLLECT_PAGES - ri.map_pages_free == pages + ri.map_pages_taken
    assert_bit_identical(rest.download(), orc.download(), "loaded pool")
    assert_bit_identical(gpu.download(), orc.download(), "saved pool")
    rest.close()
    gpu.close()


# ---- f. whole-map export and adoption ----------------------------------------------------------
@pytest.mark.parametrize("name", ["9x11", "9x17"])
def test_particle_grid_and_adoption(gpu_mod, oracle, name):
    """eslam_gpu_get_particle_grid against the numpy model applied to the device's own getters and
    to the oracle's maps; adopting particle i's map equals exporting it and setting it, and both
    twins continue alike"""
    scale, _ = G.RECT_CASES[name]
    n = 1000
    cfg = maps_config(n)
    grid = G.rect_prior("beyond", scale)
    a, orc = pair(gpu_mod, cfg, grid, n)
    assert PG.grids_equal(a.particle_grid(0), grid)
    scan = mapped_cells_scan()
    stream = S.step_stream(18, tilt=True)
    for st in stream[:12]:
        assert a.step(st) == orc.step(st)
        a.map_update(scan)
        orc.map_update(scan)
    assert_bit_identical(a.download(), orc.download(), f"{name}: the mapping run")
    own = 0
    for i in sample(n, 5):
        got, pm = a.particle_grid(i), a.particle_map(i)
        assert PG.grids_equal(got, PG.compose(pm, grid)), (name, i, "the device's own getters")
        assert PG.grids_equal(got, PG.compose(orc.particle_map(i), grid)), (name, i, "the oracle's map")
        assert got.scale == grid.scale and got.offset == grid.offset and (got.width, got.height) == (grid.width, grid.height)
        own += len(pm[0])
    assert own > 0
    b = gpu_mod.GpuFilter(cfg)
    b.load_state(a.save_state())
    i = a.best_index()
    exported = b.particle_grid(i)
    a.adopt_particle_map(i)
    b.set_map(exported)
    assert PG.grids_equal(a.get_map(), exported) and PG.grids_equal(b.get_map(), exported)
    assert int(exported.cell_start[-1]) > int(grid.cell_start[-1])
    for st in stream[12:18]:
        assert a.step(st) == b.step(st)
        a.map_update(scan)
        b.map_update(scan)
        assert map_info(a.sync()) == map_info(b.sync())
    assert_bit_identical(a.download(), b.download(), f"{name}: adopt vs export + set_map")
    for k in sample(n, 4):
        assert PG.grids_equal(a.particle_grid(k), b.particle_grid(k)), k
    for f in (a, b):
        f.close()


# ---- h. snapshot ------------------------------------------------------------------------------
def test_snapshot_with_shadow_flag_and_trail(gpu_mod, oracle):
    """The state of test_page_collection after 34 steps (shadow tables, trail entries in use, the
    9 x 11 window), saved and loaded into a fresh context: both continue for 6 steps bit-identical
    to the oracle and to each other.  The blob, read by the Python reader of the documented layout,
    holds the oracle's state: its particles, its maps (trail tiles included), and the shadow flag
    (row word 2) on every table whose map holds a cell the shared grid covers."""
    n = 1500
    cfg = maps_config(n, pages=COLLECT_PAGES, trail=16)
    grid = G.rect_prior("beyond", SCALE)
    orig, orc = pair(gpu_mod, cfg, grid, n)
    collect_run([orig], orc, n, steps=34)
    blob = orig.save_state()
    snap = F.read(blob)
    h = snap.header
    assert (h["wx"], h["wy"], h["hx"], h["hy"]) == (9, 11, 4, 5) and h["row_words"] == F.row_words(99, 16)
    p = orc.download()
    for f in F.PARTICLE_FIELDS + ("floating", "n_contact_points"):
        assert np.array_equal(np.ascontiguousarray(snap.particles[f]).view(np.uint8),
                              np.ascontiguousarray(getattr(p, f)).view(np.uint8)), f
    covered_cell = np.diff(grid.cell_start.astype(np.int64)) > 0
    flagged = trails = 0
    for i in sample(n, 40):
        sc, sm, ss = snap.particle_map(i)
        oc, om, os_ = orc.particle_map(i)
        so, oo = np.argsort(sc), np.argsort(oc)
        assert np.array_equal(sc[so], oc[oo]), i
        assert np.array_equal(u32(sm[so]), u32(om[oo])) and np.array_equal(u32(ss[so]), u32(os_[oo])), i
        t = snap.table(int(snap.sid[i]))
        assert t["shadow"] in (0, 1)
        if covered_cell[oc.astype(np.int64)].any():          # the map holds a copy of a covered cell
            assert t["shadow"] == 1, i
            flagged += 1
        trails += sum(1 for _, _, pg in t["trail"] if pg != F.NONE)
    assert flagged > 0 and trails > 0
    rest = gpu_mod.GpuFilter(cfg)
    linfo = rest.load_state(blob)
    assert (linfo.tables, linfo.pages) == (h["tables"], h["pages"])
    assert np.array_equal(rest.save_state(), blob)           # canonical bytes
    scan = mapped_cells_scan()
    for k, st in enumerate(S.step_stream(40, dx=COLLECT_DX, dyaw=0.0, tilt=True)[34:]):
        assert orig.step(st) == rest.step(st) == orc.step(st)
        for f in (orig, rest, orc):
            f.map_update(scan)
        oi, op = map_info(orc.info()), orc.download()
        for label, f in (("orig", orig), ("rest", rest)):
            assert map_info(f.sync()) == oi, (k, label)
            assert_bit_identical(f.download(), op, f"snapshot {label} step {34 + k}")
            assert np.array_equal(f.ancestors(), orc.ancestors()), (k, label)
    for label, f in (("orig", orig), ("rest", rest)):
        assert_maps_equal(f, orc, sample(n), f"snapshot {label}")
    assert np.array_equal(orig.save_state(), rest.save_state())
    rest.close()
    orig.close()


# ---- i. SurfaceHash -----------------------------------------------------------------------------
@pytest.mark.parametrize("yaw", [None, 0.3])
def test_hash_create(gpu_mod, oracle, yaw):
    """SurfaceHash::create's sweep over a 70 x 50 grid of 0.10 x 0.08 m cells"""
    from hash_util import hash_config
    grid = G.rect_rough_map(70, 50, SCALE, seed=11)
    if yaw is not None:
        grid = G.rotated(grid, yaw=yaw, tx=0.7, ty=-0.4)
    cfg = hash_config(1000, steps=8, bins=20)
    orc = O.OracleFilter(cfg, O.SUM_CONTRACT)
    gpu = gpu_mod.GpuFilter(cfg)
    for f in (orc, gpu):
        f.set_map(grid)
        f.hash_create()
    no, so = orc.hash_info()
    ng, sg = gpu.hash_info()
    assert no == ng > 0 and np.array_equal(so, sg)
    for a, b in zip(gpu.hash_poses(), orc.hash_poses()):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    gpu.close()
