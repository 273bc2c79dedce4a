"""What the sharded-snapshot tests drive (test infrastructure): a filter -- one GPU's, or one
rank's shard [lo, hi) -- is prepared, stepped to the point where it is saved (snapshot B), and
stepped three more times (snapshot E).  The ranks and the one-GPU filter run the same calls.

    hash      pose hash on (init from the hash, respawn every 2nd step): shared map only
    maps      per-particle maps; a scan merged after every step, the match weighting on odd steps
    heirloom  per-particle maps; one particle's wide map copied to every particle by a resample
              and saved at once: one table under every particle, so it straddles every boundary
"""
import eslam_abi as A
import synthetic as S
from dist_scenarios import _info, heirloom_arrays, scenario_config, scenario_grid

SAVE_AT = {"hash": 3, "maps": 3, "heirloom": 0}      # steps before snapshot B
MORE = 3                                             # steps between B and E


def config(name, n_global):
    return scenario_config(name, n_global)


def bounds(name, n_global, world):
    return A.shard_bounds(n_global, world, config(name, n_global).sum_chunk_rows)


def stream(name):
    if name == "hash":
        from hash_util import slope_stream
        return slope_stream(6)
    return S.step_stream(6, tilt=(name == "maps"))


def prepare(f, name, n_global, lo, hi):
    f.set_map(scenario_grid(name))
    if name == "hash":
        f.init_pose([0.0, 0.0, 0.18], [1.0, 0.0, 0.0, 0.0])
    elif name == "maps":
        f.init_gaussian(hi - lo, [0.0, 0.0, 0.0], [0.05, 0.05, 0.02], 0.18, 0.05)
    else:
        f.upload(heirloom_arrays(n_global, lo, hi))
        f.map_update(S.scan_patches(nx=16, ny=12, x0=-2.6, x1=4.6, y0=-2.5, y1=2.4))
        f.resample()


def advance(f, name, k0, k1, rec):
    """steps [k0, k1) of the scenario's stream; every step's eslam_update_info into rec"""
    scan = S.scan_patches() if name != "hash" else None
    probe = S.scan_patches(z=-0.15) if name != "hash" else None
    for k, st in list(enumerate(stream(name)))[k0:k1]:
        f.step(st)
        _info(rec, f"s{k}", f.sync())
        if scan is not None and k % 2 == 1:
            f.map_match(probe)
        if scan is not None:
            f.map_update(scan)
