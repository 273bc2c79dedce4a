"""One gloo rank of tests/test_gpu_kld.py's sharded test: eslam_gpu_kld_count and
eslam_gpu_resample_kld on a filter sharded over 2 or 3 ranks that share one GPU.

    RANK=r WORLD_SIZE=w ESLAM_DIST_STORE=file python tests/kld_dist_worker.py OUT.npz

Filter A (every kind of skipped particle among its particles) is only counted.  First the calls
every rank refuses before any collective (bad arguments): rank 1 and up ask first and rank 0 after
a barrier, so a call that entered a collective would hang.  Then the ranks ask together with
different theta_bins: the parameter all_gather is the call's first collective, every rank sees the
mismatch, and the counts that follow show that no rank is a collective behind.  Then COUNTS.
Filter B runs OPS, counts and count-then-resample calls in sequence; after each a rank saves the
info, its shard, the table and the minstd state.  Filter C holds one bin: the count it asks for has
fewer summation chunks than ranks, which the sharded resample refuses on every rank.  Filter D has
per-particle maps: resample_kld is refused before any collective (the barrier again).
run_ops() is the code the test runs on ONE unsharded context for the expected values.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "slam-eslam_amd"))

import numpy as np  # noqa: E402

N = 1050                                              # 17 chunks of 64: 8 + 9, or 5 + 6 + 6
BAD = [dict(bin_xy=0.0), dict(theta_bins=0), dict(theta_bins=4097), dict(epsilon=float("nan")), dict(n_min=0),
       dict(n_min=5, n_max=4), dict(min_change=-1.0), dict(z_quantile=-0.5), dict(multinomial=2)]
COUNTS = [dict(n_min=1), dict(n_min=1, theta_bins=1), dict(n_min=1, theta_bins=4096, bin_xy=0.05), dict(n_min=1, bin_xy=0.08),
          dict(n_min=20000, n_max=30000), dict(n_min=1, min_change=50.0)]
# (call, params): the first grows the filter, the third shrinks it by a multinomial draw
OPS = [("resample", dict(n_min=1)), ("count", dict(n_min=1)), ("resample", dict(n_min=1, bin_xy=0.5, theta_bins=8, multinomial=1)),
       ("count", dict(n_min=1, theta_bins=12)), ("normalize", {}), ("resample", dict(n_min=1, min_change=1e9)),
       ("resample", dict(n_min=1, bin_xy=0.3, theta_bins=6))]


def particles(x, y, th, w):
    import eslam_abi as A
    pa = A.ParticleArrays(x.shape[0])
    pa.x[:], pa.y[:], pa.orientation[:], pa.weight[:] = x, y, th, w
    pa.zpos[:], pa.zsigma[:] = 0.18, 0.01
    return pa


def cloud_a():
    import kld_cases as K
    return K.with_skipped(*K.cloud(N, seed=N), seed=5)[:4]


def cloud_b():
    """resampled: finite everywhere, some zero weights (skipped), normalised"""
    import kld_cases as K
    x, y, th, w = K.cloud(N, seed=77)
    w[::7] = 0.0
    return x, y, th, w / w.sum()


def info_words(info):
    """every field of a KldInfo as 64-bit words (the bound as its bits)"""
    flat = sum([list(t) if isinstance(t, tuple) else [t] for t in info.as_tuple()], [])
    return np.array([int(v) & (2 ** 64 - 1) for v in flat], dtype=np.uint64)


def snap(rec, key, f):
    import eslam_abi as A
    pa = f.download()
    for fld in A.ParticleArrays.FIELDS:
        rec[f"{key}/{fld}"] = np.array(getattr(pa, fld))
    rec[f"{key}/rng"] = np.array([f.rng_state().minstd_x], dtype=np.uint64)


def run_ops(rec, f):
    """OPS on filter f (sharded or not), everything saved under ops/<i>"""
    for i, (what, params) in enumerate(OPS):
        key = f"ops/{i}"
        if what == "count":
            rec[f"{key}/info"] = info_words(f.kld_count(**params))
        elif what == "normalize":
            # the multinomial draw left weights of 1 / n_before that sum below 1.  The held resample
            # that follows is the filter's own resample(), whose info.overruns a sharded filter and
            # one context report differently when draws overrun (eslam_gpu_resample_stratified_sharded
            # at the own count: 0 against 712 here).  Normalised, no draw overruns on either
            f.normalize()
        else:
            info, rinfo = f.resample_kld(**params)
            rec[f"{key}/info"] = info_words(info)
            rec[f"{key}/rinfo"] = np.array([rinfo.n_before, rinfo.n_after, rinfo.overruns, rinfo.dropped], dtype=np.uint64)
        snap(rec, key, f)


def main():
    out = sys.argv[1]
    import torch.distributed as dist
    import eslam_abi as A
    import eslam_amd
    import eslam_dist
    import kld_cases as K
    import synthetic as S
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", init_method="file://" + os.environ["ESLAM_DIST_STORE"], rank=rank, world_size=world)
    comm = eslam_dist.TorchComm(device_memory=False)

    def sharded(arrs, flags=0, with_map=False):
        cfg = A.default_config()
        cfg.flags |= flags
        f = eslam_dist.ShardedGpuFilter(cfg, N, comm, device=0)
        if with_map:
            f.set_map(S.flat_map(cells=100))
        lo, hi = f.bounds[rank], f.bounds[rank + 1]
        f.upload(particles(*[a[lo:hi] for a in arrs]))
        return f

    def code_of(call, staggered):
        if staggered and rank == 0:
            dist.barrier()
        try:
            call()
            code = 0
        except eslam_amd.EslamError as e:
            code = e.code
        if staggered and rank != 0:
            dist.barrier()
        return code

    rec = {}
    # A: counted only
    f = sharded(cloud_a())
    codes = [code_of(lambda: f.kld_count(**kw), True) for kw in BAD]
    codes += [code_of(lambda: f.resample_kld(**kw), True) for kw in BAD[:2]]
    codes.append(code_of(lambda: f.kld_count(n_min=1, theta_bins=36 + rank), False))
    codes.append(code_of(lambda: f.resample_kld(n_min=1, epsilon=0.05 + 0.01 * rank), False))
    rec["a/codes"] = np.array(codes)
    for i, params in enumerate(COUNTS):
        rec[f"a/info{i}"] = info_words(f.kld_count(**params))
    # at 2.5 m cells the particles at |x| = 2.2e8 are counted: a box of 1.76e8 cells
    rec["a/spread"] = np.array([code_of(lambda: f.kld_count(n_min=1, bin_xy=2.5), False), code_of(lambda: f.kld_count(n_min=1, max_bins=64), False)])
    snap(rec, "a", f)
    f.close()
    # B: counts and resamples in sequence
    f = sharded(cloud_b())
    run_ops(rec, f)
    rec["b/bounds"] = np.array(f.bounds, dtype=np.uint64)
    assert f.bounds == f.get_shard_bounds() and f.n_global == f.bounds[-1]
    assert (f.gbase, f.n_local) == (f.bounds[rank], f.bounds[rank + 1] - f.bounds[rank]) and f.count() == f.n_local
    f.close()
    # C: one bin asks for one particle, fewer chunks than ranks
    f = sharded(K.one_bin(N))
    rec["c/code"] = np.array([code_of(lambda: f.resample_kld(n_min=1), False)])
    rec["c/count"] = np.array([f.count(), f.n_global], dtype=np.uint64)
    snap(rec, "c", f)
    f.close()
    # D: per-particle maps keep their count
    f = sharded(cloud_b(), flags=A.FLAG_PARTICLE_MAPS, with_map=True)
    rec["d/code"] = np.array([code_of(lambda: f.resample_kld(n_min=1), True), code_of(lambda: f.resample_kld(n_min=N, n_max=N + 1), True)])
    rec["d/info"] = info_words(f.kld_count(n_min=1))
    info, rinfo = f.resample_kld(n_min=N, n_max=N)        # the count is fixed: the sharded eslam_gpu_resample
    rec["d/fixed"] = np.array([info.samples, info.clamped, rinfo.n_before, rinfo.n_after, f.count()], dtype=np.uint64)
    f.close()
    if comm.error is not None:
        raise comm.error
    np.savez(out, **rec)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
