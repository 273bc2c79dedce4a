"""The trajectory log's numpy restatement (tests/trajectory_ref.py) on hand-made cases: what the GPU
tests compare the device log with must itself say what DESIGN.md 5j says."""
import ctypes as C

import numpy as np

import moments_ref
import trajectory_ref as T


def cols(n, step):
    """five columns that name their particle and step: x = 100 step + i, the others offsets of it"""
    x = 100.0 * step + np.arange(n, dtype=np.float64)
    return x, x + 0.25, x + 0.5, 0.001 * x, 1.0 + 0.0 * x


def test_identity_without_resamples():
    log = T.TrajectoryLog(8, 5)
    for s in range(3):
        log.record(*cols(5, s))
    tr = log.trace([0, 4, 4])
    assert tr.shape == (3, 3)
    assert np.array_equal(tr["slot"], [[0, 0, 0], [4, 4, 4], [4, 4, 4]])
    assert np.array_equal(tr["step"][0], [0, 1, 2]) and np.all(tr["particles"] == 5)
    assert np.array_equal(tr["x"][1], [4.0, 104.0, 204.0]) and np.array_equal(tr["zsigma"][1], [1.0, 1.0, 1.0])
    for e in log.entries:
        assert np.array_equal(e["parent"], np.arange(5))


def test_one_resample_in_a_step():
    log = T.TrajectoryLog(8, 4)
    log.record(*cols(4, 0))
    log.record(*cols(4, 1), anc=[0, 0, 2, 3])
    assert np.array_equal(log.entries[1]["parent"], [0, 0, 2, 3])
    assert np.array_equal(log.link, np.arange(4))
    tr = log.trace([1])
    assert np.array_equal(tr["slot"][0], [0, 1]) and np.array_equal(tr["x"][0], [0.0, 101.0])


def test_two_resamples_between_records_compose():
    log = T.TrajectoryLog(8, 4)
    log.record(*cols(4, 0))
    log.compose([3, 3, 1, 0])                    # link = [3, 3, 1, 0]
    log.compose([2, 2, 0, 1])                    # link' = link[anc] = [1, 1, 3, 3]
    assert np.array_equal(log.link, [1, 1, 3, 3])
    log.record(*cols(4, 1))                      # no resample in the step itself
    assert np.array_equal(log.entries[1]["parent"], [1, 1, 3, 3])
    log.compose([1, 0, 0, 0])
    log.record(*cols(4, 2), anc=[3, 2, 1, 0])    # ... and one with: parent = link[anc]
    assert np.array_equal(log.entries[2]["parent"], [0, 0, 0, 1])


def test_count_change_between_records():
    log = T.TrajectoryLog(8, 6)
    log.record(*cols(6, 0))
    log.compose([0, 2, 5])                       # down to 3 particles
    assert len(log.link) == 3
    log.record(*cols(3, 1))
    log.compose([2, 2, 1, 0, 0])                 # up to 5
    log.record(*cols(5, 2))
    assert [len(e["parent"]) for e in log.entries] == [6, 3, 5]
    assert np.array_equal(log.entries[1]["parent"], [0, 2, 5]) and np.array_equal(log.entries[2]["parent"], [2, 2, 1, 0, 0])
    tr = log.trace([0, 4])
    assert np.array_equal(tr["slot"], [[5, 2, 0], [0, 0, 4]])
    assert np.array_equal(tr["particles"][0], [6, 3, 5])
    assert np.array_equal(tr["x"][0], [5.0, 102.0, 200.0])


def test_ring_wrap_keeps_the_newest():
    log = T.TrajectoryLog(4, 3)
    for s in range(7):
        log.record(*cols(3, s), anc=[0, 0, 1] if s % 2 else None)
    assert [e["step"] for e in log.entries] == [3, 4, 5, 6]
    tr = log.trace([2])
    assert tr.shape == (1, 4) and np.array_equal(tr["step"][0], [3, 4, 5, 6])
    # the oldest held entry's own parent is never followed
    assert np.array_equal(tr["slot"][0], [1, 1, 2, 2])
    two = log.trace([2], capacity=2)
    assert np.array_equal(two["step"][0], [5, 6]) and np.array_equal(two["slot"][0], [2, 2])
    assert log.trace([2], capacity=0).shape == (1, 0)


def test_coalescence_to_one_ancestor():
    n = 8
    log = T.TrajectoryLog(8, n)
    log.record(*cols(n, 0))
    log.record(*cols(n, 1), anc=[0, 0, 0, 0, 4, 4, 4, 4])
    log.record(*cols(n, 2), anc=[4, 4, 4, 4, 5, 5, 6, 7])
    log.record(*cols(n, 3))
    w = np.full(n, 1.0 / n)
    sm = log.smoothed(w)
    assert [s[0] for s in sm] == [0, 1, 2, 3]
    assert [s[1] for s in sm] == [1, 4, 8, 8]
    maps, _ = log.ancestor_maps()
    assert np.array_equal(maps[0], [4] * n) and np.array_equal(maps[1], [4, 4, 4, 4, 5, 5, 6, 7])
    # one common ancestor: the mean is its pose and the position's covariance vanishes
    m0 = sm[0][2]
    assert m0.particles_counted == n and list(m0.mean[:3]) == [4.0, 4.25, 4.5]
    assert all(m0.cov[4 * r + c] == 0.0 for r in range(3) for c in range(3))
    # the newest entry's estimate is the plain moments of the entry's particles
    x, y, z, yaw, zs = cols(n, 3)
    rc, want = moments_ref.moments(x, y, z, yaw, zs, w)
    assert rc == 0 and bytes(sm[3][2]) == bytes(want)


def test_clear_starts_over():
    log = T.TrajectoryLog(4, 3)
    log.record(*cols(3, 0))
    log.compose([2, 1, 0])
    log.clear(5)
    assert log.entries == [] and np.array_equal(log.link, np.arange(5))
    assert log.trace([0, 4]).shape == (2, 0) and log.smoothed(np.ones(5)) == []
    log.record(*cols(5, 1))
    assert log.entries[0]["step"] == 1           # step ids count the records since enable


def test_node_layout_is_the_abi_struct():
    import eslam_abi as A
    assert T.NODE.itemsize == C.sizeof(A.TrajectoryPose)
    for f, _ in A.TrajectoryPose._fields_:
        assert T.NODE.fields[f][1] == getattr(A.TrajectoryPose, f).offset
