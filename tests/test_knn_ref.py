"""The brute-force search references (tests/knn_ref.py) checked on the CPU: the float32 restatement is admissible under
the float64 judge on every case, it orders exact integer distances like lexsort, and the radius reference is scipy's
query_ball_point."""
import numpy as np
import pytest

import knn_ref as R

try:
    from scipy.spatial import cKDTree
except ImportError:                                         # the oracle needs scipy; this file can do without
    cKDTree = None

KS = (1, 4, 13, 32, 64)


@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_are_finite_float32_and_small(name):
    snap, q = R.CASES[name]()
    assert snap.dtype == np.float32 and q.dtype == np.float32
    assert snap.shape[1] == 3 and q.shape[1] == 3 and 1 <= len(snap) <= 5000
    assert np.isfinite(snap).all() and np.isfinite(q).all()
    assert (q[:len(snap)] == snap).all()                     # the queries are the snapshot itself, then the extras
    snap2, q2 = R.CASES[name]()
    assert (snap2 == snap).all() and (q2 == q).all()         # seeded


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_is_admissible(name):
    snap, q = R.CASES[name]()
    tie = np.arange(len(snap))
    sorted64 = R.sorted_d2_f64(q, snap, max(KS))
    for k in KS:
        k = min(k, len(snap))
        idx, d2 = R.knn_f32(q, snap, k, tie)
        assert (np.diff(d2, axis=1) >= 0).all()
        ok = R.admissible_f64(q, snap, idx, sorted64)
        assert ok.all(), (name, k, int((~ok).sum()), np.nonzero(~ok)[0][:5])


def test_admissible_rejects_a_wrong_neighbour():
    snap, q = R.CASES["uniform_cube"]()
    idx, d2 = R.knn_f32(q, snap, 9, np.arange(len(snap)))
    bad = idx[:, :8].copy()
    bad[5, 7] = idx[5, 8]                                   # the 9th neighbour in place of the 8th
    ok = R.admissible_f64(q, snap, bad)
    assert not ok[5] and ok[np.arange(len(ok)) != 5].all()
    dup = idx[:, :8].copy()
    dup[6, 3] = dup[6, 2]
    assert not R.admissible_f64(q, snap, dup)[6]
    oob = idx[:, :8].copy()
    oob[7, 0] = len(snap)
    assert not R.admissible_f64(q, snap, oob)[7]


def test_lattice_order_is_lexsort_of_exact_distances():
    snap, q = R.CASES["lattice_ties"]()
    n = len(snap)
    qi, si = q.astype(np.int64), snap.astype(np.int64)
    dd = ((qi[:, None] - si[None]) ** 2).sum(-1)            # exact integers, all below 2^24: exact in float32 too
    index = np.arange(n)
    for k in (7, 64):
        idx, d2 = R.knn_f32(q, snap, k, index)
        for r in range(len(q)):
            assert (idx[r] == np.lexsort((index, dd[r]))[:k]).all(), r
        assert (d2 == np.take_along_axis(dd, idx, 1)).all()
    # another tie order: by a permutation's rank
    rank = np.random.default_rng(0).permutation(n)
    idx, _ = R.knn_f32(q, snap, 20, rank)
    for r in range(0, len(q), 7):
        assert (idx[r] == np.lexsort((rank, dd[r]))[:20]).all(), r


def test_exclude_self_drops_the_row_or_the_last():
    snap, q = R.CASES["lattice_ties"]()
    n = len(snap)
    index = np.arange(n)
    full, _ = R.knn_f32(snap, snap, 4, index)
    idx, _ = R.knn_f32(snap, snap, 3, index, exclude_self=True)
    for r in range(n):
        assert list(idx[r]) == [j for j in full[r] if j != r][:3]
    # 300 copies of one point: row 299 is not among its own 4 best (0, 1, 2, 3) and loses the last of them
    snap, _ = R.CASES["point"]()
    idx, _ = R.knn_f32(snap, snap, 3, np.arange(300), exclude_self=True)
    assert list(idx[299]) == [0, 1, 2] and list(idx[1]) == [0, 2, 3]


@pytest.mark.parametrize("name", ["uniform_cube", "translated"])
def test_radius_is_query_ball_point(name):
    snap, q = R.CASES[name]()
    rng = np.random.default_rng(3)
    radii = rng.uniform(0.0, 0.2, len(q)).astype(np.float32)
    radii[::50] = 0.0
    if cKDTree is None:                                     # plain double loop on a 200-point subset
        snap, q, radii = snap[:200], q[:200], radii[:200]
        want = []
        for i in range(len(q)):
            d = q[i].astype(np.float64) - snap.astype(np.float64)
            want.append([j for j in range(len(snap))
                         if (d[j, 0] * d[j, 0] + d[j, 1] * d[j, 1]) + d[j, 2] * d[j, 2] <= float(radii[i]) ** 2])
    else:
        want = cKDTree(snap.astype(np.float64)).query_ball_point(q.astype(np.float64), radii.astype(np.float64),
                                                                 return_sorted=True)
    slices, members = R.radius_f64(q, snap, radii)
    assert slices[0] == 0 and slices[-1] == len(members)
    for i in range(len(q)):
        assert list(members[slices[i]:slices[i + 1]]) == list(want[i]), i


def test_radius_special_values():
    snap, q = R.CASES["sheet"]()
    q = q[:6]
    radii = np.array([-1.0, np.nan, np.inf, 0.0, -0.0, 1e-30], np.float32)
    slices, members = R.radius_f64(q, snap, radii)
    assert list(np.diff(slices)) == [0, 0, len(snap), 1, 1, 1]
    assert (members[:len(snap)] == np.arange(len(snap))).all() and list(members[len(snap):]) == [3, 4, 5]
