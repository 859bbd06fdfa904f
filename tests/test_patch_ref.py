"""CPU: the numpy restatement of the patch pipeline (tests/patch_ref.py) against the reference's own output
(tests/golden/patch_*.npz, written by tests/golden/make_patch_golden.py), and hand-checkable known answers.

Selection, radius, pi and the index columns are exact.  Rotations and feature columns agree up to the per-patch
sign s of the middle axis within 512 eps / relgap_i absolute (patch_cases.tolerance).
"""
import numpy as np
import pytest

import patch_cases as C
import patch_ref as R


@pytest.fixture(scope="module", params=["ellipsoid", "shells"])
def case(request):
    g = C.load_golden(request.param)
    return g, R.network_input(g["v"], g["f"], np.arange(len(g["f"])), int(g["k"]))


def test_radius_selection_and_centre_index_are_exact(case):
    g, out = case
    assert np.array_equal(out["r"], g["r"])
    assert np.array_equal(out["centre"], g["centre"])
    assert np.array_equal(out["off"], g["off"]) and np.array_equal(out["faces"], g["faces"])
    assert np.array_equal(out["pi"], g["pi"])


def test_rotations_and_inputs_within_the_eigen_bound(case):
    g, out = case
    tol = C.tolerance(g["relgap"])
    assert np.all(np.abs(R.relgap(out["eig"]) - g["relgap"]) <= 1e-9)
    s = R.sign_align(out["rot"], g["rot"])
    keep = g["input_faces"]
    inputs, _ = R.apply_sign(g["inputs"], g["rot"][keep], s[keep])
    _, rot_all = R.apply_sign(np.zeros((len(s), 1, 20)), g["rot"], s)
    dev_rot = np.abs(out["rot"] - rot_all).max(axis=(1, 2))
    dev_in = np.abs(out["inputs"][keep][:, :, :17] - inputs[:, :, :17]).max(axis=(1, 2))
    print(f"max deviation x relgap / eps: rotations {np.max(dev_rot * g['relgap']) / C.EPS:.1f}, "
          f"inputs {np.max(dev_in * g['relgap'][keep]) / C.EPS:.1f} (bound 512)")
    assert np.all(dev_rot <= tol)
    assert np.all(dev_in <= tol[keep])
    assert np.array_equal(out["inputs"][keep][:, :, 17:], g["inputs"][:, :, 17:])


def test_fixture_covers_padding_truncation_and_both_signs():
    e, s = C.load_golden("ellipsoid"), C.load_golden("shells")
    size_e, size_s = np.diff(e["off"]), np.diff(s["off"])
    assert size_e.min() < R.ROWS < size_e.max() and size_s.min() > R.ROWS
    assert (e["pi"] >= R.ROWS).sum() == 30 and np.all(np.isin(np.nonzero(e["pi"] >= R.ROWS)[0], e["input_faces"]))
    assert e["margin"].min() >= 1e-8 and s["margin"].min() >= 1e-8
    assert e["relgap"].min() >= 1e-5 and s["relgap"].min() >= 1e-5
    f = s["f"]                                           # every shells patch holds faces of both components
    comp = (f[:, 0] >= len(s["v"]) // 2).astype(int)
    both = np.add.reduceat(comp[s["faces"]], s["off"][:-1])
    assert np.all((both > 0) & (both < size_s))


def test_octahedron_every_patch_is_the_whole_mesh():
    v, f = C.octahedron()
    out = R.network_input(v, f, np.arange(8))
    assert np.array_equal(np.diff(out["off"]), np.full(8, 8))
    assert np.array_equal(out["faces"].reshape(8, 8), np.tile(np.arange(8), (8, 1)))
    assert np.array_equal(out["pi"], np.arange(8))
    assert np.all(out["inputs"][:, :8, 7] == 3) and np.all(out["inputs"][:, 8:, :17] == 0)
    assert np.allclose(np.linalg.det(out["rot"]), 1.0)


def test_edge_adjacency_known_answers():
    assert np.array_equal(R.tta(C.strip()[1]), C.STRIP_TT)
    tt = R.tta(C.cube()[1])
    assert np.all(tt >= 0)
    for g in range(12):
        for e in range(3):
            assert g in tt[tt[g, e]]
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])      # the edge (0, 1) has three faces: no adjacency across it
    assert np.all(R.tta(f) == -1)


def test_index_columns_on_the_strip():
    v, f = C.strip()
    ref = R.network_input(v, f, np.arange(4), neighbours="reference")
    adj = R.network_input(v, f, np.arange(4), neighbours="adjacency")
    assert np.array_equal(np.diff(ref["off"]), np.full(4, 4))
    for p in range(4):
        assert np.array_equal(ref["inputs"][p, :4, 7], [1, 2, 2, 1])
        assert np.array_equal(ref["inputs"][p, :, 17:], np.array([[1] * 3, [63] * 3, [0] * 3] + [[63] * 3] * 61))
        assert np.array_equal(adj["inputs"][p, :, 17:], np.array([[1, 1, 1], [2, 0, 0], [1, 3, 3], [2, 2, 2]] + [[63] * 3] * 60))
