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


# ------------------------------------------------------------------------------------------------ edge fixtures
# What tests/test_gpu_patch_edges.py relies on: every fixture reaches the branch it is there for.
def _patch_means(v, f, want):
    return np.array([v[np.unique(f[want["faces"][a:b]])].mean(axis=0) for a, b in zip(want["off"][:-1], want["off"][1:])])


@pytest.mark.parametrize("name", list(C.BOXES))
def test_boxes_equal_the_reference_on_the_allclose_branches(name):
    g = C.load_align(name)
    v, f, fis, out = C.edge_case("box/" + name)
    assert np.array_equal(g["v"], v) and np.array_equal(g["f"], f) and np.array_equal(g["input_faces"], np.arange(12))
    assert np.array_equal(np.diff(g["off"]), np.full(12, 12))            # every patch is the whole mesh
    # the branch the reference took, and the restatement's conditions for it
    _, translated, scaled = C.BOXES[name]
    assert np.all(g["translated"] == translated) and np.all(g["scaled"] == scaled)
    centre = v.mean(axis=0)
    size = np.linalg.norm(v - centre, axis=1).max()
    assert bool(np.allclose(np.linalg.norm(centre), 0)) != translated and bool(np.allclose(size, 1)) != scaled
    assert g["margin"].min() >= 1e-8 and abs(g["relgap"].min() - 0.053) < 1e-3 and not np.isnan(g["inputs"]).any()
    # the restatement against the reference, under the rule of the other goldens
    for key in ("r", "centre", "off", "faces", "pi"):
        assert np.array_equal(out[key], g[key]), key
    assert np.all(np.abs(R.relgap(out["eig"]) - g["relgap"]) <= 1e-9)
    dev_rot, dev_in = R.deviations(out["inputs"], out["rot"], g["inputs"], g["rot"],
                                   R.kept_centres(v, f, g["off"], g["faces"]))
    print(f"box {name}: max deviation x relgap / eps: rotations {np.max(dev_rot * g['relgap']) / C.EPS:.1f}, "
          f"inputs {np.max(dev_in * g['relgap']) / C.EPS:.1f} (bound 512)")
    assert np.all(dev_rot <= C.tolerance(g["relgap"])) and np.all(dev_in <= C.tolerance(g["relgap"]))
    assert np.array_equal(out["inputs"][:, :, 17:], g["inputs"][:, :, 17:])
    corners = g["inputs"][:, :12, 8:17].reshape(12, 36, 3)
    if name == "centred":
        assert np.array_equal(centre, np.zeros(3))
    if name == "near_origin":                            # resized and rotated about c, which the rows keep
        assert 0 < np.linalg.norm(centre) <= 1e-8
        assert np.abs((corners.max(axis=1) + corners.min(axis=1)) / 2 - centre).max() <= 1e-15
    if name == "unit_size":
        assert abs(np.linalg.norm(corners, axis=2).max() - 1.000005) <= 1e-9
    if name == "above_unit_size":
        assert abs(size - 1.00002) <= 1e-9 and abs(np.linalg.norm(corners, axis=2).max() - 1) <= 1e-12


def test_tiny_ellipsoid_is_never_translated_and_selects_as_the_unscaled_mesh():
    g = C.load_golden("ellipsoid")
    v, f, fis, out = C.edge_case("tiny_ellipsoid")
    assert np.linalg.norm(_patch_means(v, f, out), axis=1).max() < 1e-8
    assert np.array_equal(out["off"], np.concatenate([[0], np.cumsum(np.diff(g["off"])[fis])]))
    assert np.array_equal(out["faces"], np.concatenate([g["faces"][g["off"][i]:g["off"][i + 1]] for i in fis]))
    assert np.array_equal(out["pi"], g["pi"][fis]) and np.array_equal(out["r"], g["r"][fis] * 2.0 ** -27)
    assert 2.2e-4 <= R.relgap(out["eig"]).min() < 2.3e-4 and np.isfinite(out["inputs"]).all()


@pytest.mark.parametrize("order", ["last", "first"])
def test_needle_patch_does_not_hold_its_own_face(order):
    v, f, fis, out = C.edge_case("needle_" + order)
    nd = C.needle(order)[2]
    assert np.array_equal(np.diff(out["off"]), np.full(9, 8))
    assert np.array_equal(np.nonzero(out["pi"] < 0)[0], [nd]) and not np.isin(nd, out["faces"])
    assert abs(out["r"][nd] - 28.28) < 5e-3 and np.linalg.norm(v[f[nd]] - out["centre"][nd], axis=1).min() >= 33.3
    gap = R.relgap(out["eig"])
    assert 0.118 <= gap.min() < 0.119 and 0.137 < gap.max() <= 0.138 and np.isfinite(out["inputs"]).all()


def test_needle_far_has_an_empty_patch_between_others():
    v, f, fis, out = C.edge_case("needle_far")
    assert np.array_equal(np.diff(out["off"]), [8, 8, 8, 8, 0, 8, 8, 8, 8])
    assert np.array_equal(out["pi"], [0, 1, 2, 3, -1, 4, 5, 6, 7]) and not np.isin(4, out["faces"])
    assert np.array_equal(out["rot"][4], np.eye(3)) and np.all(out["inputs"][4, :, :17] == 0)
    assert np.all(out["inputs"][4, :, 17:] == 63)
    assert np.nanmin(np.delete(R.relgap(out["eig"]), 4)) >= 0.118


def test_offset_grids_lose_their_extent_in_float32():
    distinct = {key: len(np.unique(C.offset_grid(*arg)[0].astype(np.float32), axis=0)) for key, arg in C.OFFSET_GRIDS.items()}
    assert distinct["1e3"] == 81 and distinct["collapsed"] < 81 // 2
    assert len(np.unique(C.offset_grid(0.01, 1e5)[0].astype(np.float32), axis=0)) == 81      # (does not collapse them)
    for key in C.OFFSET_GRIDS:
        v, f, fis, out = C.edge_case("offset_grid/" + key)
        assert len(np.unique(v, axis=0)) == 81 and np.diff(out["off"]).min() >= 8 and np.all(out["pi"] >= 0)


def test_degenerate_face_lies_in_other_patches_and_its_own_is_empty():
    v, f, fis, out = C.edge_case("ellipsoid_degenerate")
    g = C.load_golden("ellipsoid")
    assert len(f) == 321 and R.areas(v, f, [320])[0] == 0.0
    assert not np.isin(f[320], f[:320]).any() and np.all(R.tta(f)[320] == -1)
    local = [np.nonzero(out["faces"][a:b] == 320)[0] for a, b in zip(out["off"][:-1], out["off"][1:])]
    holds = np.array([len(x) > 0 for x in local])
    assert holds.sum() == 51 and sum(int(x[0]) < R.ROWS for x in local if len(x)) == 9
    assert out["r"][320] == 0.0 and out["off"][321] == out["off"][320] and out["pi"][320] == -1
    assert (out["pi"] < 0).sum() == 1 and (out["pi"] >= R.ROWS).sum() == 30
    assert np.isfinite(out["rot"]).all() and R.relgap(out["eig"])[:320].min() >= 1e-5
    # the patches without it are the plain ellipsoid's, and without a degenerate face the option changes no bit
    sizes = np.diff(g["off"])
    assert np.array_equal(np.diff(out["off"])[:320][~holds[:320]], sizes[~holds[:320]])
    fis = np.arange(0, 320, 16)
    a, b = R.network_input(g["v"], g["f"], fis), R.network_input(g["v"], g["f"], fis, skip_degenerate=True)
    assert all(np.array_equal(a[key], b[key]) for key in a)
    # without the option the reference's NaN normal reaches the tensor wherever the scaled face's cross product
    # rounds to exactly zero (elsewhere it is a finite direction of weight ~1e-19)
    poisoned = 0
    for i in np.nonzero(holds)[0]:
        try:
            poisoned += bool(np.isnan(R.patch_input(v, f, int(i), out["faces"][out["off"][i]:out["off"][i + 1]])[1]).any())
        except np.linalg.LinAlgError:
            poisoned += 1
    assert poisoned > 0


def test_bunny_subset_has_boundary_patches_and_a_known_smallest_gap():
    fis, dropped = C.bunny_subset()
    v, f, fis2, out = C.edge_case("bunny_subset")
    assert np.array_equal(fis, fis2) and dropped <= 4 and len(fis) == 440 - dropped
    gap = R.relgap(out["eig"])
    assert 7.4e-5 <= gap[:400].min() < 7.5e-5 and gap[400:].min() >= C.BUNNY_MIN_RELGAP
    assert (out["pi"][:400] >= R.ROWS).sum() == 15 and np.all(out["pi"] >= 0)
    assert np.all((R.tta(f)[fis[400:]] < 0).any(axis=1))
    size = np.minimum(np.diff(out["off"]), R.ROWS)
    assert (out["inputs"][:, :, 7][np.arange(R.ROWS)[None, :] < size[:, None]] < 3).any()


def test_open_grid_has_boundary_rows():
    v, f, fis, out = C.edge_case("open_grid")
    size = np.minimum(np.diff(out["off"]), R.ROWS)
    assert len(fis) == 128 and (out["inputs"][:, :, 7][np.arange(R.ROWS)[None, :] < size[:, None]] < 3).any()
    assert R.relgap(out["eig"]).min() > 0 and np.isfinite(out["inputs"]).all()
