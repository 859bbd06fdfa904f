"""Guided bilateral normal filtering and Mesh.denoise on the device (csrc/mesh.hip: face geometry, the adjacent-centroid
mean, the face neighbourhoods, the filter pass, the loop) against the numpy restatement of the reference's
MeshNormalFiltering.cpp:47-244 in tests/mesh_filter_ref.py (pinned by test_mesh_filter_ref.py)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mesh_filter_ref as R
import pcd_native as nat
from conftest import ROOT, report
from PatchGeneration.Modules.Mesh import Mesh

pytestmark = pytest.mark.gpu

NAMES = ["open_grid", "cube", "two_sheets", "wide_rows", "guard"]
_CACHE = {}


def case(name):
    """The mesh and its restatement (computed once, never modified)."""
    if name not in _CACHE:
        v, f, mr = R.parity_cases()[name]
        vf, ni = R.vta(f, len(v))
        c, area, n = R.face_geometry(v, f)
        m, pairs = R.mean_adjacent_distance(c, f, vf, ni)
        radius = mr * m
        _CACHE[name] = SimpleNamespace(
            v=v, f=f, mr=mr, vf=vf, ni=ni, c=c, area=area, n=n, m=m, pairs=pairs, radius=radius,
            csr=R.neighbourhoods(c, f, vf, ni, "radius", radius), csr_vertex=R.neighbourhoods(c, f, vf, ni, "vertex"),
            bbox=float(np.linalg.norm(v.max(0) - v.min(0))))
        for a in (v, f, c, area, n) + _CACHE[name].csr + _CACHE[name].csr_vertex:
            a.setflags(write=False)
    return _CACHE[name]


def guidance(k, seed=7):
    """Unit normals near the mesh's own: a stand-in for a network's prediction."""
    g = k.n + np.random.default_rng(seed).normal(0, 0.15, k.n.shape)
    ln = np.linalg.norm(g, axis=1)
    return np.where((ln > 0)[:, None], g / np.where(ln > 0, ln, 1)[:, None], 0)


# ------------------------------------------------------------------------------------------------ 1-3: geometry
@pytest.mark.parametrize("name", NAMES)
def test_face_geometry_is_bit_identical(gpu, name):
    k = case(name)
    c, area, n = nat.mesh_face_geometry(torch.from_numpy(k.v.copy()).to(gpu), torch.from_numpy(k.f.copy()).to(gpu))
    np.testing.assert_array_equal(c.cpu().numpy(), k.c)
    np.testing.assert_array_equal(area.cpu().numpy(), k.area)
    np.testing.assert_array_equal(n.cpu().numpy(), k.n)
    mesh = Mesh(k.v.copy(), k.f.copy())
    np.testing.assert_array_equal(mesh.getFaceCentroids(), k.c)
    np.testing.assert_array_equal(mesh.getFaceAreas(), k.area)


@pytest.mark.parametrize("name", NAMES)
def test_mean_adjacent_centroid_distance(gpu, name):
    k = case(name)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    out = nat.mesh_face_scale(dev(k.c), dev(k.f), dev(k.vf), dev(k.ni)).cpu().numpy()
    assert int(out[1]) == k.pairs
    rel = abs(out[0] - k.m) / k.m
    print(f"{name}: m {out[0]!r} restatement {k.m!r} rel {rel:.2e} pairs {k.pairs}")
    assert rel <= 1e-12
    assert Mesh(k.v.copy(), k.f.copy()).getMeanCentroidDistance() == out[0]      # deterministic


def _assert_csr(got, want):
    off, nbr = got
    np.testing.assert_array_equal(off, want[0])
    np.testing.assert_array_equal(nbr, want[1])
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    inner = np.ones(len(nbr), bool)
    inner[off[:-1]] = False
    assert (np.diff(nbr)[inner[1:]] > 0).all()              # rows ascending
    assert np.bincount(rows[nbr == rows], minlength=len(off) - 1).min() == 1   # the centre, once


@pytest.mark.parametrize("name", NAMES)
def test_neighbourhoods_equal_the_restatement_on_every_row(gpu, name):
    k = case(name)
    mesh = Mesh(k.v.copy(), k.f.copy())
    _assert_csr(mesh.getFaceNeighbourhoods("radius", radius=k.radius), k.csr)         # the restatement's radius
    _assert_csr(mesh.getFaceNeighbourhoods("radius", multiple_radius=k.mr), k.csr)    # the device's own
    _assert_csr(mesh.getFaceNeighbourhoods("vertex"), k.csr_vertex)
    if name == "wide_rows":
        assert np.diff(k.csr[0]).max() > 64
    if name == "two_sheets":
        sheet = R.two_sheets()[2]
        off, nbr = mesh.getFaceNeighbourhoods()
        assert (sheet[np.repeat(np.arange(len(k.f)), np.diff(off))] == sheet[nbr]).all()


def test_neighbourhood_overflow_is_an_error_not_a_write(gpu):
    k = case("open_grid")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    cap = torch.from_numpy(np.diff(k.csr[0])).to(gpu)
    args = (dev(k.c), dev(k.f), dev(k.vf), dev(k.ni), 0, k.radius)
    off, nbr = nat.mesh_neighbourhoods(*args, cap)                                    # exact capacities fit
    _assert_csr((off.cpu().numpy(), nbr.cpu().numpy()), k.csr)
    with pytest.raises(ValueError, match="does not fit"):
        nat.mesh_neighbourhoods(*args, torch.clamp(cap - 1, min=0))


# ------------------------------------------------------------------------------------------------ 4: one pass
@pytest.mark.parametrize("name", NAMES)
def test_one_filter_pass_fp64(gpu, name):
    k = case(name)
    mesh = Mesh(k.v.copy(), k.f.copy())
    worst = 0.0
    for g in (guidance(k), None):
        want = R.filter_pass(k.c, k.area, k.n if g is None else g, k.n if g is None else g, *k.csr, 0.3, 1 * k.m)
        got = mesh.filterNormals(guided=g, multiple_radius=k.mr)
        worst = max(worst, float(np.abs(got - want).max()))
        # another source than the guidance (the later iterations of the loop)
        want = R.filter_pass(k.c, k.area, k.n if g is None else g, k.n, *k.csr, 0.45, 1.5 * k.m)
        got = mesh.filterNormals(guided=g, normals=k.n, sigma_r=0.45, multiple_sigma_s=1.5, multiple_radius=k.mr)
        worst = max(worst, float(np.abs(got - want).max()))
    report(f"one filter pass fp64, {name}: max |dn| {worst:.2e} (bound 1e-13)")
    assert worst <= 1e-13


# ------------------------------------------------------------------------------------------------ 5: the loop
def _ulp_perturbed(v, seed=9):
    return v * (1 + np.random.default_rng(seed).choice([-1.0, 1.0], v.shape) * np.finfo(np.float64).eps)


@pytest.mark.parametrize("iters", [(3, 4), (12, 16)])
@pytest.mark.parametrize("name", ["cube", "open_grid"])
def test_whole_loop_fp64(gpu, name, iters):
    k = case(name)
    want_v, want_n = R.denoise(k.v, k.f, None, *iters, csr=k.csr)
    # the restatement's own sensitivity: its answer to a 1-ulp relative perturbation of the input vertices
    sens = float(np.abs(R.denoise(_ulp_perturbed(k.v), k.f, None, *iters, csr=k.csr)[0] - want_v).max())
    mesh = Mesh(k.v.copy(), k.f.copy())
    n = mesh.denoise(normal_iterations=iters[0], vertex_iterations=iters[1])
    dev_v, dev_n = float(np.abs(mesh.v - want_v).max()), float(np.abs(n - want_n).max())
    allow = 3 * sens + 1e-12 * k.bbox
    report(f"loop fp64 {name} {iters[0]}x{iters[1]}: max |dv| {dev_v:.2e} (sensitivity {sens:.2e}, allowed {allow:.2e}, "
           f"bbox {k.bbox:.1f}), max |dn| {dev_n:.2e}")
    assert dev_v <= allow
    # with guidance
    g = guidance(k)
    want_v = R.denoise(k.v, k.f, g, *iters, csr=k.csr)[0]
    mesh = Mesh(k.v.copy(), k.f.copy())
    mesh.denoise(guided_normals=g, normal_iterations=iters[0], vertex_iterations=iters[1])
    assert float(np.abs(mesh.v - want_v).max()) <= allow


# ------------------------------------------------------------------------------------------------ 6: fp32
@pytest.mark.parametrize("name", ["cube", "open_grid"])
def test_fp32_path_against_the_fp64_device_path(gpu, name):
    k = case(name)
    v32 = k.v.astype(np.float32)
    v = v32.astype(np.float64)                              # fp32-rounded inputs for both paths
    # same neighbourhoods: built in fp64 from the same vertices
    m64, m32 = Mesh(v.copy(), k.f.copy()), Mesh(v32.copy(), k.f.copy())
    csr = m64.getFaceNeighbourhoods()
    _assert_csr(m32.getFaceNeighbourhoods(), csr)
    # one pass; allowance: 3 x what float32 numpy costs the restatement
    c, area, n = R.face_geometry(v, k.f)
    m = R.mean_adjacent_distance(c, k.f, k.vf, k.ni)[0]
    c32, area32, n32 = R.face_geometry(v32, k.f)
    ref_dev = float(np.abs(R.filter_pass(c32, area32, n32, n32, *csr, 0.3, np.float32(m)).astype(np.float64)
                           - R.filter_pass(c, area, n, n, *csr, 0.3, m)).max())
    got = m32.filterNormals(fp32=True)
    assert got.dtype == np.float32
    dev = float(np.abs(got.astype(np.float64) - m64.filterNormals()).max())
    report(f"one pass fp32 {name}: max |dn| vs fp64 device {dev:.2e}, float32 restatement "
           f"{ref_dev:.2e}")
    assert dev <= 3 * ref_dev
    # the loop
    for iters in ((3, 4), (12, 16)):
        ref_dev = float(np.abs(R.denoise(v32, k.f, None, *iters, csr=csr)[0].astype(np.float64)
                               - R.denoise(v, k.f, None, *iters, csr=csr)[0]).max())
        a, b = Mesh(v.copy(), k.f.copy()), Mesh(v32.copy(), k.f.copy())
        a.denoise(normal_iterations=iters[0], vertex_iterations=iters[1])
        b.denoise(normal_iterations=iters[0], vertex_iterations=iters[1], fp32=True)
        assert b.v.dtype == np.float32
        dev = float(np.abs(b.v.astype(np.float64) - a.v).max())
        report(f"loop fp32 {name} {iters[0]}x{iters[1]}: max |dv| vs fp64 device {dev:.2e}, "
               f"float32 restatement {ref_dev:.2e} (bbox {k.bbox:.1f})")
        assert dev <= 3 * ref_dev


# ------------------------------------------------------------------------------------------------ 7: guards
@pytest.mark.parametrize("fp32", [False, True])
def test_guards_on_a_degenerate_face_and_an_isolated_vertex(gpu, fp32):
    v, f, bad, lone = R.guard_mesh()
    if fp32:
        v = v.astype(np.float32)
    mesh = Mesh(v.copy(), f.copy())
    assert np.isfinite(mesh.getFaceCentroids()).all() and mesh.getFaceAreas()[bad] == 0
    one = mesh.filterNormals(fp32=fp32)
    assert np.isfinite(one).all() and (one[bad] == 0).all()
    n = mesh.denoise(normal_iterations=3, vertex_iterations=4, fp32=fp32)
    assert np.isfinite(mesh.v).all() and np.isfinite(n).all()
    np.testing.assert_array_equal(mesh.v[lone], v[lone])    # bit for bit
    assert (n[bad] == 0).all()
    assert np.abs(np.linalg.norm(np.delete(n, bad, 0), axis=1) - 1).max() < 1e-6
    if not fp32:
        want_v, want_n = R.denoise(v, f, None, 3, 4)
        assert np.abs(mesh.v - want_v).max() <= 1e-12 and np.abs(n - want_n).max() <= 1e-12
        # updateVertices keeps its own rule: a vertex in no face becomes 0/0, everything else moves as before
        vf, ni = R.vta(f, len(v))
        want = R.update_vertices(v, f, want_n, vf, ni, 2, keep_isolated=False)
        m2 = Mesh(v.copy(), f.copy())
        m2.updateVertices(want_n, k=2)
        assert np.isnan(m2.v[lone]).all() and np.isnan(want[lone]).all()
        np.testing.assert_allclose(np.delete(m2.v, lone, 0), np.delete(want, lone, 0), rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------ 8: behaviour
def test_range_term_keeps_the_cube_edges(gpu):
    _, f, clean = R.cube(8)
    truth = R.face_geometry(clean, f)[2]
    noisy = R.gaussian_noise(clean, f, 0.2)
    c = R.face_geometry(clean, f)[0]
    # faces in the cells along the cube's 12 edges: two of the centroid's coordinates within one cell of a side
    near = (np.minimum(c, 8 - c) < 1).sum(1) >= 2
    err = lambda v, rows=None: R.mean_angle_deg(R.face_geometry(v, f)[2], truth, rows)
    guided, plain = Mesh(noisy.copy(), f.copy()), Mesh(noisy.copy(), f.copy())
    guided.denoise()
    plain.denoise(sigma_r=1e6)                              # no range term: plain area- and distance-weighted passes
    report(f"cube, noise 0.2 x mean edge: mean normal error noisy {err(noisy):.2f} deg, denoise() {err(guided.v):.2f}, "
           f"without the range term {err(plain.v):.2f}; near the edges ({int(near.sum())} faces): noisy "
           f"{err(noisy, near):.2f}, denoise() {err(guided.v, near):.2f}, without {err(plain.v, near):.2f}")
    assert err(guided.v) < err(noisy)
    assert err(guided.v, near) < err(noisy, near)
    assert err(guided.v, near) < err(plain.v, near)


# ------------------------------------------------------------------------------------------------ 9: bunny
def test_bunny(gpu):
    d = np.load(os.path.join(ROOT, "data", "stanford_bunny_mesh.npz"))
    clean, f = d["v"].astype(np.float64), d["f"].astype(np.int64)
    truth = R.face_geometry(clean, f)[2]
    noisy = R.gaussian_noise(clean, f, 0.2)
    used = np.zeros(len(clean), bool)
    used[f.reshape(-1)] = True
    err = lambda v: R.mean_angle_deg(R.face_geometry(v, f)[2], truth)
    e0 = err(noisy)
    mesh = Mesh(noisy.copy(), f.copy())
    off, nbr = mesh.getFaceNeighbourhoods()
    vf, ni = R.vta(f, len(clean))
    c = R.face_geometry(noisy, f)[0]
    radius = 2 * R.mean_adjacent_distance(c, f, vf, ni)[0]
    rows = np.sort(np.random.default_rng(13).choice(len(f), 500, replace=False))
    roff, rnbr = R.neighbourhoods(c, f, vf, ni, "radius", radius, rows=rows)
    for t, i in enumerate(rows):
        np.testing.assert_array_equal(nbr[off[i]:off[i + 1]], rnbr[roff[t]:roff[t + 1]])
    sizes = np.diff(off)
    for fp32 in (False, True):
        m = Mesh(noisy.astype(np.float32) if fp32 else noisy.copy(), f.copy())
        n = m.denoise(normal_iterations=5, fp32=fp32)
        assert np.isfinite(m.v[used]).all() and np.isfinite(n).all()
        np.testing.assert_array_equal(m.v[~used], (noisy.astype(np.float32) if fp32 else noisy)[~used])
        e1 = err(m.v.astype(np.float64))
        report(f"bunny ({len(f)} faces, {int((~used).sum())} vertices in no face, rows mean {sizes.mean():.1f} max "
               f"{sizes.max()}), fp32={fp32}: mean normal error {e0:.2f} -> {e1:.2f} deg after 5 x 16")
        assert e1 <= e0 / 2 + 2


# ------------------------------------------------------------------------------------------------ 10: API
def test_api(gpu):
    k = case("open_grid")
    for dt in (np.float64, np.float32):
        v = k.v.astype(dt)
        mesh = Mesh(v, k.f.copy())
        n = mesh.denoise(normal_iterations=2, vertex_iterations=2, fp32=dt == np.float32)
        assert mesh.v is v and v.dtype == dt and not np.array_equal(v, k.v.astype(dt))   # in place, same dtype
        assert n.shape == (len(k.f), 3)
    # normal_iterations = 0 leaves v untouched and returns the guidance
    mesh = Mesh(k.v.copy(), k.f.copy())
    n = mesh.denoise(normal_iterations=0)
    np.testing.assert_array_equal(mesh.v, k.v)
    np.testing.assert_array_equal(n, k.n)
    # the neighbourhoods follow the faces: reassigned, and edited in place
    off0, _ = mesh.getFaceNeighbourhoods()
    mesh.f = k.f[:100].copy()
    off1, nbr1 = mesh.getFaceNeighbourhoods()
    assert len(off1) == 101 and nbr1.max() < 100
    mesh.f[:] = mesh.f[::-1].copy()
    c = R.face_geometry(k.v, mesh.f)[0]
    vf, ni = R.vta(mesh.f, len(k.v))
    want = R.neighbourhoods(c, mesh.f, vf, ni, "radius", 2 * R.mean_adjacent_distance(c, mesh.f, vf, ni)[0])
    _assert_csr(mesh.getFaceNeighbourhoods(), want)
    # bad arguments raise before any kernel runs
    mesh = Mesh(k.v.copy(), k.f.copy())
    for bad in (dict(guided_normals=k.n[:-1]), dict(guided_normals=k.n.T), dict(sigma_r=0), dict(sigma_r=-1.0),
                dict(mode="edge"), dict(multiple_sigma_s=0), dict(normal_iterations=-1)):
        with pytest.raises(ValueError):
            mesh.denoise(**bad)
    with pytest.raises(ValueError):
        mesh.filterNormals(normals=k.n[:5])
    with pytest.raises(ValueError):
        mesh.getFaceNeighbourhoods("ball")
    np.testing.assert_array_equal(mesh.v, k.v)
