"""GPU: the network input built on the device (csrc/patch.hip behind Mesh.getPatch* and PatchCollector) against the
reference's own output (tests/golden/patch_*.npz) and the numpy restatement (tests/patch_ref.py).

Exact: edge adjacency, radius, selection CSR, centre index, index columns, chunking, run-to-run.  Rotations and
feature columns: up to the per-patch sign of the middle axis within 512 eps / relgap_i (patch_cases.tolerance).
"""
import numpy as np
import pytest
import torch

import patch_cases as C
import patch_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(gpu):
    import pcd_native as nat
    from PatchGeneration.Modules.Mesh import Mesh
    from PatchGeneration.Modules.PatchCollector import PatchCollector, PatchDataset
    return nat, Mesh, PatchCollector, PatchDataset


def _mesh_arrays(name):
    if name in ("ellipsoid", "shells"):
        g = C.load_golden(name)
        return np.array(g["v"]), np.array(g["f"])
    return getattr(C, name)()


_full = {}


def full_run(mods, name, dtype=np.float64, neighbours="reference"):
    """collectNetworkInput over every face of a fixture, once per (fixture, dtype, mode)."""
    key = (name, np.dtype(dtype).name, neighbours)
    if key not in _full:
        v, f = _mesh_arrays(name)
        ds = mods[2](mods[1](v, f), 4).collectNetworkInput(128, neighbours=neighbours, dtype=dtype)
        for a in (ds.data_patch, ds.data_rotations, ds.centre_index, ds.patch_size, ds.radius):
            a.setflags(write=False)
        _full[key] = ds
    return _full[key]


# ------------------------------------------------------------------------------------------------ adjacency
@pytest.mark.parametrize("name", ["ellipsoid", "shells", "cube", "open_grid", "strip", "bunny"])
def test_edge_adjacency_equals_the_restatement(mods, gpu, name):
    nat = mods[0]
    v, f = _mesh_arrays(name)
    want = R.tta(f)
    for it in (torch.int64, torch.int32):
        got = nat.mesh_tta(torch.as_tensor(np.ascontiguousarray(f)).to(gpu).to(it), len(v), out_dtype=it)
        assert got.dtype == it and np.array_equal(got.cpu().numpy(), want)
    if name == "strip":
        assert np.array_equal(want, C.STRIP_TT)
    if name in ("open_grid", "bunny"):
        assert (want < 0).any()                          # the boundary is exercised


def test_edge_adjacency_rejects_bad_faces_and_skips_non_manifold_edges(mods, gpu):
    nat = mods[0]
    f = torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]], device=gpu)
    assert bool((nat.mesh_tta(f, 5) == -1).all())
    with pytest.raises(ValueError):
        nat.mesh_tta(f, 4)
    m = mods[1](*C.strip())
    assert np.array_equal(m.getTriangleTriangleAdjacency(), C.STRIP_TT)
    assert np.array_equal(m.getNeighbourhood(0, 2), [0, 1, 2]) and len(m.getNeighbourhood(0, 0)) == 0
    assert np.array_equal(m.getAreas(np.arange(4)), np.full(4, 0.5))


# ------------------------------------------------------------------------------------------------ radius, selection
@pytest.mark.parametrize("name", ["ellipsoid", "shells"])
def test_radius_and_selection_equal_the_reference(mods, name):
    g = C.load_golden(name)
    m = mods[1](np.array(g["v"]), np.array(g["f"]))
    assert np.array_equal(m.getPatchRadius(k=int(g["k"])), g["r"])
    off, faces = m.getPatchFaces(k=int(g["k"]))
    assert np.array_equal(off, g["off"]) and np.array_equal(faces, g["faces"])


@pytest.mark.parametrize("name", ["open_grid", "bunny"])
def test_radius_and_selection_equal_the_restatement(mods, name):
    v, f = _mesh_arrays(name)
    fis = np.arange(len(f)) if name == "open_grid" else np.sort(np.random.default_rng(11).choice(len(f), 2000, replace=False))
    centre, r = R.radius_centre(v, f, R.tta(f), fis)
    rows = [R.select(v, f, centre[i], r[i]) for i in range(len(fis))]
    m = mods[1](v, f)
    assert np.array_equal(m.getPatchRadius(fis), r)
    off, faces = m.getPatchFaces(fis)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(x) for x in rows])]))
    assert np.array_equal(faces, np.concatenate(rows))


def test_capacity_one_short_is_an_error_and_nothing_is_written(mods, gpu):
    g = C.load_golden("ellipsoid")
    m = mods[1](np.array(g["v"]), np.array(g["f"]))
    fis = m._faces_arg(None)
    total = int(g["off"][-1])
    buf = torch.full((total - 1,), -7, dtype=torch.int64, device=gpu)
    with pytest.raises(ValueError):
        m._patches(fis, 4, out=buf)
    assert bool((buf == -7).all())
    buf = torch.full((total,), -7, dtype=torch.int64, device=gpu)
    _, _, off, faces = m._patches(fis, 4, out=buf)
    assert faces.data_ptr() == buf.data_ptr() and np.array_equal(buf.cpu().numpy(), g["faces"])


# ------------------------------------------------------------------------------------------------ inputs, rotations
@pytest.mark.parametrize("name", ["ellipsoid", "shells"])
def test_inputs_and_rotations_equal_the_reference(mods, name):
    g = C.load_golden(name)
    ds = full_run(mods, name)
    keep, tol = g["input_faces"], C.tolerance(g["relgap"])
    assert ds.data_patch.shape == (len(g["f"]), 64, 20) and ds.data_patch.dtype == np.float64
    assert np.array_equal(ds.centre_index, g["pi"]) and np.array_equal(ds.patch_size, np.diff(g["off"]))
    assert np.array_equal(ds.radius, g["r"])
    assert ds.status == {"degenerate_faces": 0, "centre_outside_window": int((g["pi"] >= 64).sum()), "centre_missing": 0}
    assert ds.batch_size == mods[3].getPreferredBatchSize(len(g["f"]), 128)
    s = R.sign_align(ds.data_rotations, g["rot"])
    want_in, _ = R.apply_sign(g["inputs"], g["rot"][keep], s[keep])
    _, want_rot = R.apply_sign(np.zeros((len(s), 1, 20)), g["rot"], s)
    dev_rot = np.abs(ds.data_rotations - want_rot).max(axis=(1, 2))
    dev_in = np.abs(ds.data_patch[keep][:, :, :17] - want_in[:, :, :17]).max(axis=(1, 2))
    print(f"{name}: max deviation x relgap / eps: rotations {np.max(dev_rot * g['relgap']) / C.EPS:.1f}, "
          f"inputs {np.max(dev_in * g['relgap'][keep]) / C.EPS:.1f} (bound 512)")
    assert np.all(dev_rot <= tol) and np.all(dev_in <= tol[keep])
    assert np.array_equal(ds.data_patch[keep][:, :, 17:], g["inputs"][:, :, 17:])
    # canonical middle axis, proper rotation
    big = np.take_along_axis(ds.data_rotations[:, 1], np.abs(ds.data_rotations[:, 1]).argmax(1)[:, None], 1)
    assert np.all(big > 0) and np.allclose(np.linalg.det(ds.data_rotations), 1.0, atol=1e-12)


@pytest.mark.parametrize("name", ["ellipsoid", "shells"])
def test_float32_is_the_float64_result_cast_and_runs_repeat_bitwise(mods, name):
    ds = full_run(mods, name)
    d32 = full_run(mods, name, np.float32)
    assert d32.data_patch.dtype == np.float32 and np.array_equal(d32.data_patch, ds.data_patch.astype(np.float32))
    assert np.array_equal(d32.data_rotations, ds.data_rotations)
    v, f = _mesh_arrays(name)
    again = mods[2](mods[1](v, f), 4).collectNetworkInput(128)
    assert np.array_equal(again.data_patch, ds.data_patch) and np.array_equal(again.data_rotations, ds.data_rotations)


def test_adjacency_index_columns_equal_the_restatement(mods):
    g = C.load_golden("ellipsoid")
    fis = np.arange(0, len(g["f"]), 7)
    want = R.network_input(g["v"], g["f"], fis, neighbours="adjacency")
    ds = full_run(mods, "ellipsoid", neighbours="adjacency")
    assert np.array_equal(ds.data_patch[fis][:, :, 17:], want["inputs"][:, :, 17:])
    assert np.array_equal(ds.data_patch[:, :, :17], full_run(mods, "ellipsoid").data_patch[:, :, :17])
    v, f = C.strip()
    for mode, rows in (("adjacency", [[1, 1, 1], [2, 0, 0], [1, 3, 3], [2, 2, 2]] + [[63] * 3] * 60),
                       ("reference", [[1] * 3, [63] * 3, [0] * 3] + [[63] * 3] * 61)):
        st = mods[2](mods[1](v, f), 4).collectNetworkInput(4, neighbours=mode)
        assert np.array_equal(st.patch_size, [4, 4, 4, 4])
        for p in range(4):
            assert np.array_equal(st.data_patch[p, :, 17:], rows)
            assert np.array_equal(st.data_patch[p, :4, 7], [1, 2, 2, 1])


def test_octahedron_every_patch_is_the_whole_mesh(mods):
    v, f = C.octahedron()
    ds = mods[2](mods[1](v, f), 4).collectNetworkInput(8)
    assert np.array_equal(ds.patch_size, np.full(8, 8)) and np.array_equal(ds.centre_index, np.arange(8))
    assert np.all(ds.data_patch[:, :8, 7] == 3) and np.all(ds.data_patch[:, 8:, :17] == 0)
    assert np.all(ds.data_patch[:, 8:, 17:] == 63)


# ------------------------------------------------------------------------------------------------ chunking
def test_subsets_and_chunks_are_bitwise_rows_of_the_full_run(mods):
    ds = full_run(mods, "ellipsoid")
    v, f = _mesh_arrays("ellipsoid")
    pc = mods[2](mods[1](v, f), 4)
    fis = np.array([317, 5, 5, 0, 64, 200])
    sub = pc.collectNetworkInput(4, faces=fis)
    assert np.array_equal(sub.data_patch, ds.data_patch[fis]) and np.array_equal(sub.data_rotations, ds.data_rotations[fis])
    assert np.array_equal(sub.centre_index, ds.centre_index[fis])
    for size in (1, 63, 64, 65, len(f)):
        got = list(pc.iterNetworkInput(size))
        assert [len(b.faces) for b in got] == [min(size, len(f) - s) for s in range(0, len(f), size)]
        assert all(b.inputs.is_cuda and b.inputs.shape[1:] == (64, 20) for b in got)
        assert np.array_equal(torch.cat([b.inputs for b in got]).cpu().numpy(), ds.data_patch)
        assert np.array_equal(torch.cat([b.rotations for b in got]).cpu().numpy(), ds.data_rotations)
    cf = torch.cat([b.inputs for b in pc.iterNetworkInput(100, channels_first=True, dtype=np.float32)])
    assert cf.shape == (len(f), 20, 64) and cf.dtype == torch.float32
    assert np.array_equal(cf.cpu().numpy(), ds.data_patch.astype(np.float32).transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------ round trip
def test_unalign_returns_the_face_normals_and_feeds_denoise(mods):
    ds = full_run(mods, "ellipsoid")
    v, f = _mesh_arrays("ellipsoid")
    m = mods[1](v.copy(), f)
    fn = m.getFaceNormals()
    inside = (ds.centre_index >= 0) & (ds.centre_index < 64)
    assert inside.sum() == 290
    aligned = np.zeros((len(f), 3))
    aligned[inside] = ds.data_patch[np.nonzero(inside)[0], ds.centre_index[inside], 3:6]
    back = ds.unalign(aligned)
    assert np.abs(back[inside] - fn[inside]).max() <= 1e-12
    guided = np.where(inside[:, None], back, fn)
    out = m.denoise(guided_normals=guided, normal_iterations=2, vertex_iterations=4)
    assert out.shape == (len(f), 3) and np.isfinite(out).all() and np.isfinite(m.v).all()
    assert np.abs(m.v - v).max() > 0


# ------------------------------------------------------------------------------------------------ input checks
def test_empty_out_of_range_and_degenerate_inputs(mods):
    v, f = _mesh_arrays("ellipsoid")
    pc = mods[2](mods[1](v, f), 4)
    ds = pc.collectNetworkInput(8, faces=[])
    assert ds.data_patch.shape == (0, 64, 20) and ds.data_rotations.shape == (0, 3, 3) and len(ds) == 0
    assert ds.centre_index.shape == (0,) and ds.patch_size.shape == (0,) and ds.batch_size == 0
    off, faces = pc.mesh.getPatchFaces([])
    assert np.array_equal(off, [0]) and faces.shape == (0,)
    for bad in ([len(f)], [-1], [0, 10 ** 12]):
        with pytest.raises(ValueError):
            pc.collectNetworkInput(8, faces=bad)
        with pytest.raises(ValueError):
            pc.mesh.getPatchRadius(bad)
    with pytest.raises(ValueError):
        pc.collectNetworkInput(8, neighbours="igl")
    with pytest.raises(ValueError):
        pc.collectNetworkInput(8, dtype=np.float16)
    with pytest.raises(ValueError):
        mods[2](object())
    fd = np.concatenate([f, [[0, 0, 1]]])               # one face of zero area
    dg = mods[2](mods[1](v, fd), 4).collectNetworkInput(8)
    assert dg.data_patch.shape == (len(fd), 64, 20) and dg.status["degenerate_faces"] == 1
    ok = mods[2](mods[1](v, f), 4).collectNetworkInput(8)
    assert ok.status["degenerate_faces"] == 0
