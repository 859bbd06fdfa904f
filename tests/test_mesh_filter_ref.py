"""Known answers for the numpy restatement of the guided bilateral mesh normal filtering (tests/mesh_filter_ref.py),
so that the yardstick of test_gpu_mesh_filter.py is itself pinned.  No device needed."""
import numpy as np

import mesh_filter_ref as R


def test_planar_grid_is_a_fixed_point():
    v, f = R.grid(9, 8)
    out_v, n = R.denoise(v, f, normal_iterations=3, vertex_iterations=4)
    np.testing.assert_array_equal(n, np.tile([0.0, 0.0, 1.0], (len(f), 1)))
    bbox = np.linalg.norm(v.max(0) - v.min(0))
    assert np.abs(out_v - v).max() <= 1e-15 * bbox


def test_interior_neighbourhood_size_of_the_regular_grid():
    # Unit cells split by the (0,0)-(1,1) diagonal: centroids at (x + 2/3, y + 1/3) and (x + 1/3, y + 2/3).  Faces over
    # an edge lie sqrt(2)/3 (the diagonal) or sqrt(5)/3 (a cell side, twice) apart, so m = (sqrt(2) + 2 sqrt(5)) / 9 =
    # 0.654 in the interior and the radius is 2 m = 1.308, r^2 = 1.711.  Around a lower triangle the squared distances
    # are a^2 + b^2 to the lower triangle of cell (a, b): 0, 1 x 4 within, 2 outside -> 5 faces; and (a - 1/3)^2 +
    # (b + 1/3)^2 to the upper one: 2/9, 5/9 x 2, 8/9 within, 17/9 = 1.889 outside -> 4 faces.  All 9 share a vertex with
    # the centre.  The upper triangles are the point reflection.  (The boundary shifts m by a few per cent; the nearest
    # squared distances to r^2 are 1 and 1.889.)
    nx, ny = 10, 9
    v, f = R.grid(nx, ny)
    off, nbr, radius = R.default_neighbourhoods(v, f, multiple_radius=2)
    assert 1.0 < radius < np.sqrt(17 / 9)
    assert abs(radius - 2 * (np.sqrt(2) + 2 * np.sqrt(5)) / 9) < 0.05
    sizes = np.diff(off).reshape(nx - 1, ny - 1, 2)
    assert (sizes[2:-2, 2:-2] == 9).all()
    assert sizes.max() == 9 and sizes.min() < 9            # boundary rows are shorter
    # vertex mode: 6 faces around each of the three corners, minus the shared ones: 13 in the interior
    voff, _, _ = R.default_neighbourhoods(v, f, mode="vertex")
    assert (np.diff(voff).reshape(nx - 1, ny - 1, 2)[1:-1, 1:-1] == 13).all()


def test_two_sheets_do_not_see_each_other():
    v, f, sheet = R.two_sheets()
    off, nbr, radius = R.default_neighbourhoods(v, f)
    c = R.face_geometry(v, f)[0]
    rows = np.repeat(np.arange(len(f)), np.diff(off))
    assert (sheet[rows] == sheet[nbr]).all()
    for i in range(len(f)):
        assert (sheet[R.euclidean_ball(c, i, radius)] != sheet[i]).any()
        assert i in nbr[off[i]:off[i + 1]]
        assert (np.diff(nbr[off[i]:off[i + 1]]) > 0).all()


def test_no_parity_mesh_has_a_centroid_distance_at_its_radius():
    for name, (v, f, mr) in R.parity_cases().items():
        vf, ni = R.vta(f, len(v))
        c = R.face_geometry(v, f)[0]
        radius = mr * R.mean_adjacent_distance(c, f, vf, ni)[0]
        gap = np.inf
        for s in range(0, len(c), 512):
            d = np.linalg.norm(c[s:s + 512, None, :] - c[None, :, :], axis=2)
            gap = min(gap, float(np.abs(d - radius).min()))
        assert gap > 1e-9 * radius, (name, gap, radius)


def test_degenerate_face_and_isolated_vertex():
    v, f, bad, lone = R.guard_mesh()
    c, area, n = R.face_geometry(v, f)
    assert area[bad] == 0 and (n[bad] == 0).all() and np.isfinite(n).all()
    out_v, out_n = R.denoise(v, f, normal_iterations=2, vertex_iterations=3)
    assert np.isfinite(out_v).all() and np.isfinite(out_n).all()
    assert (out_n[bad] == 0).all()
    np.testing.assert_array_equal(out_v[lone], v[lone])
    # Mesh.updateVertices' own rule for a vertex in no face stays 0/0
    vf, ni = R.vta(f, len(v))
    assert np.isnan(R.update_vertices(v, f, n, vf, ni, 1, keep_isolated=False)[lone]).all()


def test_float32_run_stays_close_to_float64():
    v, f, _ = R.cube(4, 0.1, 2)
    csr = R.default_neighbourhoods(v, f)[:2]
    v64, n64 = R.denoise(v, f, normal_iterations=2, vertex_iterations=3, csr=csr)
    v32, n32 = R.denoise(v.astype(np.float32), f, normal_iterations=2, vertex_iterations=3, csr=csr)
    assert v32.dtype == np.float32 and n32.dtype == np.float32
    assert np.abs(v32 - v64).max() < 1e-4 and np.abs(n32 - n64).max() < 1e-4
