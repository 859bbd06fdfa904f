"""Meshes, the golden loaders and the tolerance shared by the patch tests (test_patch_ref.py, test_gpu_patch.py,
test_gpu_patch_edges.py)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = np.finfo(np.float64).eps

_cache = {}


def load_golden(name):
    """tests/golden/patch_<name>.npz as a dict (the shells' inputs come in three parts); loaded once."""
    if name not in _cache:
        g = dict(np.load(os.path.join(GOLDEN, f"patch_{name}.npz")))
        if "inputs" not in g:
            g["inputs"] = np.concatenate([np.load(os.path.join(GOLDEN, f"patch_{name}_inputs_{p}.npz"))["inputs"]
                                          for p in range(3)])
        assert len(g["inputs"]) == len(g["input_faces"])
        for a in g.values():
            a.setflags(write=False)
        _cache[name] = g
    return _cache[name]


def cached(key, make):
    """make() once per key: the restatement's output for a fixture, shared by the tests and left unchanged."""
    if key not in _cache:
        out = make()
        for a in (out.values() if isinstance(out, dict) else ()):
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def tolerance(relgap):
    """512 eps / relgap per patch, absolute, for rotations and feature columns (all aligned coordinates lie in
    [-1, 1]): eigenvector perturbation |dv| <= |dT| / gap with |dT| <~ m eps |T| over m <= 160 summed terms."""
    return 512 * EPS / np.asarray(relgap)


def octahedron():
    """The mesh of the reference's Tests/test_PatchCollector.py."""
    v = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1], [0, -1, 0], [-1, 0, 0]], dtype=np.float64)
    f = np.array([[1, 0, 2], [1, 2, 3], [3, 2, 4], [3, 4, 5], [4, 0, 5], [0, 1, 5], [2, 0, 4], [1, 3, 5]])
    return v, f


def strip():
    """Four triangles in a row; edge adjacency [[-1,1,-1],[-1,2,0],[1,3,-1],[-1,-1,2]]."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 2, 0], [1, 2, 0]], dtype=np.float64)
    f = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 5, 4]])
    return v, f


STRIP_TT = np.array([[-1, 1, -1], [-1, 2, 0], [1, 3, -1], [-1, -1, 2]])


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return v, f


def open_grid(n=9, seed=5):
    """An n x n vertex height field with a boundary (2 (n-1)^2 faces), jittered so that no test is a tie."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    v = np.stack([x, y, 0.3 * np.sin(x) * np.cos(0.7 * y)], axis=-1).reshape(-1, 3) + rng.normal(0, 0.05, (n * n, 3))
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i, i + n, i + 1], axis=1), np.stack([i + 1, i + n, i + n + 1], axis=1)])
    return v, f


def bunny():
    d = np.load(os.path.join(os.path.dirname(GOLDEN), "..", "data", "stanford_bunny_mesh.npz"))
    return np.asarray(d["v"], dtype=np.float64), np.asarray(d["f"], dtype=np.int64)


# ---------------------------------------------------------------------------------------------- edge fixtures
# (test_patch_ref.py asserts what each of them is said to reach; test_gpu_patch_edges.py runs them on the device)
def box(sides=(1.0, 0.8, 0.6), shift=(0.0, 0.0, 0.0), scale=1.0):
    """cube() centred on the origin with the given sides, times scale, plus shift: every patch is the whole mesh."""
    v, f = cube()
    return (v - 0.5) * np.asarray(sides, dtype=np.float64) * scale + np.asarray(shift, dtype=np.float64), f


_HALF_DIAGONAL = 0.5 * np.sqrt(1.0 + 0.8 ** 2 + 0.6 ** 2)
# name -> (box arguments, does Patch.alignPatch translate, does it scale): its two numpy.allclose branches
BOXES = {
    "centred": ({}, False, True),                                       # the vertex mean is exactly 0
    "near_origin": ({"shift": (3e-9, -2e-9, 2.5e-9)}, False, True),     # |c| <= 1e-8: resized and rotated about c
    "unit_size": ({"scale": (1.0 + 5e-6) / _HALF_DIAGONAL}, False, False),   # |size - 1| <= 1e-8 + 1e-5
    "above_unit_size": ({"scale": (1.0 + 2e-5) / _HALF_DIAGONAL}, False, True),
}


def box_variant(name):
    return box(**BOXES[name][0])


def load_align(name):
    """The reference's output for box_variant(name) out of tests/golden/patch_align.npz, keyed as load_golden's."""
    if "align" not in _cache:
        _cache["align"] = dict(np.load(os.path.join(GOLDEN, "patch_align.npz")))
        for a in _cache["align"].values():
            a.setflags(write=False)
    return {key.split("/", 1)[1]: a for key, a in _cache["align"].items() if key.startswith(name + "/")}


def tiny_ellipsoid():
    """(v, f, faces): the golden ellipsoid times 2^-27, so that every patch's vertex mean is below 1e-8 and no patch
    is translated, while the scaling is exact in binary and the selection is the unscaled mesh's."""
    g = load_golden("ellipsoid")
    return np.array(g["v"]) * 2.0 ** -27, np.array(g["f"]), np.arange(0, len(g["f"]), 5)


NEEDLE = np.array([[0, 0, 0], [100, 0, 0], [0, 1, 0]], dtype=np.float64)


def _needle_parts(at):
    ov, of = octahedron()
    ov = ov * np.array([2.0, 1.5, 1.0]) + np.random.default_rng(7).normal(0, .05, ov.shape) + np.asarray(at)
    return ov, of


def needle(order="last"):
    """(v, f, index of the needle's face).  A long thin triangle whose ball (r = 28.28) holds none of its own vertices
    (each >= 33.3 from its centre) but all of a small octahedron at its centroid: a patch without its own face."""
    ov, of = _needle_parts(NEEDLE.mean(axis=0))
    if order == "last":
        return np.concatenate([ov, NEEDLE]), np.concatenate([of, [[6, 7, 8]]]), 8
    assert order == "first"
    return np.concatenate([NEEDLE, ov]), np.concatenate([[[0, 1, 2]], of + 3]), 0


def needle_far():
    """(v, f, 4): the octahedron moved to x = 1000 and the needle as face 4 of 9: its patch is empty, between others."""
    ov, of = _needle_parts((1000.0, 0.0, 0.0))
    return np.concatenate([ov, NEEDLE]), np.concatenate([of[:4], [[6, 7, 8]], of[4:]]), 4


def offset_grid(scale, offset):
    """open_grid() as v * scale + offset: far from the origin the fp32 copy of the vertices, which the selection's
    cell grid is built over, loses the mesh's own extent."""
    v, f = open_grid()
    return v * scale + offset, f


OFFSET_GRIDS = {"1e3": (0.01, 1e3), "collapsed": (0.001, 1e5)}


def ellipsoid_degenerate():
    """(v, f): the golden ellipsoid plus one face of three collinear vertices just outside face 10, sharing nothing
    with the rest: it lies in other faces' patches, and its own ball (r = 0) is empty."""
    g = load_golden("ellipsoid")
    v, f = np.array(g["v"]), np.array(g["f"])
    p = 1.02 * v[f[10]].mean(axis=0)
    d = np.array([0.01, 0.004, -0.003])
    n = len(v)
    return np.concatenate([v, [p, p + d, p + 2 * d]]), np.concatenate([f, [[n, n + 1, n + 2]]])


BUNNY_MIN_RELGAP = 5e-5


def bunny_subset():
    """(faces, boundary faces dropped): 400 random faces of the bunny plus the 40 lowest-numbered faces with a
    boundary edge, less those of the 40 whose relative eigen-gap (restatement) is below 5e-5."""
    if "bunny_subset" not in _cache:
        import patch_ref as R
        v, f = bunny()
        rand = np.random.default_rng(11).choice(len(f), 400, replace=False)
        edge = np.nonzero((R.tta(f) < 0).any(axis=1))[0][:40]
        gap = R.relgap(R.network_input(v, f, edge)["eig"])
        keep = edge[gap >= BUNNY_MIN_RELGAP]
        _cache["bunny_subset"] = (np.concatenate([rand, keep]).astype(np.int64), len(edge) - len(keep))
    return _cache["bunny_subset"]


def edge_case(name):
    """(v, f, requested faces, the restatement's network_input for them) of a named edge fixture; computed once."""
    def make():
        import patch_ref as R
        skip = False
        if name.startswith("box/"):
            v, f = box_variant(name[4:])
        elif name.startswith("needle_"):
            v, f, _ = needle_far() if name == "needle_far" else needle(name[7:])
        elif name.startswith("offset_grid/"):
            v, f = offset_grid(*OFFSET_GRIDS[name[12:]])
        elif name == "ellipsoid_degenerate":
            (v, f), skip = ellipsoid_degenerate(), True
        elif name == "bunny_subset":
            v, f = bunny()
        elif name == "tiny_ellipsoid":
            v, f, _ = tiny_ellipsoid()
        else:
            v, f = open_grid()
        fis = {"bunny_subset": lambda: bunny_subset()[0], "tiny_ellipsoid": lambda: tiny_ellipsoid()[2]}.get(
            name, lambda: np.arange(len(f)))()
        want = R.network_input(v, f, fis, skip_degenerate=skip)
        rows = [want["faces"][a:b] for a, b in zip(want["off"][:-1], want["off"][1:])]
        want["adjacency_columns"] = np.array([R.index_columns(R.tta(f[row]), "adjacency") for row in rows])
        for a in (v, f, fis, *want.values()):
            a.setflags(write=False)
        return v, f, fis, want
    assert name in EDGE_CASES, name
    return cached("edge/" + name, make)


EDGE_CASES = (["open_grid", "bunny_subset", "tiny_ellipsoid", "needle_last", "needle_first", "needle_far",
               "ellipsoid_degenerate"] + ["box/" + b for b in BOXES] + ["offset_grid/" + o for o in OFFSET_GRIDS])
