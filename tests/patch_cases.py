"""Meshes, the golden loader and the tolerance shared by the patch tests (test_patch_ref.py, test_gpu_patch.py)."""
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
