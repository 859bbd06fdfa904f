"""Generate tests/golden/patch_ellipsoid.npz, patch_shells*.npz and patch_align.npz by running the REFERENCE's patch
pipeline.  `make_patch_golden.py NAME...` writes only the named ones (ellipsoid, shells, align); no name, all three.

TEST INFRASTRUCTURE ONLY (build container, needs the reference checkout next to this repository's tests, as
make_golden.py does).  The reference's PatchCollector.collectPatches, Patch.toGraph and FileDataset.file2input run
unmodified; the four igl functions they call are replaced by numpy statements of their published behaviour, and h5py
is stubbed when absent (only the file-system half of DataUtils uses it).

Fixtures (numpy.random.default_rng(3), the ellipsoid's noise drawn first, then the shells'); v0 = the unit icosphere
subdivided twice (162 vertices, 320 faces):
  ellipsoid   v0 * (1, 0.7, 0.45) + N(0, 0.02)                        320 faces, padding and truncation
  shells      [v0 ; 1.12 v0] + N(0, 0.02), two closed components      640 faces, every patch spans both sheets
Stored per fixture: v, f, the selection CSR and r for every face, the rotations, pi and relative eigen-gap for every
face, the [64, 20] inputs of every third face plus every face whose centre lies beyond the window (input_faces), and
the reference's seconds per patch.  The shells' inputs go to three files of their own so that no file passes 1 MiB.
patch_align.npz holds the four boxes of patch_cases.BOXES (the two numpy.allclose branches of Patch.alignPatch), every
array under "<variant>/<key>": all 12 inputs each, plus translated / scaled [12]: whether alignPatch called translate
and resize on that patch.
The generator asserts: selection margin min|d - r| / r >= 1e-8, relative gap >= 1e-5, no NaN.
"""
import contextlib
import io
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import patch_cases  # noqa: E402
import refshim  # noqa: E402

refshim.install()


# ---- numpy statements of the igl functions the patch pipeline calls
def triangle_triangle_adjacency(f):
    f = np.asarray(f)
    edges = {}
    for g in range(len(f)):
        for e in range(3):
            a, b = int(f[g, e]), int(f[g, (e + 1) % 3])
            edges.setdefault((min(a, b), max(a, b)), []).append((g, e))
    tt = -np.ones((len(f), 3), dtype=np.int64)
    tti = -np.ones((len(f), 3), dtype=np.int64)
    for users in edges.values():
        if len(users) == 2:
            (g0, e0), (g1, e1) = users
            tt[g0, e0], tti[g0, e0], tt[g1, e1], tti[g1, e1] = g1, e1, g0, e0
    return tt, tti


def vertex_triangle_adjacency(f, n):
    flat = np.asarray(f, dtype=np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    return (order // 3).astype(np.int64), np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n))]).astype(np.int64)


def barycenter(v, f):
    return (v[f[:, 0]] + v[f[:, 1]] + v[f[:, 2]]) / 3.0


def remove_unreferenced(v, f):
    used = np.unique(f)
    imap = -np.ones(len(v), dtype=np.int64)
    imap[used] = np.arange(len(used))
    return v[used], imap[f], imap, used


igl = sys.modules["igl"]
igl.triangle_triangle_adjacency = triangle_triangle_adjacency
igl.vertex_triangle_adjacency = vertex_triangle_adjacency
igl.barycenter = barycenter
igl.remove_unreferenced = remove_unreferenced
try:
    import h5py  # noqa: F401
except ImportError:
    sys.modules["h5py"] = types.ModuleType("h5py")

sys.path.insert(0, REF)
from PatchGeneration.Modules import Mesh as RefMeshModule  # noqa: E402
from PatchGeneration.Modules.Mesh import Mesh, Patch  # noqa: E402
from PatchGeneration.Modules.PatchCollector import PatchCollector  # noqa: E402
from PatchGeneration.Modules.Network.DataUtils import FileDataset  # noqa: E402


def icosphere(levels):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
         [8, 6, 7], [9, 8, 1]]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(levels):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.array(v), np.array(f, dtype=np.int64)


def run_reference(v, f, k=4, keep_all=False):
    mesh = Mesh(v.copy(), f.copy())
    mesh.gt = mesh.getFaceNormals()
    log = {"sel": [], "eig": [], "branch": []}
    get_faces, get_rot = Mesh.getFacesInRange, Patch.getPaperRotationMatrix
    get_align, get_translate, get_resize, get_rotate = Patch.alignPatch, Mesh.translate, Mesh.resize, Mesh.rotate
    state = {"rec": None, "depth": 0}                    # alignPatch's own calls of translate / resize (depth 0)

    def align(self):
        state["rec"], state["depth"] = [False, False], 0
        try:
            return get_align(self)
        finally:
            log["branch"].append(tuple(state["rec"]))
            state["rec"] = None

    def translate(self, translation):
        if state["rec"] is not None and state["depth"] == 0:
            state["rec"][0] = True
        return get_translate(self, translation)

    def nested(inner, slot):
        def call(self, arg):
            if slot is not None and state["rec"] is not None and state["depth"] == 0:
                state["rec"][slot] = True
            state["depth"] += 1
            try:
                return inner(self, arg)
            finally:
                state["depth"] -= 1
        return call

    def faces_in_range(self, center, rng):
        out = get_faces(self, center, rng)
        d = np.linalg.norm(self.getVertices() - center, axis=1)
        log["sel"].append((np.array(center), float(rng), np.array(out), float(np.min(np.abs(d - rng)) / rng)))
        return out

    def rotation_matrix(self):
        out = get_rot(self)
        log["eig"].append(np.array(out.eig[0][out.sort]))
        return out

    Mesh.getFacesInRange, Patch.getPaperRotationMatrix = faces_in_range, rotation_matrix
    Patch.alignPatch, Mesh.translate = align, translate
    Mesh.resize, Mesh.rotate = nested(get_resize, 1), nested(get_rotate, None)
    try:
        pc = PatchCollector(mesh, k)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            patches = pc.collectPatches(np.arange(len(f)))
            inputs = np.array([FileDataset.file2input(*p[1].toGraph(), 64) for p in patches])
        seconds = (time.perf_counter() - t0) / len(f)
    finally:
        Mesh.getFacesInRange, Patch.getPaperRotationMatrix = get_faces, get_rot
        Patch.alignPatch, Mesh.translate, Mesh.resize, Mesh.rotate = get_align, get_translate, get_resize, get_rotate
    assert len(log["branch"]) == len(f)
    rot = np.array([p[1].lastRotationApplied for p in patches])
    pi = np.array([int(np.asarray(p[1].pi).reshape(-1)[0]) for p in patches], dtype=np.int64)
    eig = np.array(log["eig"])
    gap = np.minimum(eig[:, 0] - eig[:, 1], eig[:, 1] - eig[:, 2]) / eig[:, 0]
    margin = np.array([s[3] for s in log["sel"]])
    rows = [s[2].astype(np.int64) for s in log["sel"]]
    assert margin.min() >= 1e-8, margin.min()
    assert gap.min() >= 1e-5, gap.min()
    assert not np.isnan(inputs).any() and not np.isnan(rot).any()
    keep = np.union1d(np.arange(0, len(f), 1 if keep_all else 3), np.nonzero(pi >= 64)[0]).astype(np.int64)
    return {"v": v, "f": f, "k": np.int64(k), "r": np.array([s[1] for s in log["sel"]]),
            "centre": np.array([s[0] for s in log["sel"]]),
            "off": np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64),
            "faces": np.concatenate(rows), "rot": rot, "pi": pi, "eig": eig, "relgap": gap, "margin": margin,
            "input_faces": keep, "inputs": inputs[keep], "seconds_per_patch": np.float64(seconds),
            "translated": np.array([b[0] for b in log["branch"]]), "scaled": np.array([b[1] for b in log["branch"]])}


def write_align():
    out = {}
    for name in patch_cases.BOXES:
        v, f = patch_cases.box_variant(name)
        g = run_reference(v, f, keep_all=True)
        g.pop("seconds_per_patch")
        assert np.array_equal(np.diff(g["off"]), np.full(len(f), len(f))) and len(g["inputs"]) == len(f)
        print(f"align/{name}: margin {g['margin'].min():.2e}, gap {g['relgap'].min():.2e}, "
              f"translated {int(g['translated'].sum())}, scaled {int(g['scaled'].sum())} of {len(f)}")
        out.update({f"{name}/{key}": val for key, val in g.items()})
    np.savez_compressed(os.path.join(HERE, "patch_align.npz"), **out)


def main(names=("ellipsoid", "shells", "align")):
    rng = np.random.default_rng(3)
    v0, f0 = icosphere(2)
    assert v0.shape == (162, 3) and f0.shape == (320, 3)
    ell = v0 * np.array([1.0, 0.7, 0.45]) + rng.normal(0.0, 0.02, v0.shape)
    sh = np.concatenate([v0, 1.12 * v0]) + rng.normal(0.0, 0.02, (2 * len(v0), 3))
    fsh = np.concatenate([f0, f0 + len(v0)])
    for name, v, f in (("ellipsoid", ell, f0), ("shells", sh, fsh)):
        if name not in names:
            continue
        g = run_reference(v, f)
        del g["translated"], g["scaled"]
        sizes = np.diff(g["off"])
        print(f"{name}: {len(f)} faces, patches {sizes.min()}-{sizes.max()} faces, margin {g['margin'].min():.2e}, "
              f"gap {g['relgap'].min():.2e}, centres beyond the window {int((g['pi'] >= 64).sum())}, "
              f"{len(g['input_faces'])} inputs stored, {g['seconds_per_patch'] * 1e3:.2f} ms/patch")
        inputs = g.pop("inputs")
        if name == "shells":                           # its inputs in three parts (rows of input_faces in order)
            np.savez_compressed(os.path.join(HERE, f"patch_{name}.npz"), **g)
            for part, rows in enumerate(np.array_split(np.arange(len(inputs)), 3)):
                np.savez_compressed(os.path.join(HERE, f"patch_{name}_inputs_{part}.npz"), inputs=inputs[rows])
        else:
            np.savez_compressed(os.path.join(HERE, f"patch_{name}.npz"), inputs=inputs, **g)
    if "align" in names:
        write_align()
    for fn in os.listdir(HERE):
        if fn.startswith("patch_") and fn.endswith(".npz"):
            assert os.path.getsize(os.path.join(HERE, fn)) < 1 << 20, fn


if __name__ == "__main__":
    main(tuple(sys.argv[1:]) or ("ellipsoid", "shells", "align"))
