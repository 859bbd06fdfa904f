"""numpy restatement of the reference's network-input pipeline, pinned by tests/golden/patch_*.npz.

PatchGeneration/Modules/Mesh.py (selectPaperPatch :300-307, getFacesInRange :157-163, createPatch :289-295,
Patch.alignPatch :473-482, Patch.toGraph :497-506), RotationMatrix.py:9-35 and Network/DataUtils.py file2input
:41-70, statement for statement in fp64, with this project's three decisions:
  * absent edge-neighbours (-1) are skipped in the two-ring instead of indexing the last face,
  * an edge shared by more than two faces is no adjacency,
  * the middle axis is canonical: row 1's largest-magnitude component is positive, row 2 = row 0 x row 1,
  * an empty patch (the reference fails on one) is the identity rotation over 64 rows of padding, pi = -1,
  * with skip_degenerate, a face without a finite normal adds nothing to the alignment tensor.
Test infrastructure only: the device code under test shares nothing with this file.
"""
import numpy as np

ROWS = 64


def tta(f):
    """igl.triangle_triangle_adjacency(f)[0]: slot e = the face across (f[e], f[(e+1)%3]), -1 when there is none."""
    f = np.asarray(f, dtype=np.int64)
    nf = len(f)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo * (int(f.max()) + 1 if nf else 1) + hi
    order = np.argsort(key, kind="stable")
    _, start, cnt = np.unique(key[order], return_index=True, return_counts=True)
    two = start[cnt == 2]
    c0, c1 = order[two], order[two + 1]
    ok = (c0 // 3 != c1 // 3) & (lo[c0] != hi[c0])
    out = -np.ones(3 * nf, dtype=np.int64)
    out[c0[ok]] = c1[ok] // 3
    out[c1[ok]] = c0[ok] // 3
    return out.reshape(nf, 3)


def areas(v, f, faces):
    t = v[f[np.asarray(faces, dtype=np.int64)]]
    return 0.5 * np.linalg.norm(np.cross(t[..., 1, :] - t[..., 0, :], t[..., 2, :] - t[..., 0, :], axis=-1), axis=-1)


def face_normals(v, f):
    fv = v[f]
    cr = np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return cr / np.linalg.norm(cr, axis=1)[:, None]


def two_ring(f2f, fi):
    res = np.array([fi], dtype=np.int64)
    for _ in range(2):
        nb = f2f[res].reshape(-1)
        res = np.union1d(res, nb[nb >= 0])
    return res


def radius_centre(v, f, f2f, fis, k=4):
    """(centre [n,3], r [n]) of selectPaperPatch for every face of fis."""
    centre = np.empty((len(fis), 3))
    r = np.empty(len(fis))
    for i, fi in enumerate(fis):
        nh = two_ring(f2f, int(fi))
        r[i] = k * (np.sum(areas(v, f, nh)) / nh.shape[0]) ** 0.5
        centre[i] = np.average(v[f[fi]], axis=0)
    return centre, r


def select(v, f, centre, r):
    """The faces with a vertex strictly inside the ball, ascending (getFacesInRange)."""
    vm = np.linalg.norm(v - centre, axis=1) < r
    return np.nonzero(vm[f].any(axis=1))[0]


def rotation(pv, pf, pi, skip_degenerate=False):
    """RotationMatrix.__init__ on the centred, scaled patch; returns (matrix, eigenvalues descending).  With
    skip_degenerate a face whose normal is not finite is left out of the sum for T and of max(ar)."""
    bcs = (pv[pf[:, 0]] + pv[pf[:, 1]] + pv[pf[:, 2]]) / 3.0
    fn = face_normals(pv, pf)
    dcs = np.delete(bcs, pi, axis=0) - bcs[pi]
    nj = np.delete(fn, pi, axis=0)
    raw = np.cross(np.cross(dcs, nj, axis=1), dcs)
    with np.errstate(invalid="ignore", divide="ignore"):
        wj = np.nan_to_num(raw / np.linalg.norm(raw, axis=1, keepdims=True))
    njp = 2 * np.sum(np.multiply(nj, wj), axis=1)[:, None] * wj - nj
    ar = areas(pv, pf, np.delete(np.arange(len(pf)), pi, axis=0))
    if skip_degenerate:
        ok = np.isfinite(nj).all(axis=1)
        dcs, njp, ar = dcs[ok], njp[ok], ar[ok]
    muj = (ar / np.max(ar)) * np.exp(-np.linalg.norm(dcs, axis=1) / (1. / 3.))
    T = np.sum(muj[:, None, None] * (njp[..., None] * njp[:, None]), axis=0)
    w, V = np.linalg.eigh(T)
    order = np.flip(np.argsort(w))
    m = V.T[order].copy()
    if np.sum(m[0] * fn[pi]) < 0:
        m[0] *= -1
    if m[1, np.argmax(np.abs(m[1]))] < 0:            # this project's canonical middle axis
        m[1] *= -1
    m[2] = np.cross(m[0], m[1])
    return m, w[order]


def patch_input(v, f, fi, faces, neighbours="reference", skip_degenerate=False):
    """One patch: (inputs [64,20], rotation [3,3], pi, eigenvalues [3]); faces = select(...) of face fi."""
    if len(faces) == 0:
        out = np.zeros((ROWS, 20))
        out[:, 17:] = ROWS - 1
        return out, np.eye(3), -1, np.zeros(3)
    sub = f[faces]
    used = np.unique(sub)
    pv = np.array(v[used], dtype=np.float64)
    pf = np.searchsorted(used, sub)
    hit = np.nonzero(faces == fi)[0]
    pi = int(hit[0]) if len(hit) else -1
    # Patch.alignPatch
    n = pv.shape[0]
    center = np.sum(pv, axis=0) / n
    size = np.max(np.linalg.norm(pv - center, axis=1))
    if not np.allclose(np.linalg.norm(center), 0):
        pv += -center
    if not np.allclose(size, 1):                      # Mesh.resize(1)
        c = np.sum(pv, axis=0) / n
        pv += -c
        pv *= 1 / np.max(np.linalg.norm(pv, axis=1))
        pv += c
    R, w = rotation(pv, pf, pi, skip_degenerate)
    c = np.sum(pv, axis=0) / n                       # Mesh.rotate
    pv += -c
    pv = np.dot(R, pv.T).T
    pv += c
    # Patch.toGraph
    E = tta(pf)
    fea = np.concatenate(((pv[pf[:, 0]] + pv[pf[:, 1]] + pv[pf[:, 2]]) / 3.0, face_normals(pv, pf),
                          areas(pv, pf, np.arange(len(pf))).reshape(-1, 1), (E != -1).sum(axis=1).reshape(-1, 1),
                          pv[pf].reshape(-1, 9)), axis=1)
    # FileDataset.file2input with the [m, 3] adjacency it is handed
    m = len(pf)
    out = np.zeros((ROWS, 20))
    out[:min(m, ROWS), :17] = fea[:ROWS]
    out[:, 17:] = index_columns(E, neighbours)
    return out, R, pi, w


def index_columns(E, neighbours="reference"):
    """file2input's three index columns [64, 3] for a patch's local edge adjacency E [m, 3]."""
    out = np.full((ROWS, 3), ROWS - 1.0)
    for i in range(min(len(E), ROWS)):
        if neighbours == "reference":
            idx = [e for e in range(3) if E[i, e] == 1]
        else:
            idx = [int(E[i, e]) for e in range(3) if 0 <= E[i, e] < ROWS] or [i]
        if idx:
            out[i] = (idx + [idx[-1]] * 2)[:3]
    return out


def network_input(v, f, fis, k=4, neighbours="reference", skip_degenerate=False):
    """Everything for the faces fis: a dict of r, centre, the CSR (off, faces), inputs, rotations, pi, eig."""
    v = np.asarray(v, dtype=np.float64)
    f = np.asarray(f, dtype=np.int64)
    fis = np.asarray(fis, dtype=np.int64)
    centre, r = radius_centre(v, f, tta(f), fis, k)
    rows = [select(v, f, centre[i], r[i]) for i in range(len(fis))]
    res = [patch_input(v, f, int(fi), rows[i], neighbours, skip_degenerate) for i, fi in enumerate(fis)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return {"r": r, "centre": centre, "off": off,
            "faces": np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64),
            "inputs": np.array([x[0] for x in res]).reshape(-1, ROWS, 20),
            "rot": np.array([x[1] for x in res]).reshape(-1, 3, 3),
            "pi": np.array([x[2] for x in res], dtype=np.int64),
            "eig": np.array([x[3] for x in res]).reshape(-1, 3)}


def sign_align(rot, ref_rot):
    """The per-patch sign s = +-1 that maps ref_rot's rows 1 and 2 onto rot's (the middle axis is free in eigh)."""
    s = np.sign(np.sum(rot[:, 1] * ref_rot[:, 1], axis=1))
    return np.where(s == 0, 1.0, s)


def apply_sign(inputs, rot, s, centre=None):
    """inputs [n,64,20] and rot [n,3,3] with the y and z of every coordinate and normal, and rows 1, 2, times s.
    centre [n,3]: the point each patch was rotated about and kept (kept_centres), which the flip leaves in place; the
    rows of padding stay zero."""
    inputs, rot = np.array(inputs, dtype=np.float64), np.array(rot, dtype=np.float64)
    cols = [1, 2, 4, 5, 9, 10, 12, 13, 15, 16]
    if centre is not None:
        real = inputs[:, :, 6:17].any(axis=2)[:, :, None]
        shift = np.where(real, np.tile(np.asarray(centre)[:, 1:], 4)[:, None, :], 0.0)
        pos = [1, 2, 9, 10, 12, 13, 15, 16]
        inputs[:, :, pos] -= shift
    inputs[:, :, cols] *= s[:, None, None]
    if centre is not None:
        inputs[:, :, pos] += shift
    rot[:, 1:] *= s[:, None, None]
    return inputs, rot


def kept_centres(v, f, off, faces):
    """Per patch the vertex mean c where Patch.alignPatch does not translate (|c| <= 1e-8: the patch is resized and
    rotated about c and stays there), else 0 (an empty patch: 0)."""
    out = np.zeros((len(off) - 1, 3))
    for i in range(len(off) - 1):
        if off[i + 1] > off[i]:
            c = v[np.unique(f[faces[off[i]:off[i + 1]]])].mean(axis=0)
            if np.allclose(np.linalg.norm(c), 0):
                out[i] = c
    return out


def deviations(inputs, rot, want_inputs, want_rot, centre=None):
    """Per patch the largest absolute deviation of (the rotation, the feature columns 0-16) from the wanted ones, once
    the wanted ones carry the sign of the middle axis that sign_align finds."""
    wi, wr = apply_sign(want_inputs, want_rot, sign_align(rot, want_rot), centre)
    return (np.abs(rot - wr).max(axis=(1, 2)),
            np.abs(np.asarray(inputs, dtype=np.float64)[:, :, :17] - wi[:, :, :17]).max(axis=(1, 2)))


def relgap(eig):
    """min adjacent eigenvalue gap / largest eigenvalue, per patch."""
    e = np.asarray(eig)
    with np.errstate(invalid="ignore"):                  # (an empty patch has no eigenvalues: NaN)
        return np.minimum(e[:, 0] - e[:, 1], e[:, 1] - e[:, 2]) / e[:, 0]
