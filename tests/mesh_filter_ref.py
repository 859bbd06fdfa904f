"""A plain numpy restatement of the reference's guided bilateral mesh normal filtering
(src/GCNDenoiser/GCNDenoiser/MeshNormalFiltering.cpp:47-244, MeshDenoisingBase.cpp:24-143), the yardstick of
test_mesh_filter_ref.py (known answers, CPU) and test_gpu_mesh_filter.py (the HIP kernels), and the small meshes both
use.  Every function works in the dtype of the vertices it is given (float64: the parity yardstick; float32: the
measure of what fp32 arithmetic costs); the neighbourhoods and the mean-distance sums are always float64."""
import math

import numpy as np


# ------------------------------------------------------------------------------------------------ restatement
def vta(f, nv):
    """igl.vertex_triangle_adjacency: (VF, NI), every vertex's incident faces in face order (one entry per corner)."""
    flat = np.asarray(f, np.int64).reshape(-1)
    vf = np.argsort(flat, kind="stable") // 3
    ni = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=nv))]).astype(np.int64)
    return vf.astype(np.int64), ni


def _len(d):
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def face_geometry(v, f):
    """centroid ((p0 + p1) + p2) / 3, area 0.5 |(p1 - p0) x (p2 - p1)| (= the reference's 0.5 |(p1 - p0) x (p1 - p2)|:
    the second edge is negated exactly), unit normal of the same cross product, zero for a face of zero area."""
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    c = ((p0 + p1) + p2) / v.dtype.type(3)
    u, w = p1 - p0, p2 - p1
    r = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                  u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    ln = _len(r)
    ok = (ln > 0) & np.isfinite(ln)
    n = np.where(ok[:, None], r / np.where(ok, ln, 1)[:, None], 0).astype(v.dtype)
    return c, v.dtype.type(0.5) * ln, n


def mean_adjacent_distance(c, f, vf, ni):
    """Mean |c_g - c_i| over the ordered pairs (i, g) of faces sharing an edge (getRadius / getSigmaS with multiple 1,
    MeshNormalFiltering.cpp:134-168): for every edge (a, b) of face i, every other face in a's row that holds b.
    Returns (mean, pairs); the distances are in c's dtype, their sum in float64."""
    nf = len(f)
    total, pairs = 0.0, 0
    for e in range(3):
        a, b = f[:, e], f[:, (e + 1) % 3]
        deg = ni[a + 1] - ni[a]
        i = np.repeat(np.arange(nf), deg)
        pos = np.arange(deg.sum()) - np.repeat(np.cumsum(deg) - deg, deg) + np.repeat(ni[a], deg)
        g = vf[pos]
        keep = (g != i) & (f[g] == np.repeat(b, deg)[:, None]).any(1)
        total += float(_len(c[g[keep]] - c[i[keep]]).astype(np.float64).sum())
        pairs += int(keep.sum())
    return (total / pairs if pairs else 0.0), pairs


def vertex_neighbours(f, vf, ni):
    """Per face, the faces sharing a vertex with it (itself included), ascending: the vertex-based neighbourhood."""
    return [sorted({int(h) for vtx in f[i] for h in vf[ni[vtx]:ni[vtx + 1]]}) for i in range(len(f))]


def neighbourhoods(c, f, vf, ni, mode="radius", radius=0.0, rows=None):
    """The CSR (offsets, faces) of the face neighbourhoods, rows ascending, centre included.  radius: the literal
    breadth-first search of getRadiusBasedFaceNeighbor (MeshNormalFiltering.cpp:47-78) over vertex-sharing steps,
    stepping only onto faces within `radius` of the centre's centroid; vertex: the faces sharing a vertex.
    rows: only these faces' rows (offsets then index into `rows`)."""
    vn = vertex_neighbours(f, vf, ni)
    cl = np.asarray(c, np.float64).tolist()
    out = []
    for i in (range(len(f)) if rows is None else rows):
        i = int(i)
        if mode == "vertex":
            out.append(vn[i])
            continue
        ci = cl[i]
        flag = {i}
        queue = [i]
        head = 0
        while head < len(queue):
            for h in vn[queue[head]]:
                if h not in flag:
                    ch = cl[h]
                    dx, dy, dz = ci[0] - ch[0], ci[1] - ch[1], ci[2] - ch[2]
                    if math.sqrt((dx * dx + dy * dy) + dz * dz) <= radius:
                        queue.append(h)
                    flag.add(h)
            head += 1
        out.append(sorted(queue))
    off = np.concatenate([[0], np.cumsum([len(r) for r in out])]).astype(np.int64)
    return off, np.array([x for r in out for x in r], np.int64)


def euclidean_ball(c, i, radius):
    return np.nonzero(_len(c - c[i]) <= radius)[0]


def filter_pass(c, area, g, src, off, nbr, sigma_r, sigma_s):
    """One pass (MeshNormalFiltering.cpp:207-236): s_i = sum_j src_j A_j exp(-|c_i-c_j|^2 / 2 sigma_s^2)
    exp(-|g_i-g_j|^2 / 2 sigma_r^2), out = s / |s|; |s| zero or not finite keeps src_i; a neighbour of zero area weighs
    0 and is not read; a centre of zero area gets the zero normal."""
    t = c.dtype.type
    i = np.repeat(np.arange(len(c)), np.diff(off))
    j = nbr
    ds, dr = t(2) * (t(sigma_s) * t(sigma_s)), t(2) * (t(sigma_r) * t(sigma_r))
    with np.errstate(all="ignore"):
        d, e = c[i] - c[j], g[i] - g[j]
        ws = np.exp(-(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) / ds))
        wr = np.exp(-(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) / dr))
        valid = area[j] > 0
        w = np.where(valid, (area[j] * ws) * wr, 0).astype(c.dtype)
        s = np.add.reduceat(np.where(valid[:, None], src[j], 0).astype(c.dtype) * w[:, None], off[:-1], axis=0)
        ln = _len(s)
        ok = (ln > 0) & np.isfinite(ln)
        out = np.where(ok[:, None], s / np.where(ok, ln, 1)[:, None], src).astype(c.dtype)
    out[~(area > 0)] = 0
    return out


def update_vertices(v, f, n, vf, ni, k, keep_isolated=True):
    """k Jacobi sweeps of v_i += sum_{f∋i} sum_{c∈f} n_f (n_f · (v_c − v_i)) / (3 deg_i) (Mesh.updateVertices,
    Mesh.py:377-418).  A vertex in no face keeps its position (keep_isolated) or becomes NaN, as updateVertices does."""
    deg = ni[1:] - ni[:-1]
    has = np.nonzero(deg > 0)[0]
    own = np.repeat(np.arange(len(v)), deg)
    nn = n[vf]
    v = v.copy()
    for _ in range(k):
        acc = np.zeros((len(has), 3), v.dtype)
        for corner in range(3):
            d = v[f[vf, corner]] - v[own]
            dot = (nn[:, 0] * d[:, 0] + nn[:, 1] * d[:, 1]) + nn[:, 2] * d[:, 2]
            acc = acc + np.add.reduceat(dot[:, None] * nn, ni[has], axis=0)
        new = v.copy() if keep_isolated else np.full_like(v, np.nan)
        new[has] = v[has] + acc / (v.dtype.type(3) * deg[has].astype(v.dtype))[:, None]
        v = new
    return v


def default_neighbourhoods(v, f, mode="radius", multiple_radius=2, radius=None):
    """(offsets, faces, radius) on the mesh (v, f), always in float64."""
    v = np.asarray(v, np.float64)
    vf, ni = vta(f, len(v))
    c = face_geometry(v, f)[0]
    if mode == "radius" and radius is None:
        radius = multiple_radius * mean_adjacent_distance(c, f, vf, ni)[0]
    off, nbr = neighbourhoods(c, f, vf, ni, mode, radius)
    return off, nbr, radius


def denoise(v, f, guided=None, normal_iterations=12, vertex_iterations=16, sigma_r=0.3, multiple_radius=2,
            multiple_sigma_s=1, mode="radius", csr=None):
    """The loop of updateFilteredNormalsWithPredictedNormal (MeshNormalFiltering.cpp:170-244) in v's dtype:
    returns (vertices, last filtered normals).  csr: the neighbourhoods (offsets, faces) when already known."""
    vf, ni = vta(f, len(v))
    off, nbr = csr if csr is not None else default_neighbourhoods(v, f, mode, multiple_radius)[:2]
    v = v.copy()
    g = None if guided is None else np.asarray(guided, v.dtype)
    out = None
    for it in range(normal_iterations):
        c, area, cur = face_geometry(v, f)
        if g is None:
            g = cur
        sigma_s = multiple_sigma_s * mean_adjacent_distance(c, f, vf, ni)[0]
        out = filter_pass(c, area, g, g if it == 0 else cur, off, nbr, sigma_r, sigma_s)
        v = update_vertices(v, f, out, vf, ni, vertex_iterations)
    return v, out


def mean_angle_deg(n, ref, rows=None):
    d = np.clip((n * ref).sum(1), -1, 1)
    return float(np.degrees(np.arccos(d if rows is None else d[rows])).mean())


# ------------------------------------------------------------------------------------------------ meshes
def grid(nx, ny, noise=0.0, seed=0, z=0.0, x0=0.0):
    """nx x ny vertices on the unit lattice in the plane z, every cell split by its (0,0)-(1,1) diagonal:
    2 (nx-1)(ny-1) faces with normal +z.  noise: uniform in [-noise, noise]^3."""
    xs, ys = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    v = np.stack([xs.ravel() + x0, ys.ravel(), np.full(nx * ny, z)], axis=1)
    vid = lambda i, j: i * ny + j
    faces = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            faces.append((vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)))
            faces.append((vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)))
    if noise:
        v = v + np.random.default_rng(seed).uniform(-noise, noise, v.shape)
    return v, np.array(faces, np.int64)


def cube(n=8, noise=0.0, seed=0):
    """The closed surface of the cube [0, n]^3, n x n cells a side, 12 n^2 faces, normals outwards.
    Returns (v, f, clean v)."""
    ids, verts, faces = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(verts)
            verts.append(p)
        return ids[p]

    for axis in range(3):
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def pt(a, b):
                        q = [0, 0, 0]
                        q[axis], q[(axis + 1) % 3], q[(axis + 2) % 3] = side, a, b
                        return tuple(q)
                    quad = [vid(pt(i, j)), vid(pt(i + 1, j)), vid(pt(i + 1, j + 1)), vid(pt(i, j + 1))]
                    if side == 0:
                        quad.reverse()
                    faces.append((quad[0], quad[1], quad[2]))
                    faces.append((quad[0], quad[2], quad[3]))
    clean = np.array(verts, np.float64)
    v = clean + np.random.default_rng(seed).uniform(-noise, noise, clean.shape) if noise else clean.copy()
    return v, np.array(faces, np.int64), clean


def two_sheets(nx=7, ny=6, gap=0.65, noise=0.05, seed=3):
    """Two parallel noisy grids `gap` apart that share no vertex (gap = 0.5 x the default radius of the unit grid,
    2 x 0.654): each face's Euclidean ball reaches the other sheet, its neighbourhood must not.
    Returns (v, f, sheet id per face)."""
    v0, f0 = grid(nx, ny, noise, seed)
    v1, f1 = grid(nx, ny, noise, seed + 1, z=gap)
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)]), np.repeat([0, 1], [len(f0), len(f1)])


def guard_mesh(noise=0.05, seed=5):
    """A noisy 6 x 5 grid plus one face of zero area (a repeated corner) and one vertex in no face.
    Returns (v, f, index of the degenerate face, index of the isolated vertex)."""
    v, f = grid(6, 5, noise, seed)
    f = np.concatenate([f, [[7, 13, 13]]]).astype(np.int64)
    v = np.concatenate([v, [[2.5, 2.5, 1.0]]])
    return v, f, len(f) - 1, len(v) - 1


def mean_edge_length(v, f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    e = np.unique(e[e[:, 0] != e[:, 1]], axis=0)
    return float(np.linalg.norm(v[e[:, 0]] - v[e[:, 1]], axis=1).mean())


def gaussian_noise(v, f, factor=0.2, seed=11):
    """v + N(0, (factor x mean edge length)^2) per coordinate."""
    return v + np.random.default_rng(seed).normal(0.0, factor * mean_edge_length(v, f), v.shape)


def parity_cases():
    """The five small meshes of the device parity tests: name -> (v, f, multiple_radius).  Fixed seeds: no centroid
    distance of any of them lies within 1e-9 (relative) of its radius (test_mesh_filter_ref.py), so a neighbourhood
    cannot flip on the last bits of the radius."""
    sv, sf, _ = two_sheets()
    gv, gf, _, _ = guard_mesh()
    cv, cf, _ = cube(8, 0.1, 2)
    return {
        "open_grid": grid(13, 11, 0.1, 1) + (2,),          # 240 faces: one partial block, boundary edges
        "cube": (cv, cf, 2),                               # 768 faces, closed, sharp edges
        "two_sheets": (sv, sf, 2),                         # unconnected sheets inside each other's balls
        "wide_rows": grid(41, 41, 0.1, 4) + (5,),          # 40 x 40 cells, rows longer than one wave
        "guard": (gv, gf, 2),                              # a zero-area face and an isolated vertex
    }
