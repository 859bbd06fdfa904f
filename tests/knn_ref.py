"""Brute-force references for the neighbour searches, and the hard geometries they are checked on (numpy only).

* d2_f32 / knn_f32   the search kernels' own arithmetic restated in float32: dist2 = ((dx*dx) + (dy*dy)) + (dz*dz), every
                     step rounded, and the order contract ascending (d2, tie) -- tie is the original index, or the rank
                     in a grid's spatial order (the inverse of Grid.perm()).  A kernel must match it bit for bit.
* admissible_f64     the float64 judge of ANY fp32 evaluation of the distances: independent of the restatement.
* radius_f64         the radius selection: float64 ((dx^2 + dy^2) + dz^2) <= r^2 on the exactly converted fp32 inputs.
* CASES              named (snapshot, queries) generators: translated, degenerate, clustered, tied and tiny clouds.
"""
import numpy as np

U = 2.0 ** -24                       # unit roundoff of float32
ADMISSIBLE = 1.0 + 11.0 * U          # (1 + 5u) / (1 - 5u) < 1 + 11u: five roundings in dist2, each side
CHUNK = 1024                         # query rows per block: a [CHUNK, n] matrix at n = 5000 is 20 MB in float32


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def d2_f32(q, pts):
    """dist2 of the kernels in float32: [nq, n].  Subtract, three products, two sums, each rounded to float32, summed
    as ((xx + yy) + zz).  (numpy rounds every elementwise operation to the array type: no fused multiply-add.)"""
    q, pts = _f32(q), _f32(pts)
    out = np.empty((len(q), len(pts)), np.float32)
    for s in range(0, len(q), CHUNK):
        c = q[s:s + CHUNK]
        dx = c[:, None, 0] - pts[None, :, 0]
        dy = c[:, None, 1] - pts[None, :, 1]
        dz = c[:, None, 2] - pts[None, :, 2]
        out[s:s + CHUNK] = ((dx * dx) + (dy * dy)) + (dz * dz)
    return out


def knn_f32(q, pts, k, tie, exclude_self=False):
    """(idx int64 [nq, k], d2 float32 [nq, k]): the k snapshot points of smallest (d2_f32, tie[j]) per query, in that
    order.  exclude_self: query i is snapshot point i; entry i is dropped from the k + 1 best (and the last of them
    when i is not among them: k + 1 or more exact duplicates of smaller tie), as the kernel does."""
    q, pts = _f32(q), _f32(pts)
    n = len(pts)
    tie = np.asarray(tie).astype(np.uint64)
    assert tie.shape == (n,)
    kk = k + 1 if exclude_self else k
    assert 1 <= kk <= n
    idx = np.empty((len(q), k), np.int64)
    d2o = np.empty((len(q), k), np.float32)
    for s in range(0, len(q), CHUNK):
        d2 = d2_f32(q[s:s + CHUNK], pts)
        # d2 >= +0: the float's bit pattern orders like the float; the keys are distinct (tie is a permutation)
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | tie[None, :]
        part = np.argpartition(key, kk - 1, axis=1)[:, :kk] if kk < n else np.tile(np.arange(n), (len(d2), 1))
        order = np.argsort(np.take_along_axis(key, part, 1), axis=1)
        best = np.take_along_axis(part, order, 1)
        if exclude_self:
            rows = np.arange(s, s + len(d2))[:, None]
            keep = np.argsort(best == rows, axis=1, kind="stable")[:, :k]   # the entries that are not i, in order
            best = np.take_along_axis(best, keep, 1)
        idx[s:s + CHUNK] = best
        d2o[s:s + CHUNK] = np.take_along_axis(d2, best, 1)
    return idx, d2o


def d2_f64(q, pts):
    """((dx^2 + dy^2) + dz^2) in float64 on the float32 inputs converted exactly: [nq, n]."""
    q, pts = _f32(q).astype(np.float64), _f32(pts).astype(np.float64)
    dx = q[:, None, 0] - pts[None, :, 0]
    dy = q[:, None, 1] - pts[None, :, 1]
    dz = q[:, None, 2] - pts[None, :, 2]
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def sorted_d2_f64(q, pts, kmax):
    """The kmax smallest float64 distances of every query, ascending: [nq, kmax] (shared by admissible_f64 calls)."""
    q, pts = _f32(q), _f32(pts)
    kmax = min(kmax, len(pts))
    out = np.empty((len(q), kmax), np.float64)
    for s in range(0, len(q), CHUNK):
        d = d2_f64(q[s:s + CHUNK], pts)
        out[s:s + CHUNK] = np.sort(np.partition(d, kmax - 1, axis=1)[:, :kmax] if kmax < len(pts) else d, axis=1)
    return out


def admissible_f64(q, pts, idx, sorted_d64=None):
    """bool [nq]: row i of idx [nq, k] is an admissible k-NN list of query i -- its entries are distinct, in range, and
    every one satisfies d64[j] <= d64_kth * (1 + 11u), d64_kth the true k-th smallest float64 distance.  Each of the
    five roundings of an fp32 dist2 contributes at most u, so d32 lies in d64 * (1 +- 5u) to first order; a returned
    key is <= the true k-th key; (1 + 5u) / (1 - 5u) < 1 + 11u.  sorted_d64: sorted_d2_f64(q, pts, >= k), computed
    once by a caller that judges many lists of the same queries."""
    q, pts, idx = _f32(q), _f32(pts), np.asarray(idx).astype(np.int64)
    n, k = len(pts), idx.shape[1]
    ok = ((idx >= 0) & (idx < n)).all(1)
    srt = np.sort(idx, 1)
    ok &= (srt[:, 1:] != srt[:, :-1]).all(1)
    if sorted_d64 is None:
        sorted_d64 = sorted_d2_f64(q, pts, k)
    kth = sorted_d64[:, k - 1]
    d = q.astype(np.float64)[:, None, :] - pts.astype(np.float64)[np.clip(idx, 0, n - 1)]
    got = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
    return ok & (got <= kth[:, None] * ADMISSIBLE).all(1)


def radius_f64(q, pts, radii):
    """(slices int64 [nq + 1], members int64): the snapshot points with float64 ((dx^2 + dy^2) + dz^2) <= r^2, r the
    float32 radius converted exactly, per query in ascending original index.  r < 0 or NaN: nobody; r = +inf: everyone."""
    q, pts = _f32(q), _f32(pts)
    r = _f32(radii).astype(np.float64)
    assert r.shape == (len(q),)
    r2 = r * r
    counts = np.zeros(len(q), np.int64)
    members = []
    for s in range(0, len(q), CHUNK):
        inside = (d2_f64(q[s:s + CHUNK], pts) <= r2[s:s + CHUNK, None]) & (r[s:s + CHUNK, None] >= 0.0)
        counts[s:s + CHUNK] = inside.sum(1)
        members.append(np.nonzero(inside)[1])              # row-major: ascending index within each query
    slices = np.zeros(len(q) + 1, np.int64)
    np.cumsum(counts, out=slices[1:])
    return slices, np.concatenate(members).astype(np.int64) if members else np.zeros(0, np.int64)


def inverse_perm(perm):
    """tie for rank order: inverse_perm(Grid.perm())[j] = rank of snapshot point j in the grid's spatial order."""
    perm = np.asarray(perm).astype(np.int64)
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    return inv


# ----------------------------------------------------------------------------------------------------------- cases
def _rng(name):
    return np.random.default_rng([int(b) for b in name.encode()])


def _cube(rng, n=4000):
    return rng.random((n, 3)).astype(np.float32)


def _with(snap, *extras):
    snap = _f32(snap)
    return snap, np.concatenate([snap] + [_f32(e) for e in extras])


def uniform_cube():
    return _with(_cube(_rng("uniform_cube")))


def translated():
    """The cube at +32768 on every axis (ulp 2^-8): lattice coordinates o + c h round at ulp(offset)."""
    snap = _cube(_rng("uniform_cube")) + np.float32(32768.0)
    jit = _rng("translated").integers(-2, 3, snap.shape).astype(np.float32) * np.float32(2.0 ** -8)
    return _with(snap, snap + jit)


def translated_mixed():
    return _with(_cube(_rng("translated_mixed")) + np.array([-4096.0, 0.5, 1e5], np.float32))


def sheet():
    rng = _rng("sheet")
    snap = _cube(rng) * np.array([1.0, 1.0, 1e-3], np.float32)
    above = np.concatenate([rng.random((64, 2)), rng.uniform(0.05, 0.6, (64, 1)) + 1e-3], 1)
    return _with(snap, above)


def line():
    rng = _rng("line")
    snap = np.zeros((3000, 3), np.float32)
    snap[:, 0] = np.cumsum(rng.exponential(1.0, 3000) ** 2)   # irregular: gaps over several orders of magnitude
    return _with(rng.permutation(snap))


def plane_exact():
    snap = _cube(_rng("plane_exact"))
    snap[:, 2] = 0.0
    return _with(snap)


def point():
    rng = _rng("point")
    p = np.array([0.3, -1.2, 2.5], np.float32)
    dirs = np.concatenate([np.eye(3), -np.eye(3), rng.normal(size=(10, 3))])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return _with(np.tile(p, (300, 1)), p + dirs)


def single():
    rng = _rng("single")
    return _with(np.array([[1.5, -2.0, 0.25]], np.float32), rng.normal(size=(5, 3)))


def needle():
    return _with(_cube(_rng("needle")) * np.array([1e3, 1.0, 1e-3], np.float32))


def two_clusters():
    """Two clusters of extent 1e-3, 1e4 apart (the far one sits at ulp 2^-10 ~ its own extent: it collapses onto a few
    float32 points, 2000 near-duplicates), queries in the void between them and far outside."""
    rng = _rng("two_clusters")
    a = _cube(rng, 2000) * np.float32(1e-3)
    b = _cube(rng, 2000) * np.float32(1e-3) + np.array([1e4, 0.0, 0.0], np.float32)
    t = rng.random((32, 1))
    between = t * np.array([[1e4, 0.0, 0.0]]) + rng.normal(0, 1e-3, (32, 3))
    outside = rng.normal(size=(8, 3))
    outside = outside / np.linalg.norm(outside, axis=1, keepdims=True) * rng.uniform(3e4, 3e5, (8, 1))
    return _with(rng.permutation(np.concatenate([a, b])), between, outside)


def lattice_ties():
    g = np.stack(np.meshgrid(*[np.arange(12, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return _with(np.concatenate([g, g[:100]]))


def tiny_values():
    return _with(_cube(_rng("tiny_values")) * np.float32(1e-18))


CASES = {f.__name__: f for f in (uniform_cube, translated, translated_mixed, sheet, line, plane_exact, point, single,
                                 needle, two_clusters, lattice_ties, tiny_values)}
