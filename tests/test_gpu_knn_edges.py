"""The neighbour searches against brute force on hard geometry (tests/knn_ref.py): pcd_knn for every top-k template
and output variant, the Morton query-order path, the radius selection, rebuilt grids and the fused loop's K1 lists.

Every comparison is exact and runs over every row: lists and d2 against the float32 restatement of dist2 in the
documented (d2, index) -- or (d2, rank) -- order, bit for bit, and the device's lists against the float64 judge
(admissible_f64), which knows nothing of the restatement.  Radius members against float64 brute force.
"""
import functools

import numpy as np
import pytest
import torch

import knn_ref as R
import pcd_native as nat
from Pointcloud.Modules.Object import Pointcloud
from Pointcloud.Modules.Processor import Processor
from conftest import report

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 8, 9, 12, 13, 14, 16, 17, 31, 32, 33, 63, 64)
K_HINTS = (8, 64)
KMAX = 64


def T(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)           # (a copy: the shared references are read-only)


def bits(a):
    """uint32 view of a float32 array (bitwise comparison: -0.0 != +0.0, NaN == NaN)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_lists(got_idx, got_d2, ref_idx, ref_d2, what):
    gi, gd = got_idx.cpu().numpy().astype(np.int64), got_d2.cpu().numpy()
    bad = (gi != ref_idx).any(1) | (bits(gd) != bits(ref_d2)).any(1)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(bad)} rows differ; row {r}: got {gi[r].tolist()} "
                             f"{gd[r].tolist()} want {ref_idx[r].tolist()} {ref_d2[r].tolist()}")


# ------------------------------------------------------------------------------- shared references (computed once)
@functools.lru_cache(maxsize=None)
def case(name):
    snap, q = R.CASES[name]()
    snap.setflags(write=False)
    q.setflags(write=False)
    return snap, q


@functools.lru_cache(maxsize=None)
def ref_by_index(name):
    """The restatement's min(n, 64) nearest of every query in (d2, original index) order: every k is a prefix."""
    snap, q = case(name)
    idx, d2 = R.knn_f32(q, snap, min(KMAX, len(snap)), np.arange(len(snap)))
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


@functools.lru_cache(maxsize=None)
def judge(name):
    snap, q = case(name)
    s = R.sorted_d2_f64(q, snap, KMAX)
    s.setflags(write=False)
    return s


_grids = {}


def grid_for(name, k_hint, dev):
    if (name, k_hint) not in _grids:
        _grids[name, k_hint] = nat.Grid(T(case(name)[0], dev), k_hint=k_hint)
    return _grids[name, k_hint]


_dev_q = {}


def queries(name, dev):
    if name not in _dev_q:
        _dev_q[name] = T(case(name)[1], dev)
    return _dev_q[name]


# ------------------------------------------------------------------------------------- (a) pcd_knn, every template
@pytest.mark.parametrize("name,k", [(name, k) for name in R.CASES for k in KS if k <= len(case(name)[0])])
def test_knn_bitwise_every_template(name, k, gpu):
    """k > n is not a case: pcd_knn refuses it (test_knn_small_clouds asserts the refusal)."""
    snap, q = case(name)
    ref_idx, ref_d2 = ref_by_index(name)
    for k_hint in K_HINTS:
        idx, d2 = grid_for(name, k_hint, gpu).knn(queries(name, gpu), k, with_d2=True)
        ok = R.admissible_f64(q, snap, idx.cpu().numpy(), judge(name))
        assert ok.all(), (name, k, k_hint, int((~ok).sum()), np.nonzero(~ok)[0][:5])
        same_lists(idx, d2, ref_idx[:, :k], ref_d2[:, :k], f"{name} k={k} k_hint={k_hint}")


@pytest.mark.parametrize("n", [1, 2, 5, 13, 14, 33, 64, 65])
def test_knn_small_clouds(n, gpu):
    """n == k, and n == k + 1 with exclude_self (every snapshot point but the row's own); k > n is refused."""
    rng = np.random.default_rng(n)
    snap = rng.normal(size=(n, 3)).astype(np.float32)
    if n >= 5:
        snap[3] = snap[1]                                   # one exact duplicate pair
    q = np.concatenate([snap, rng.normal(size=(7, 3)).astype(np.float32)])
    tie = np.arange(n)
    for k_hint in K_HINTS:
        grid = nat.Grid(T(snap, gpu), k_hint=k_hint)
        k = min(n, KMAX)                                    # n == k (n == k + 1 at n = 65)
        idx, d2 = grid.knn(T(q, gpu), k, with_d2=True)
        assert R.admissible_f64(q, snap, idx.cpu().numpy()).all()
        same_lists(idx, d2, *R.knn_f32(q, snap, k, tie), f"n = {n} k = {k}")
        if n <= KMAX:
            with pytest.raises(ValueError, match="exceeds the number of snapshot points"):
                grid.knn(T(snap, gpu), n, exclude_self=True)
        if n < KMAX:
            with pytest.raises(ValueError, match="exceeds the number of snapshot points"):
                grid.knn(T(q, gpu), n + 1)
        if n >= 2:
            k = min(n, KMAX) - 1                            # n == k + 1 with exclude_self (n == k + 2 at n = 65)
            for bits_ in (64, 32):
                idx, d2 = grid.knn(T(snap, gpu), k, exclude_self=True, with_d2=True, idx_bits=bits_)
                same_lists(idx, d2, *R.knn_f32(snap, snap, k, tie, exclude_self=True), f"n = {n} k = {k} no self")
                assert not (idx.cpu().numpy() == np.arange(n)[:, None]).any()


# ----------------------------------------------------------------------------------------- (b) output variants
VARIANT_CASES = ("uniform_cube", "translated", "lattice_ties")


@pytest.mark.parametrize("k", [3, 13, 32])
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_knn_idx32_and_sorted_ids(name, k, gpu):
    snap, q = case(name)
    n = len(snap)
    for k_hint in K_HINTS:
        grid, dq = grid_for(name, k_hint, gpu), queries(name, gpu)
        i64, d64 = grid.knn(dq, k, with_d2=True)
        i32, d32 = grid.knn(dq, k, with_d2=True, idx_bits=32)
        assert i32.dtype == torch.int32 and torch.equal(i32.long(), i64) and torch.equal(d32, d64)
        perm = grid.perm().cpu().numpy().astype(np.int64)
        assert (np.sort(perm) == np.arange(n)).all()
        ref_idx, ref_d2 = R.knn_f32(q, snap, k, R.inverse_perm(perm))   # ties break by rank
        for bits_ in (64, 32):
            r, d2 = grid.knn(dq, k, with_d2=True, idx_bits=bits_, sorted_ids=True)
            r = r.cpu().numpy().astype(np.int64)
            assert ((r >= 0) & (r < n)).all()
            same_lists(torch.from_numpy(perm[r]), d2, ref_idx, ref_d2, f"{name} sorted_ids k={k} k_hint={k_hint}")


@pytest.mark.parametrize("name", VARIANT_CASES)
def test_knn_exclude_self(name, gpu):
    snap, _ = case(name)
    tie = np.arange(len(snap))
    ds = T(snap, gpu)
    for k_hint in K_HINTS:
        grid = grid_for(name, k_hint, gpu)
        for k in (3, 12, 63):
            ref = R.knn_f32(snap, snap, k, tie, exclude_self=True)
            for bits_ in (64, 32):
                idx, d2 = grid.knn(ds, k, exclude_self=True, with_d2=True, idx_bits=bits_)
                same_lists(idx, d2, *ref, f"{name} exclude_self k={k} idx_bits={bits_} k_hint={k_hint}")
        with pytest.raises(ValueError, match="exceeds pcd_max_k"):
            grid.knn(ds, 64, exclude_self=True)
        with pytest.raises(ValueError, match="exclude_self requires original ids"):
            grid.knn(ds, 3, exclude_self=True, sorted_ids=True)


@pytest.mark.parametrize("name", list(R.CASES))
def test_nn_is_column_zero(name, gpu):
    for k_hint in K_HINTS:
        grid, dq = grid_for(name, k_hint, gpu), queries(name, gpu)
        idx, d2 = grid.knn(dq, 1, with_d2=True)
        nd2, nidx = grid.nn(dq)
        assert torch.equal(nidx, idx[:, 0])
        assert (bits(nd2.cpu().numpy()) == bits(d2[:, 0].cpu().numpy())).all()


# --------------------------------------------------------------------------- (c) the Morton query-order path
NQ_ORDERED = 40000            # >= 32768: one call takes the query-order path; two calls of 20000 do not


@functools.lru_cache(maxsize=None)
def ordered_case(name):
    snap, _ = case(name)
    rng = np.random.default_rng(40000)
    q = snap[rng.integers(0, len(snap), NQ_ORDERED)] + rng.normal(0, 0.05, (NQ_ORDERED, 3)).astype(np.float32)
    q = np.ascontiguousarray(q[rng.permutation(NQ_ORDERED)], dtype=np.float32)
    radii = rng.uniform(0.0, 0.15, NQ_ORDERED).astype(np.float32)
    radii[::97] = 0.0
    radii[5::101] = -1.0
    radii[::4001] = np.inf
    return q, radii, R.knn_f32(q, snap, 32, np.arange(len(snap))), R.radius_f64(q, snap, radii)


@pytest.mark.parametrize("name", ["uniform_cube", "translated"])
def test_query_order_path(name, gpu):
    snap, _ = case(name)
    q, radii, (ref_idx, ref_d2), (ref_sl, ref_m) = ordered_case(name)
    grid = grid_for(name, 8, gpu)
    dq, dr = T(q, gpu), T(radii, gpu)
    half = NQ_ORDERED // 2
    parts = [(dq[:half], dr[:half]), (dq[half:], dr[half:])]
    sorted64 = R.sorted_d2_f64(q, snap, 32)
    for k in (13, 32):
        idx, d2 = grid.knn(dq, k, with_d2=True)
        two = [grid.knn(p, k, with_d2=True) for p, _ in parts]
        assert torch.equal(idx, torch.cat([t[0] for t in two])), k
        assert torch.equal(d2.view(torch.int32), torch.cat([t[1] for t in two]).view(torch.int32)), k
        assert R.admissible_f64(q, snap, idx.cpu().numpy(), sorted64).all()
        same_lists(idx, d2, ref_idx[:, :k], ref_d2[:, :k], f"{name} ordered k={k}")
    nd2, nidx = grid.nn(dq)
    two = [grid.nn(p) for p, _ in parts]
    assert torch.equal(nidx, torch.cat([t[1] for t in two]))
    assert torch.equal(nd2.view(torch.int32), torch.cat([t[0] for t in two]).view(torch.int32))
    assert (nidx.cpu().numpy() == ref_idx[:, 0]).all() and (bits(nd2.cpu().numpy()) == bits(ref_d2[:, 0])).all()
    counts = grid.radius_counts(dq, dr)
    assert torch.equal(counts, torch.cat([grid.radius_counts(p, r) for p, r in parts]))
    assert (counts.cpu().numpy() == np.diff(ref_sl)).all()
    sl, m = grid.radius(dq, dr)
    two = [grid.radius(p, r) for p, r in parts]
    assert torch.equal(m, torch.cat([t[1] for t in two]))
    assert torch.equal(sl, torch.cat([two[0][0], two[1][0][1:] + two[0][0][-1]]))
    assert (sl.cpu().numpy() == ref_sl).all() and (m.cpu().numpy() == ref_m).all()


# ------------------------------------------------------------------------------------------------- (d) radius
def radius_case(name):
    """Per-query radii: one of {0, the restatement's 1st / 8th / 40th neighbour's float64 distance rounded to float32
    (the <= sits exactly on a member), 3 x the bounding-box diagonal, +inf, -1}, and 200 rows with a uniform radius up
    to the largest 40th-neighbour distance."""
    snap, q = case(name)
    n, nq = len(snap), len(q)
    ref_idx, _ = ref_by_index(name)
    rng = np.random.default_rng(sum(name.encode()))
    s64, q64 = snap.astype(np.float64), q.astype(np.float64)
    nbr = np.stack([np.sqrt(((q64 - s64[ref_idx[:, min(c, ref_idx.shape[1] - 1)]]) ** 2).sum(1)) for c in (0, 7, 39)], 1)
    diag = 3.0 * np.linalg.norm(s64.max(0) - s64.min(0))
    table = np.concatenate([np.zeros((nq, 1)), nbr, np.full((nq, 1), diag), np.full((nq, 1), np.inf),
                            np.full((nq, 1), -1.0)], 1)
    radii = table[np.arange(nq), rng.integers(0, table.shape[1], nq)]
    rows = rng.choice(nq, min(200, nq), replace=False)
    radii[rows] = rng.uniform(0.0, nbr[:, 2].max(), len(rows))
    return radii.astype(np.float32)


@pytest.mark.parametrize("name", list(R.CASES))
def test_radius_is_float64_brute_force(name, gpu):
    snap, q = case(name)
    radii = radius_case(name)
    ref_sl, ref_m = R.radius_f64(q, snap, radii)
    for k_hint in K_HINTS:
        grid = grid_for(name, k_hint, gpu)
        counts = grid.radius_counts(queries(name, gpu), T(radii, gpu))
        assert (counts.cpu().numpy() == np.diff(ref_sl)).all(), (name, k_hint)
        sl, m = grid.radius(queries(name, gpu), T(radii, gpu))
        assert (sl.cpu().numpy() == ref_sl).all() and (m.cpu().numpy() == ref_m).all(), (name, k_hint)


# ------------------------------------------------------------------------------------------------ (e) rebuild
@pytest.mark.parametrize("k_hint", [8, 256])
@pytest.mark.parametrize("name", ["translated", "sheet", "two_clusters"])
def test_rebuild_answers_identically(name, k_hint, gpu):
    snap, q = case(name)
    g0 = grid_for(name, 64, gpu)
    g1 = g0.rebuild(k_hint)
    assert (np.sort(g1.perm().cpu().numpy()) == np.arange(len(snap))).all()
    dq = queries(name, gpu)
    ref_idx, ref_d2 = ref_by_index(name)
    for k in (4, 32):
        i0, d0 = g0.knn(dq, k, with_d2=True)
        i1, d1 = g1.knn(dq, k, with_d2=True)
        assert torch.equal(i0, i1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32)), k
        same_lists(i1, d1, ref_idx[:, :k], ref_d2[:, :k], f"{name} rebuilt {k_hint} k={k}")
    dr = T(radius_case(name), gpu)
    s0, m0 = g0.radius(dq, dr)
    s1, m1 = g1.radius(dq, dr)
    assert torch.equal(s0, s1) and torch.equal(m0, m1)


# ---------------------------------------------------------------------------- (f) the fused loop's K1 lists
FUSED_CASES = ("uniform_cube", "translated", "sheet", "needle", "two_clusters", "lattice_ties")


def fused_lists_against_brute_force(name, k, gpu, anchoring=True, seeding=True, cells_per_axis=None):
    """cells_per_axis: the loop on a grid of that many cells along the longest axis, not Processor._fused_for's."""
    snap, _ = case(name)
    n = len(snap)
    k_update = 8
    kstore = max(k, k_update)
    cap = nat.list_cap(kstore)
    ka = min(2 * cap, n)                                    # the anchors' list length 2K
    rng = np.random.default_rng(k)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    _, d2self = R.knn_f32(snap, snap, 2, np.arange(n))
    d = 2.0 * float(np.sqrt(d2self[:, 1].astype(np.float64)).mean())
    proc = Processor(Pointcloud(T(snap, gpu).clone(), T(nrm, gpu).clone()), k_hint=16)
    if cells_per_axis is None:
        fused = proc._fused_for(kstore)
    else:
        extent = float((snap.max(0).astype(np.float64) - snap.min(0)).max())
        fused = nat.FusedDenoiser(nat.Grid(T(snap, gpu), cell=extent / cells_per_axis), kstore)
    fused.set_anchoring(anchoring)
    fused.set_seeding(seeding)
    tie = R.inverse_perm(fused.grid.perm().cpu().numpy())    # the (d2, rank) order the kernels key on
    params = nat.make_params(k=k, k_update=k_update, d=d)
    fused.load(proc.graph.pos, proc.graph.n)
    pos = torch.empty((n, 3), device=gpu)
    far = 0.0
    stats = []

    def step(t):
        nonlocal far
        fused.store(pos)
        p_t = pos.cpu().numpy()
        assert np.isfinite(p_t).all(), (name, k, t)
        fused.iterate(params, 1)
        got = fused.lists(kstore).cpu().numpy()
        ref_idx, ref_d2 = R.knn_f32(p_t, snap, ka, tie)
        far = max(far, float(np.sqrt(ref_d2[:, -1].astype(np.float64)).max()))
        bad = (got != ref_idx[:, :kstore]).any(1)
        if bad.any():
            r = int(np.nonzero(bad)[0][0])
            raise AssertionError(f"{name} k={k} iteration {t}: {int(bad.sum())} of {n} rows differ; row {r}: got "
                                 f"{got[r].tolist()} want {ref_idx[r, :kstore].tolist()} d2 {ref_d2[r, :kstore].tolist()}")
        stats.append((t, fused.redo_rows(), fused.tile_stats()))
        return p_t

    seen = [step(t) for t in (1, 2, 3)]
    # every 7th row farther than the largest 2K-th neighbour distance seen (`far`) from every position it has held: an
    # anchor is one of those positions with D <= far, so the row cannot certify (the test needs d_k < D - |q - anchor|)
    fused.store(pos)
    moved = pos.cpu().numpy().copy()
    seen.append(moved.copy())
    rows = np.arange(0, n, 7)
    drift = max(float(np.linalg.norm(p[rows].astype(np.float64) - moved[rows], axis=1).max()) for p in seen)
    axis = rng.integers(0, 3, len(rows))
    shift = (2.0 * far + 2.0 * drift) * rng.choice([-1.0, 1.0], len(rows))
    moved[rows, axis] = (moved[rows, axis] + shift).astype(np.float32)
    for p in seen:
        assert (np.linalg.norm(moved[rows].astype(np.float64) - p[rows], axis=1) > far).all()
    fused.load(T(moved, gpu), proc.graph.n)
    p4 = step(4)
    assert (p4 == moved).all()
    redo4 = stats[-1][1]
    # beyond the issue's four iterations, the re-anchoring of rows that sit in the void: the same rows three times as
    # far again (their anchors' radius finds nothing), then nudged (anchors with a D of many cells: a cap box over the
    # quantised search's cell limit goes to the exact-key search)
    for t, amount in ((5, 3.0 * shift), (6, 0.25 * np.abs(shift))):
        fused.store(pos)
        moved = pos.cpu().numpy().copy()
        moved[rows, axis] = (moved[rows, axis] + amount).astype(np.float32)
        fused.load(T(moved, gpu), proc.graph.n)
        assert (step(t) == moved).all()
    report(f"fused K1 {name} k={k} anchoring={anchoring} seeding={seeding} cells {fused.grid.info()['dims']}: "
           + "; ".join(f"it{t} redo {redo} {ts}" for t, redo, ts in stats))
    if cap <= 32 and anchoring and seeding:
        assert redo4 >= len(rows), (stats, len(rows))


@pytest.mark.parametrize("k", [8, 13, 16, 32, 64])
@pytest.mark.parametrize("name", FUSED_CASES)
def test_fused_lists_are_brute_force(name, k, gpu):
    fused_lists_against_brute_force(name, k, gpu)


@pytest.mark.parametrize("anchoring,seeding", [(False, True), (True, False)])
@pytest.mark.parametrize("name", ["translated", "two_clusters"])
def test_fused_lists_without_anchoring_or_seeding(name, anchoring, seeding, gpu):
    fused_lists_against_brute_force(name, 16, gpu, anchoring=anchoring, seeding=seeding)


@pytest.mark.parametrize("name", ["uniform_cube", "translated"])
def test_fused_lists_on_a_fine_grid(name, gpu):
    """About one point per occupied cell, 40 cells an axis: the void rows' cap boxes pass the quantised search's cell
    limit (tile_stats' spilled_big_box), which the grids of _fused_for cannot reach at these sizes."""
    fused_lists_against_brute_force(name, 16, gpu, cells_per_axis=40)


def test_fused_refuses_fewer_points_than_k(gpu):
    """The documented refusal: k above the number of points."""
    snap = np.random.default_rng(1).random((12, 3)).astype(np.float32)
    proc = Processor(Pointcloud(T(snap, gpu).clone(), T(snap, gpu).clone()), k_hint=16)
    fused = proc._fused_for(16)
    fused.load(proc.graph.pos, proc.graph.n)
    with pytest.raises(ValueError, match="k exceeds the number of points"):
        fused.iterate(nat.make_params(k=16, k_update=8, d=0.1), 1)
