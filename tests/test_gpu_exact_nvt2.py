"""The exact NVT2 mode (`pcd_denoiser_set_exact_nvt2`) and the fused feature decomposition (`pcd_denoiser_decompose`).

The default NVT2 stage (`k_nvt2`) leaves the tensor unnormalised and solves it with a fixed-sweep Jacobi; the exact
variant (`k_nvt2_exact`) restates the reference's second vote as its first (Processor.py:110-117: getBetterFilteredNVT
on the filtered normals, Decompositionor.py:278-300): T / Σw and LAPACK's ssyevd, NVT1's arithmetic.  Everything here
is compared bit for bit (`assert_array_equal`):

* against the reference's own run (fandisk fixtures: `it1_eigval2`, `it1_eigvec2[..., 0]`, `it1_classes`);
* `decompose` against the op-by-op path (Selector -> pcd_nvt_csr -> pcd_vu_smooth -> pcd_nvt_csr), at every list cap,
  a list shorter than its cap, fewer than two blocks, and rows where no neighbour votes (the all-ones fallback);
* `Processor.getMyFeatureDecomposition(fused=True)` against `fused=False`;
* no side effects of `decompose` or of the switch, invariance to the windows / seeding / anchoring switches, and the
  default mode untouched;
* one chained iteration against the reference in both modes (the edge phase's deviation, the classes, the share of
  bit-identical rows): the measured figures are printed (DESIGN.md's parity table records them).
"""
import math

import numpy as np
import pytest
import torch

import pcd_native as nat
from oracle import pcd_oracle as O
from conftest import report
from Pointcloud.Modules.Object import Pointcloud
from Pointcloud.Modules.Processor import Processor

pytestmark = pytest.mark.gpu
KU = 8
MAX_LIST_MISMATCH = 0.001      # rows whose stored kNN list differs from the other side's (near-ties): at most 0.1 %


def _dev(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def _caller_rows(fd, grid, field, N, dev):
    """A state field (spatial order, float4 rows) in caller order [N, 3]."""
    rows = torch.arange(N, device=dev, dtype=torch.int32)
    out = torch.empty((N, 3), device=dev)
    out[grid.perm().long()] = fd.pack(field, rows)[:, :3]
    return out


def _unpack_caller(fd, grid, field, rows3, N, dev):
    f4 = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    f4[:, :3] = _dev(rows3, dev)[grid.perm().long()]
    fd.unpack(field, torch.arange(N, device=dev, dtype=torch.int32), f4)


# ------------------------------------------------------------------------------------- 1. the reference, bitwise
@pytest.mark.parametrize("k", [32, 16])
def test_exact_nvt2_is_the_reference_bitwise(golden, gpu, k):
    """K1, the reference's `it1_f_n` written over f_n, then the exact NVT2 stage with the probe on (the staging of
    test_gpu_stages.staged_iteration): eigenvalues, edge vectors (sign included) and classes are the reference's on
    every row whose stored list is the fixture's.  N = 6,475: the last block is partial."""
    f = golden(f"fandisk_k{k}")
    pos0, N = f["pos0"], len(f["pos0"])
    pos_t, n_t = _dev(pos0, gpu), _dev(f["n0"], gpu)
    grid = nat.Grid(pos_t, k_hint=k)
    fd = nat.FusedDenoiser(grid, max(k, KU))
    fd.load(pos_t, n_t)
    fd.set_probe(True)
    fd.set_exact_nvt2(True)
    p = nat.make_params(k=k, k_update=KU, d=float(f["d"]))
    fd.stage(p, nat.STAGE_KNN_NVT1)
    _unpack_caller(fd, grid, nat.FIELD_FN, f["it1_f_n"], N, gpu)
    fd.stage(p, nat.STAGE_NVT2)
    eig = fd.probe().cpu().numpy()
    edge = _caller_rows(fd, grid, nat.FIELD_EDGE, N, gpu).cpu().numpy()
    fd.stage(p, nat.STAGE_FINISH)                        # (no phase applied; classes and lists come out after finish)
    cls = torch.empty(N, dtype=torch.int64, device=gpu)
    fd.store(None, None, cls)
    same = (fd.lists(k).cpu().numpy() == f[f"knn{k}"]).all(1)
    report(f"fandisk k={k}: exact NVT2 compared on {int(same.sum())} of {N} rows ({int((~same).sum())} with another list)")
    assert (~same).mean() <= MAX_LIST_MISMATCH
    np.testing.assert_array_equal(eig[same, :3], f["it1_eigval2"][same])
    np.testing.assert_array_equal(edge[same], f["it1_eigvec2"][..., 0][same])
    np.testing.assert_array_equal(cls.cpu().numpy()[same], f["it1_classes"][same])


# ------------------------------------------------------------------------------------- 2. decompose vs op by op
def _random_cloud(n, seed):
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand((n, 3), generator=g)
    nrm = torch.nn.functional.normalize(torch.randn((n, 3), generator=g), dim=1)
    return pos.contiguous(), nrm.contiguous()


def _cloud_for(name, golden):
    if name == "fandisk":
        f = golden("fandisk_k32")
        return torch.from_numpy(f["pos0"].copy()), torch.from_numpy(f["n0"].copy())
    if name == "random300":
        return _random_cloud(300, 5)
    from test_gpu_scale import bunny_cloud
    return bunny_cloud(20_000, 3, 0.005)


# (cloud, k, rho, rows taking the all-ones fallback expected).  k = 12: the list is shorter than its cap (16);
# random300: fewer than two 256-row blocks; k = 64: the largest cap (pcd_denoiser_iterate accepts it, so must this).
# rho >= π/2: no pair votes, not even a row's own entry (acos(0) > rho fails), so every row takes the fallback; below
# π/2 the own entry always votes (the snapshot point of a row is its own neighbour) and no row does.
DECOMPOSE_CASES = [("fandisk", 32, None, False), ("fandisk", 16, None, False), ("fandisk", 12, None, False),
                   ("random300", 8, None, False), ("random300", 8, 1.6, True), ("fandisk", 16, math.pi / 2, True),
                   ("bunny20k", 64, None, False)]


@pytest.mark.parametrize("cloud,k,rho,fallback", DECOMPOSE_CASES,
                         ids=[f"{c}-k{k}" + ("" if r is None else f"-rho{r:.2f}") for c, k, r, _ in DECOMPOSE_CASES])
def test_decompose_is_the_op_by_op_path_bitwise(golden, gpu, cloud, k, rho, fallback):
    pos, nrm = _cloud_for(cloud, golden)
    N = pos.size(0)
    proc = Processor(Pointcloud(pos.to(gpu), nrm.to(gpu)), k_hint=k)
    angle = rho if rho is not None else math.pi * 5 / 12
    # op by op: Selector.getKNNSelection -> pcd_nvt_csr -> pcd_vu_smooth -> pcd_nvt_csr (+ pcd_classify)
    sel = proc.selector.getKNNSelection(k)
    n = proc.graph.n
    nvt = proc.decompositionor.getBetterFilteredNVT(sel, n, angle)
    ref_fn = nvt.getVUSmoothedNormals(n)
    ref = proc.decompositionor.getBetterFilteredNVT(sel, ref_fn, angle)
    ref_cls = ref.getClasses()
    # fused
    fd = proc._fused_for(k)
    fd.set_probe(True)
    fd.load(proc.graph.pos, n)
    ku = KU if k >= KU else k
    eigval, eigvec, f_n, cls = fd.decompose(nat.make_params(k=k, k_update=ku, rho=angle), want_classes=True)
    same = (fd.lists(k) == sel.j.view(N, k)).all(1)
    wsum = fd.probe()[:, 3]
    n_fb = int((wsum == k).sum())
    report(f"{cloud} k={k} rho={angle:.3f}: decompose compared on {int(same.sum())} of {N} rows "
           f"({int((~same).sum())} with another list); {n_fb} rows with Σw = k (every neighbour votes, or none: the fallback)")
    assert (~same).float().mean().item() <= MAX_LIST_MISMATCH
    if fallback:                                         # (rho >= π/2: no pair can vote, Σw = k is the fallback's)
        assert n_fb >= 1
    same = same.cpu().numpy()
    np.testing.assert_array_equal(fd.probe()[:, :3].cpu().numpy()[same], eigval.cpu().numpy()[same])
    np.testing.assert_array_equal(eigval.cpu().numpy()[same], ref.eigval.cpu().numpy()[same])
    np.testing.assert_array_equal(eigvec.cpu().numpy()[same], ref.eigvec.cpu().numpy()[same])
    np.testing.assert_array_equal(f_n.cpu().numpy()[same], ref_fn.cpu().numpy()[same])
    np.testing.assert_array_equal(cls.cpu().numpy()[same], ref_cls.cpu().numpy()[same])


def test_decompose_outputs_are_nullable_and_checked(golden, gpu):
    f = golden("fandisk_k16")
    pos_t, n_t = _dev(f["pos0"], gpu), _dev(f["n0"], gpu)
    fd = nat.FusedDenoiser(nat.Grid(pos_t, k_hint=16), 16)
    p = nat.make_params(k=16, k_update=8)
    with pytest.raises(ValueError):                      # nothing loaded: as pcd_denoiser_iterate
        fd.decompose(p)
    fd.load(pos_t, n_t)
    with pytest.raises(ValueError):                      # k beyond the k_max given at create: as pcd_denoiser_iterate
        fd.decompose(nat.make_params(k=32, k_update=8))
    full = fd.decompose(p, want_classes=True)
    from ctypes import byref, c_void_p
    ev = torch.empty((len(f["pos0"]), 3), device=gpu)
    nat.check(nat.lib().pcd_denoiser_decompose(fd.handle, byref(p), nat.ptr(ev), None, None, None,
                                               c_void_p(nat.stream_ptr())), "pcd_denoiser_decompose")
    np.testing.assert_array_equal(ev.cpu().numpy(), full[0].cpu().numpy())
    nat.check(nat.lib().pcd_denoiser_decompose(fd.handle, byref(p), None, None, None, None,
                                               c_void_p(nat.stream_ptr())), "pcd_denoiser_decompose")


# ------------------------------------------------------------------------------------- 3. Processor
def test_processor_fused_decomposition_equals_op_by_op(golden, gpu):
    f = golden("fandisk_k32")
    pc = Pointcloud(_dev(f["pos0"], gpu), _dev(f["n0"], gpu))
    proc = Processor(pc, k_hint=16)
    pos_before, n_obj, n_before = proc.graph.pos.clone(), proc.graph.n, proc.graph.n.clone()
    for N in (16, 32):
        dec_a, fn_a = proc.getMyFeatureDecomposition(N, fused=False)
        dec_b, fn_b = proc.getMyFeatureDecomposition(N, fused=True)
        np.testing.assert_array_equal(dec_b.eigval.cpu().numpy(), dec_a.eigval.cpu().numpy())
        np.testing.assert_array_equal(dec_b.eigvec.cpu().numpy(), dec_a.eigvec.cpu().numpy())
        np.testing.assert_array_equal(fn_b.cpu().numpy(), fn_a.cpu().numpy())
        np.testing.assert_array_equal(dec_b.getClasses().cpu().numpy(), dec_a.getClasses().cpu().numpy())
        assert fn_b.dtype == fn_a.dtype and fn_b.device == fn_a.device
    assert proc.graph.n is n_obj
    assert torch.equal(proc.graph.pos, pos_before) and torch.equal(proc.graph.n, n_before)


# ------------------------------------------------------------------------------------- 4-6. switches, side effects
def _run(pos_t, n_t, p, iters, k, setup=None, before=None):
    """load; iterate(iters); store -> (pos, n, classes, edge vectors) as numpy.  setup(fd): before load; before(fd):
    between load and iterate."""
    fd = nat.FusedDenoiser(nat.Grid(pos_t, k_hint=k), max(k, KU))
    if setup:
        setup(fd)
    fd.load(pos_t, n_t)
    if before:
        before(fd)
    fd.iterate(p, iters)
    N = pos_t.size(0)
    out = (torch.empty_like(pos_t), torch.empty_like(n_t), torch.empty(N, dtype=torch.int64, device=pos_t.device),
           torch.empty_like(pos_t))
    fd.store(*out)
    return [t.cpu().numpy() for t in out]


def _assert_same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_decompose_and_the_switch_leave_no_trace(golden, gpu, exact):
    f = golden("fandisk_k32")
    pos_t, n_t = _dev(f["pos0"], gpu), _dev(f["n0"], gpu)
    p = nat.make_params(k=32, k_update=KU, d=float(f["d"]))
    on = (lambda fd: fd.set_exact_nvt2(True)) if exact else None
    plain = _run(pos_t, n_t, p, 2, 32, setup=on)
    # load; decompose; iterate(2); store == load; iterate(2); store
    _assert_same(_run(pos_t, n_t, p, 2, 32, setup=on, before=lambda fd: fd.decompose(p, want_classes=True)), plain)
    if exact:
        return

    # exact on, one iteration, exact off, load again: a fresh default run
    def toggled(fd):
        fd.set_exact_nvt2(True)
        fd.load(pos_t, n_t)
        fd.iterate(p, 1)
        fd.set_exact_nvt2(False)
    _assert_same(_run(pos_t, n_t, p, 2, 32, setup=toggled), plain)


def test_decompose_between_iterations_keeps_the_loop_state(golden, gpu):
    """iterate(1); decompose; iterate(1) == iterate(2): no position moved, normals not rebound, and store()'s
    classes / edge vectors are the last iteration's (decompose keeps its own)."""
    f = golden("fandisk_k32")
    pos_t, n_t = _dev(f["pos0"], gpu), _dev(f["n0"], gpu)
    p = nat.make_params(k=32, k_update=KU, d=float(f["d"]))
    plain = _run(pos_t, n_t, p, 2, 32)
    fd = nat.FusedDenoiser(nat.Grid(pos_t, k_hint=32), 32)
    fd.load(pos_t, n_t)
    fd.iterate(p, 1)
    N = pos_t.size(0)
    a = (torch.empty_like(pos_t), torch.empty_like(n_t), torch.empty(N, dtype=torch.int64, device=gpu), torch.empty_like(pos_t))
    b = tuple(torch.empty_like(t) for t in a)
    fd.store(*a)
    fd.decompose(p)
    fd.store(*b)
    _assert_same([t.cpu().numpy() for t in a], [t.cpu().numpy() for t in b])
    fd.iterate(p, 1)
    fd.store(*b)
    _assert_same([t.cpu().numpy() for t in b], plain)


def test_exact_nvt2_is_invariant_to_the_work_switches(gpu):
    """Exact on: LDS windows off == on, seeding / anchoring off == on, bit for bit (60k points, k = 32, 3 iterations:
    test_gpu_slab._cloud)."""
    from test_gpu_slab import _cloud, _d
    pos, nrm = _cloud(gpu)
    p = nat.make_params(k=32, k_update=KU, d=_d(pos))
    base = _run(pos, nrm, p, 3, 32, setup=lambda fd: fd.set_exact_nvt2(True))

    def no_windows(fd):
        fd.set_exact_nvt2(True)
        fd.set_windows(False)

    def no_seeding(fd):
        fd.set_exact_nvt2(True)
        fd.set_seeding(False)
        fd.set_anchoring(False)

    def no_anchoring(fd):
        fd.set_exact_nvt2(True)
        fd.set_anchoring(False)
    _assert_same(_run(pos, nrm, p, 3, 32, setup=no_windows), base)
    _assert_same(_run(pos, nrm, p, 3, 32, setup=no_seeding), base)
    _assert_same(_run(pos, nrm, p, 3, 32, setup=no_anchoring), base)
    # and the mode is on: LAPACK's sign convention differs from the default solver's on some row
    default = _run(pos, nrm, p, 3, 32)
    assert (default[3] != base[3]).any()


def test_default_mode_is_untouched(golden, gpu):
    """Exact off (the setter called with 0) == a denoiser on which the setter was never called, after 2 iterations:
    positions, normals, classes, edge vectors."""
    f = golden("fandisk_k32")
    pos_t, n_t = _dev(f["pos0"], gpu), _dev(f["n0"], gpu)
    p = nat.make_params(k=32, k_update=KU, d=float(f["d"]))
    _assert_same(_run(pos_t, n_t, p, 2, 32, setup=lambda fd: fd.set_exact_nvt2(False)), _run(pos_t, n_t, p, 2, 32))


# ------------------------------------------------------------------------------------- 7. chained iteration
def _staged(pos0, n0, d, dev, k, exact):
    """One fused iteration stage by stage on its own f_n (test_gpu_stages.staged_iteration without injection), in
    default or exact mode: positions after the edge phase and after the iteration, f_n, classes, lists."""
    pos_t, n_t = _dev(pos0, dev), _dev(n0, dev)
    grid = nat.Grid(pos_t, k_hint=k)
    fd = nat.FusedDenoiser(grid, max(k, KU))
    fd.set_exact_nvt2(exact)
    fd.load(pos_t, n_t)
    p = nat.make_params(k=k, k_update=KU, d=d)
    N = len(pos0)
    red4 = torch.zeros(4, dtype=torch.float64, device=dev)
    fd.stage(p, nat.STAGE_KNN_NVT1)
    fd.stage(p, nat.STAGE_NVT2)
    out = {}
    for ph in range(3):
        if p.phase_kind[ph] in (nat.STEP_FLAT, nat.STEP_NEW):
            fd.stage(p, nat.STAGE_PHASE_SUM, ph, red4)
            fd.stage(p, nat.STAGE_PHASE_CENTRE, ph, red4)
            fd.stage(p, nat.STAGE_PHASE_MAXDIST, ph, None)
        fd.stage(p, nat.STAGE_PHASE_APPLY, ph, None)
        if ph == 1:
            q = torch.empty((N, 3), device=dev)
            fd.store(q)
            out["pos_after_1"] = q.cpu().numpy()
    fd.stage(p, nat.STAGE_FINISH)
    q, fn = torch.empty((N, 3), device=dev), torch.empty((N, 3), device=dev)
    cls = torch.empty(N, dtype=torch.int64, device=dev)
    fd.store(q, fn, cls)
    out.update(pos=q.cpu().numpy(), f_n=fn.cpu().numpy(), classes=cls.cpu().numpy(), knn=fd.lists(k).cpu().numpy())
    return out


def _decided(got, ref_cls, ref_fn, knn, k):
    """The rows test_gpu_stages.check_stages calls decided: class, update neighbours' classes, own and neighbours'
    smoothed normals and the update list all agree with the reference's."""
    from test_gpu_stages import angle
    fn_ok = angle(got["f_n"], ref_fn) < 1e-5
    fn_same = np.abs(got["f_n"] - ref_fn).max(1) < 1e-5
    nb_fn_ok = fn_ok[knn[:, :k]].all(1) & fn_ok
    cls_ok = got["classes"] == ref_cls
    nb = knn[:, :KU]
    knn_ok = (got["knn"][:, :KU] == nb).all(1)
    return cls_ok & cls_ok[nb].all(1) & fn_same & fn_same[nb].all(1) & nb_fn_ok & knn_ok


def _chained(label, pos0, n0, d, dev, k, ref_cls, ref_fn, ref_knn, ref_after_1, ref_pos):
    bbox = float(np.linalg.norm(pos0.max(0) - pos0.min(0)))
    fig = {}
    for exact in (False, True):
        got = _staged(pos0, n0, d, dev, k, exact)
        m = _decided(got, ref_cls, ref_fn, ref_knn, k) & (ref_cls == 1)
        assert m.sum() > 0, label
        dev_ = np.linalg.norm(got["pos_after_1"] - ref_after_1, axis=1)[m] / bbox
        fig[exact] = dict(p999=float(np.percentile(dev_, 99.9)), max=float(dev_.max()),
                          identical=float((got["pos"] == ref_pos).all(1).mean()))
        if exact:
            # NVT2's inputs are the reference's: the row's list, and f_n bit-identical on it
            bits = (got["f_n"] == ref_fn).all(1)
            same_list = (got["knn"][:, :k] == ref_knn[:, :k]).all(1)
            inputs = bits & bits[ref_knn[:, :k]].all(1) & same_list
            fig["inputs"] = float(inputs.mean())
            cls_equal = bool((got["classes"] == ref_cls)[inputs].all())
    report(f"{label} chained iteration, edge phase over the decided rows / bbox: default p99.9 {fig[False]['p999']:.3g} "
           f"max {fig[False]['max']:.3g}, exact p99.9 {fig[True]['p999']:.3g} max {fig[True]['max']:.3g}; rows "
           f"bit-identical after the iteration: default {fig[False]['identical']:.6f}, exact {fig[True]['identical']:.6f}; "
           f"rows with the reference's NVT2 inputs {fig['inputs']:.6f}")
    assert fig[True]["p999"] <= fig[False]["p999"], fig
    # (not vacuous: check_stages allows 0.5 % of the rows a neighbour whose f_n differs; a row with another list can
    # sit in up to k others' lists, so well over half of the rows must carry the reference's inputs)
    assert fig["inputs"] > 0.8 and cls_equal, fig
    assert fig[True]["identical"] >= fig[False]["identical"], fig


def test_chained_iteration_fandisk(golden, gpu):
    """One iteration on its own f_n against the reference's run, default and exact mode.  Measured on an MI355X: edge
    phase p99.9 1.33e-6 -> 6.7e-9, max 3.06e-6 -> 2.3e-8 x bbox; rows bit-identical to pos_it1 70.05 % -> 96.28 %; every
    row carries the reference's NVT2 inputs (DESIGN.md's parity table)."""
    f = golden("fandisk_k32")
    _chained("fandisk k=32", f["pos0"], f["n0"], float(f["d"]), gpu, 32, f["it1_classes"], f["it1_f_n"],
             f["knn32"].astype(np.int64), f["it1_pos_after_1"], f["pos_it1"])


def test_chained_iteration_bunny_50k(gpu):
    """The same on a 50,000-point sample of the headline workload against the CPU oracle (O.denoise_iteration).
    Measured on an MI355X: edge phase p99.9 9.7e-7 -> 0, max 2.36e-6 -> 1.4e-8 x bbox; identical rows 93.35 % -> 99.46 %."""
    from test_gpu_scale import bunny_cloud
    pos, nrm = bunny_cloud(50_000, 2, 0.005)
    p0, n0 = pos.numpy(), nrm.numpy()
    knn = O.FrozenKNN(p0)
    d = 2 * O.mean_edge_length(p0, knn)
    rec = {}
    rpos, _, _ = O.denoise_iteration(p0, n0, knn, d, 32, KU, record=rec)
    _chained("bunny 50k k=32", p0, n0, d, gpu, 32, rec["classes"], rec["f_n"], rec["knn"].astype(np.int64),
             rec["pos_after_1"], rpos)
