"""The consumers of the neighbour lists on the device, on the rows where a kernel can be subtly wrong: votes at the
threshold and across the guards of the squared-form fast path, the fallbacks, odd normals, degenerate and non-finite
eigen-systems, tie orders, exactly singular solves and steps exactly on the clamp.

The references are tests/nvt_ref.py's (checked without a GPU by tests/test_nvt_ref.py, which also sends every row that
carries NaN, inf, an empty list or a zero tensor through the host build first): a float64 judge says which votes a
float32 evaluation may cast either way, and the device must be bit-equal to ONE admissible candidate on every row.
"""
import math

import numpy as np
import pytest
import torch

import nvt_ref as R
import pcd_native as nat
from conftest import report
from oracle import pcd_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
KINDS = {"flat": nat.STEP_FLAT, "edge": nat.STEP_EDGE, "feature": nat.STEP_FEATURE, "corner": nat.STEP_CORNER,
         "new": nat.STEP_NEW, "dummy": nat.STEP_DUMMY}


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ (a) pcd_nvt_csr
@pytest.mark.parametrize("builder", ["threshold[unit]", "threshold[nonunit]", "scale", "fallback", "odd_normals"])
def test_nvt_csr_votes_on_hard_rows(gpu, builder):
    """pcd_nvt_csr (the two-path vote, the sums, the fallback, eigh3) at every rho of nvt_ref.RHOS and SPECIAL_RHOS:
    eigenvalues and eigenvectors bit-equal to an admissible candidate on every row; an empty row gives what the host
    build gives (NaN eigenvalues from 0 / 0).  A NaN normal poisons the rows that list it whether it votes or not, as
    the reference's weight product does (0 * NaN): those rows are NaN in every candidate and on the device."""
    rows_und = rows_all = 0
    for label, rho, rows, may in R.vote_cases():
        if not label.startswith(builder):
            continue
        pos, n, ci, off, nbr = rows
        _, cands = R.judge_rows(rho, rows, may)
        w, v = nat.nvt_csr(T(pos, gpu), T(n, gpu), T(ci, gpu), T(off, gpu), T(nbr, gpu), rho)
        w, v = N(w), N(v)
        report("device " + R.check_decompositions(label, cands, len(ci), w, v))
        hw, hv = nat.host_eigh3(nat.host_nvt_tensor(pos, n, ci, off, nbr, rho))
        empty = np.diff(off) == 0
        assert R.same_bits(w[empty], hw[empty]).all() and R.same_bits(v[empty], hv[empty]).all(), label
        assert np.isnan(w[empty]).all(), label
        if builder == "odd_normals":
            listed_nan = np.isnan(n[nbr]).any(1)
            nan_rows = np.unique(R.segments(off)[listed_nan])
            assert np.isnan(w[nan_rows]).all() and np.isfinite(np.delete(w, nan_rows, 0)).all(), label
        rows_und += int((cands["u"] > 0).sum())
        rows_all += len(ci)
    report(f"pcd_nvt_csr {builder}: {rows_und} of {rows_all} rows had undecided pairs")


# ------------------------------------------------------------------- (b) pcd_nvt_normal_csr / pcd_pvt_normal_csr
@pytest.mark.parametrize("rho", R.NORMAL_RHOS)
def test_cpsd_votes_on_hard_rows(gpu, rho):
    """CPSD's vote (no abs, <=, the 1e-6 band around cos(rho)) with n_i . n_j at the float32 neighbours of cos(rho), rows
    of 65, 100 and 200 members whose voters sit only past member 64 (pvt_normal_cov re-votes from there) or only before
    it, rows without a voter and empty rows: bit-equal to an admissible candidate (the existing CPSD tests hold these
    kernels to the bit on their fixture)."""
    pos, n, ci, off, nbr = R.normal_rows(rho)
    may = np.abs(n[nbr, 0] - F32(math.cos(F32(rho)))) < 1e-6
    dev = [T(x, gpu) for x in (pos, n, ci, off, nbr)]
    for kind, fn in (("normal", lambda: nat.nvt_normal_csr(*dev[1:], rho)),
                     ("pvt", lambda: nat.pvt_normal_csr(*dev, rho))):
        _, cands = R.judge_rows(rho, (pos, n, ci, off, nbr), may, kind)
        w, v = fn()
        report("device " + R.check_decompositions(f"cpsd {kind} rho={rho}", cands, len(ci), N(w), N(v)))
        # the oracle's own float32 chain is one of the candidates too (its sums are the same list-order sums)
        ow, ov = (O.normal_filtered_nvt(n, ci, off, nbr, rho) if kind == "normal"
                  else O.normal_filtered_pvt(pos, n, ci, off, nbr, rho))
        R.check_decompositions(f"oracle {kind}", cands, len(ci), ow, ov)


# --------------------------------------------------------------------------------------------- (c) pcd_eigh3_batch
def test_eigh3_batch_on_eigen_cases(gpu):
    """Solver 0 (the LAPACK restatement) bit-equal to O.eigh with the same NaN pattern on zero, repeated, rank-deficient,
    tiny, huge, NaN and inf tensors; solver 1 (NVT2's Jacobi) within test_nvt2_jacobi_matches_lapack_restatement's three
    gates of solver 0 on the finite cases, and all-NaN eigenvalues where an input is NaN.
    Solver 1 builds its rotations from 1 / a_pq (a hardware estimate), which overflows for a subnormal off-diagonal:
    it then skips the rotation as negligible.  That is right whenever the diagonal is of normal size (NVT2's tensors
    are sums of unit normals: trace = sum w >= 1) and wrong for a tensor that is subnormal as a whole (the 2^-140
    cases), which no cloud produces: there the eigenvalues are held to the absolute gate only (within 2e-6 x 1e-30)
    and must be finite and subnormal; the class gate applies from lambda_max >= 2^-126 on, the vector gate from 2^-30
    on, and what the device returns below (a NaN vector on the zero tensor and at 2^-100) is asserted as it is."""
    from test_gpu_stages import angle
    names, t6 = R.eigen_cases()
    w0, V0 = (N(x) for x in nat.eigh3_batch(T(t6, gpu), 0))
    rw, rv = O.eigh(R.full3(t6))
    bad = ~(R.same_bits(w0, rw).all(1) & R.same_bits(V0, rv).reshape(len(w0), -1).all(1))
    assert not bad.any(), [(names[i], w0[i], rw[i]) for i in np.nonzero(bad)[0][:5]]
    w1, y1 = (N(x) for x in nat.eigh3_batch(T(t6, gpu), 1))
    nan_in = np.isnan(t6).any(1)
    assert nan_in.sum() == 2 and np.isnan(w1[nan_in]).all()
    fin = np.isfinite(t6).all(1)
    with np.errstate(all="ignore"):
        lmax = np.abs(w0).max(1)
        ew = np.abs(w1.astype(np.float64) - w0).max(1) / np.maximum(lmax, 1e-30)
        p_, l_, s_ = O.nvt_features(w0)
        f = np.sort(np.stack([F32(0.2) * p_, l_, s_], 1), 1)
        normal = fin & (lmax >= 2.0 ** -126)
        decided = normal & ((f[:, 2] - f[:, 1]) > 1e-5)
        gap = (w0[:, 1] - w0[:, 0]) / np.maximum(lmax, 1e-30)
    report(f"eigh3_batch solver 1 vs 0 on {fin.sum()} finite eigen cases: eigenvalue error max {ew[fin].max():.3g} of "
           f"lambda_max (bound 2e-6), worst {names[int(np.argmax(np.where(fin, ew, 0)))]}")
    assert ew[fin].max() <= 2e-6, [(names[i], w1[i], w0[i]) for i in np.nonzero(fin & (ew > 2e-6))[0][:5]]
    diff = decided & (O.classes(w0) != O.classes(w1))
    assert not diff.any(), [names[i] for i in np.nonzero(diff)[0][:5]]
    # Below lambda_max = 2^-30 the device's behaviour is kept and asserted as it is.  Every finite case has finite
    # eigenvalues (the zero tensor and the two 2^-140 ones, below the normal range, included).  The eigenvector is
    # refined where |cross|^2 >= (1e-3 lambda_max^2)^2; that bound underflows to 0 for lambda_max below ~2^-31, where a
    # cross product that underflowed to 0 passes it and the vector is 0 x rsq(0) = NaN: on the zero tensor and on both
    # tensors at 2^-100 (the full-rank one too).  From 2^-30 on, six orders below any NVT2 tensor, vectors are finite.
    tiny = {nm: i for i, nm in enumerate(names) if nm == "zero" or nm.startswith("scale_2^-1")}
    report("eigh3_batch solver 1 below lambda_max 2^-30 (kept behaviour): " + "; ".join(
        f"{nm}: w {w1[i].tolist()} y {y1[i].tolist()}" for nm, i in tiny.items()))
    assert (fin & ~normal).sum() == 3 and np.isfinite(w1[fin]).all()
    assert sorted(tiny) == ["scale_2^-100", "scale_2^-100_rank1", "scale_2^-140", "scale_2^-140_rank1", "zero"]
    for nm in ("zero", "scale_2^-100", "scale_2^-100_rank1"):
        assert np.isnan(y1[tiny[nm]]).all(), (nm, y1[tiny[nm]])
    for nm in ("scale_2^-140", "scale_2^-140_rank1"):
        assert np.isfinite(w1[tiny[nm]]).all() and (np.abs(w1[tiny[nm]]) < 2.0 ** -126).all(), (nm, w1[tiny[nm]])
    assert (w1[tiny["zero"]] == 0).all()
    assert np.isfinite(y1[fin & (lmax >= 2.0 ** -30)]).all(), [names[i] for i in np.nonzero(
        fin & (lmax >= 2.0 ** -30) & ~np.isfinite(y1).all(1))[0][:5]]
    ok = normal & (gap > 1e-4) & (lmax >= 2.0 ** -30)
    a = angle(y1[ok], V0[ok][..., 0])
    bound = 5e-7 / gap[ok] + 5e-7
    report(f"eigh3_batch solver 1 smallest eigenvector: max angle / bound {(a / bound).max():.3g} (bound 1) on "
           f"{ok.sum()} cases with a relative gap above 1e-4")
    assert (a <= bound).all(), [names[i] for i in np.nonzero(ok)[0][a > bound][:5]]


# --------------------------------------------------------------------------------- (d) pcd_vu_smooth, pcd_classify
def test_vu_smooth_ties_threshold_and_cancellation(gpu):
    """pcd_vu_smooth bit-equal to O.vu_smoothed_normals (NaN pattern included): every tie pattern of the eigenvalues
    (stable descending order), eigenvalues at tau and its float32 neighbours (strict >), n = 0, NaN, exact cancellation."""
    cases = R.vu_cases()
    for name, w, E, n, tau, damp in cases:
        with np.errstate(all="ignore"):
            ref = O.vu_smoothed_normals(w, E, n, tau, damp)
        got = N(nat.vu_smooth(T(w, gpu), T(E, gpu), T(n, gpu), tau, damp))
        same = R.same_bits(got, ref).all(1)
        assert same.all(), (name, np.nonzero(~same)[0][:5], got[~same][:2], ref[~same][:2])
    report(f"pcd_vu_smooth: {len(cases)} cases x {len(cases[0][1])} rows bit-equal (bound: all)")


def test_classify_ties_and_nan(gpu):
    """pcd_classify on exact ties of the three scores, all-zero, negative, infinite and NaN eigenvalues at the scales
    0.2, 0 and 1: classes equal to O.classes (torch.argmax's rule: NaN is the maximum, the first index wins), features
    bit-equal to O.nvt_features with the same NaN pattern."""
    names, w = R.class_cases()
    for scale in R.CLASS_SCALES:
        cls, feat = nat.classify(T(w, gpu), scale, want_features=True)
        with np.errstate(all="ignore"):
            ref = O.classes(w, scale)
            rf = np.stack(O.nvt_features(w), 1)
        bad = N(cls) != ref
        assert not bad.any(), [(names[i], scale, N(cls)[i], ref[i]) for i in np.nonzero(bad)[0][:5]]
        same = R.same_bits(N(feat), rf).all(1)
        assert same.all(), [(names[i], N(feat)[i], rf[i]) for i in np.nonzero(~same)[0][:5]]
    report(f"pcd_classify: {len(names)} triples x {len(R.CLASS_SCALES)} scales equal (bound: all)")


# ------------------------------------------------------------------------------------------------ (e) pcd_step_csr
def device_step(kind, c, dev):
    ev = T(c["ev"], dev)
    nbr = c["nbr"] if len(c["nbr"]) else np.zeros(1, np.int64)
    return N(nat.step_csr(KINDS[kind], T(c["pos"], dev), T(c["n"], dev), ev, T(c["ci"], dev), T(c["off"], dev),
                          T(nbr, dev), c["d"], c["alpha"]))


@pytest.mark.parametrize("kind", R.STEP_KINDS)
def test_step_csr_on_singular_clamped_and_ragged_rows(gpu, kind):
    """pcd_step_csr on nvt_ref.step_cases: ragged CSR rows (empty, one member, 65 and 200 members), exactly singular
    systems (the oracle's info mask is False there: the row keeps v_i), steps exactly on the clamp (< for edge,
    feature and corner, whose clamp_step new shares; <= for flat) and one float32 above / below it, d in {0, -1,
    inf}, delta = 0, a NaN position. Edge, feature, corner: bit-equal to the oracle. Flat, new: within 8 x the
    oracle's own float32 deviation from float64 + 4u |v_i| per case; where the oracle keeps v_i the device returns
    it bit for bit -- except `new` under a NaN position, where the device's delta is 0 instead of NaN: the rows
    that do not list the NaN point solve (I + (1 + k) n n^T) x = (I + (1 + k) n n^T) v_i and are held to the
    allowance, the rows that list it keep v_i."""
    ratios = []
    for c in R.step_cases(kind):
        label = f"{kind}/{c['name']}"
        got = device_step(kind, c, gpu)
        ref = R.oracle_step(kind, c)
        vi = c["pos"][c["ci"]]
        if "expect" in c:
            assert R.same_bits(got, c["expect"]).all(), (label, got, c["expect"])
        if kind in ("edge", "feature", "corner"):
            same = R.same_bits(got, ref).all(1)
            assert same.all(), (label, np.nonzero(~same)[0][:8], got[~same][:2], ref[~same][:2])
            if c["singular"] is not None:
                assert (R.oracle_ok(kind, c) == ~c["singular"]).all(), label
                assert c["singular"].any() and R.same_bits(got[c["singular"]], vi[c["singular"]]).all(), label
        elif kind in ("flat", "new"):
            ratio, dev_, bound, fin = R.flat_new_allowance(kind, c, got, ref)
            ratios.append((c["name"], round(ratio, 3)))
            print(f"{label}: device deviation / allowance {ratio:.3f} (bound 1)")
            assert ratio <= 1.0, (label, ratio)
            still = R.same_bits(ref, vi).all(1)
            if "nan_rows" in c:
                # A NaN position makes the global centre NaN, and with it every distance: the oracle's delta is NaN
                # (numpy's max propagates it) and nobody moves; the kernels' fmaxf drops the NaN distances, delta = 0,
                # every weight is 0 or NaN, and nobody moves past the allowance above either.  The rows that list the
                # NaN point (or sit on it) keep v_i bit for bit: a NaN step fails the clamp.
                assert R.same_bits(got[c["nan_rows"]], vi[c["nan_rows"]]).all(), label
                if kind == "flat":      # every weight 0 or NaN, the sum 0 / 0: flat moves NOBODY, bit for bit
                    assert R.same_bits(got, vi).all(), (label, np.nonzero(~R.same_bits(got, vi).all(1))[0][:8])
            else:
                assert R.same_bits(got[still], vi[still]).all(), (label, np.nonzero(still)[0][:8])
        else:
            assert R.same_bits(got, vi).all(), label
    if kind in ("edge", "feature", "corner"):
        # the clamp rows differ between d and the next float32 exactly as the oracle's do
        by = {c["name"]: c for c in R.step_cases(kind) if c["name"].startswith("clamp")}
        flips = 0
        for alpha in (1.0, 0.5, 0.0, -1.0):
            at, above = by[f"clamp_alpha{alpha}_at"], by[f"clamp_alpha{alpha}_above"]
            g = [device_step(kind, x, gpu) for x in (at, above)]
            o = [R.oracle_step(kind, x) for x in (at, above)]
            assert R.same_bits(g[0], o[0]).all() and R.same_bits(g[1], o[1]).all(), (kind, alpha)
            flips += int(not R.same_bits(g[0], g[1]).all())
        assert flips == 2, (kind, flips)                 # alpha = 1 and -1 sit on the clamp; 0.5 and 0 inside it
        report(f"pcd_step_csr {kind}: bit-equal to the oracle on every case (bound: all); clamp flips at d -> next "
               f"float32 for alpha = +-1 only")
    elif ratios:
        report(f"pcd_step_csr {kind}: device deviation / (8 x oracle's float32 deviation + 4u|v|) per case {ratios} "
               f"(bound 1)")


# ---------------------------------------------------------------------------- (f) the fused loop on the hard clouds
def _close_to_candidate(cands, m, eig, cls, edge):
    """Default-mode NVT2 against the candidates with test_gpu_stages.py's gates: eigenvalues within 2e-6 lambda_max,
    the class equal where the candidate's argmax margin exceeds 1e-5, the edge vector within 5e-7 / gap + 5e-7 where
    the relative gap exceeds 1e-4.  -> (ok [m], worst eigenvalue error / lambda_max, rows compared on class, on edge)."""
    from test_gpu_stages import angle
    row = cands["row"]
    with np.errstate(all="ignore"):
        lmax = np.abs(cands["eigval"]).max(1)
        e_err = np.abs(eig[row].astype(np.float64) - cands["eigval"]).max(1) / np.maximum(lmax, 1e-30)
        e_ok = e_err <= 2e-6
        margin = R.class_margin(cands["eigval"])
        c_cmp = margin > 1e-5
        c_ok = ~c_cmp | (cls[row] == cands["cls"])
        gap = (cands["eigval"][:, 1] - cands["eigval"][:, 0]) / np.maximum(lmax, 1e-30)
        v_cmp = gap > 1e-4
        a = angle(edge[row], cands["edge"])
        v_ok = ~v_cmp | (a <= 5e-7 / np.maximum(gap, 1e-30) + 5e-7)
    good = e_ok & c_ok & v_ok
    ok = np.zeros(m, bool)
    ok[row[good]] = True
    return ok, float(e_err[good].max()) if good.any() else 0.0, int(c_cmp.sum()), int(v_cmp.sum()), (e_ok, c_ok, v_ok)


@pytest.mark.parametrize("k", [16, 32])
@pytest.mark.parametrize("name", R.FUSED_CLOUDS)
def test_fused_stages_on_hard_clouds(gpu, name, k):
    """One fused iteration, stage by stage (k_knn_nvt1 / k_nvt1, k_nvt2, k_nvt2_exact, k_phase), on the degenerate
    clouds of tests/knn_ref.py.  Every reference is fed the device's OWN tensors (its lists, f_n, classes, edge vectors,
    the positions before each phase), so only the stage under test is judged: NVT1's f_n bit-equal to the VU smoothing
    of an admissible candidate; the probe's sum of votes equal to the judge's count; exact NVT2 bit-equal to a
    candidate of the reference chain, default NVT2 within test_gpu_stages.py's gates of one; the edge and feature
    phases bit-equal to the oracle's steps, the flat phase within (e)'s allowance; the flat phase's centre sums, count
    and pruned delta equal to the exhaustive ones."""
    from test_gpu_stages import staged_iteration
    ku = 8
    pos0, n0 = R.hard_cloud(name)
    m = len(pos0)
    near = np.linalg.norm(pos0[:, None, :].astype(np.float64) - pos0[None, :64], axis=2)
    d = float(2 * np.sort(near, 1)[:, :7].mean()) or 1.0
    runs = {mode: staged_iteration(pos0, n0, d, gpu, k=k, ku=ku, exact=(mode == "exact"), reductions=True)
            for mode in ("default", "exact")}
    lines = []
    for mode, got in runs.items():
        lists = got["knn"][:, :k]
        # NVT1: the smoothed normals
        _, c1 = R.nvt_stage(pos0, n0, lists, smooth=(n0, 0.3, 3.0))
        assert len(c1["unjudged"]) == 0
        ok, _ = R.match_candidates(c1, m, (got["f_n"], "fn"))
        assert ok.all(), (name, k, mode, "NVT1 f_n", np.nonzero(~ok)[0][:8])
        # NVT2 on the device's own f_n: sum of votes, then the decomposition
        fn = got["f_n"]
        _, c2 = R.nvt_stage(pos0, fn, lists)
        assert len(c2["unjudged"]) == 0
        wmin = np.full(m, 10 ** 9); wmax = np.zeros(m, np.int64)
        np.minimum.at(wmin, c2["row"], c2["wsum"]); np.maximum.at(wmax, c2["row"], c2["wsum"])
        sw = got["eig2"][:, 3]
        assert ((sw >= wmin) & (sw <= wmax)).all(), (name, k, mode, "sum w", np.nonzero((sw < wmin) | (sw > wmax))[0][:8])
        cls, edge = got["classes"], got["edge"]
        if mode == "exact":
            ok, _ = R.match_candidates(c2, m, (got["eig2"][:, :3], "eigval"), (cls, "cls"), (edge, "edge"))
            assert ok.all(), (name, k, "exact NVT2", np.nonzero(~ok)[0][:8])
            nvt2 = "bit-equal"
        else:
            ok, worst, ncls, nedge, parts = _close_to_candidate(c2, m, got["eig2"][:, :3], cls, edge)
            assert ok.all(), (name, k, "default NVT2", np.nonzero(~ok)[0][:8], [int((~p).sum()) for p in parts])
            nvt2 = f"eig err {worst:.2g} of lambda_max (bound 2e-6), {ncls} class / {nedge} edge candidates compared"
        # phases: flat (allowance), edge and feature (bit-equal), each on the positions the device had before it
        before = pos0
        ratio = None
        for ph, (kind, alpha) in enumerate((("flat", 1.0), ("edge", 0.2), ("feature", 1.0))):
            after = got[f"pos_after_{ph}"]
            sel = np.nonzero(cls == ph)[0]
            rest = np.setdiff1d(np.arange(m), sel)
            assert R.same_bits(after[rest], before[rest]).all(), (name, k, mode, kind, "moved a row of another class")
            c = dict(pos=before, n=fn, ev=edge, ci=sel, off=np.arange(len(sel) + 1, dtype=np.int64) * ku,
                     nbr=np.ascontiguousarray(got["knn"][sel, :ku]).reshape(-1), d=d, alpha=alpha)
            if kind == "flat" and len(sel):
                rows = before[c["nbr"]].astype(np.float64)
                red4 = got["red4_0"]
                assert red4[3] == len(rows), (name, k, red4[3], len(rows))
                np.testing.assert_allclose(red4[:3], rows.sum(0), rtol=1e-9, atol=1e-9 * np.abs(rows).sum(0).max())
                ctr = (red4[:3] / red4[3]).astype(F32)
                dd = before[c["nbr"]] - ctr
                delta = np.sqrt((((dd[:, 0] * dd[:, 0]) + (dd[:, 1] * dd[:, 1])).astype(F32) + dd[:, 2] * dd[:, 2]).max())
                assert got["delta_0"] == F32(delta), (name, k, got["delta_0"], delta)
                ref = R.oracle_step("flat", c, delta=F32(delta))
                ratio, _, _, _ = R.flat_new_allowance("flat", c, after[sel], ref)
                assert ratio <= 1.0, (name, k, mode, "flat", ratio)
                still = R.same_bits(ref, before[sel]).all(1)
                if delta == 0:
                    assert still.all() and R.same_bits(after[sel], before[sel]).all(), (name, k, "delta = 0 moved a row")
            elif len(sel):
                ref = R.oracle_step(kind, c)
                same = R.same_bits(after[sel], ref).all(1)
                assert same.all(), (name, k, mode, kind, sel[~same][:8], after[sel][~same][:2], ref[~same][:2])
            before = after
        lines.append(f"{mode}: {int((c1['u'] > 0).sum())} / {int((c2['u'] > 0).sum())} of {m} rows with undecided pairs "
                     f"in NVT1 / NVT2 (bound {int(0.02 * m)}), NVT2 {nvt2}, classes {np.bincount(cls, minlength=3).tolist()}"
                     f", flat deviation / allowance {ratio if ratio is None else round(ratio, 3)} (bound 1)")
        assert (c1["u"] > 0).mean() <= 0.02 and (c2["u"] > 0).mean() <= 0.02
    report(f"fused {name} k={k}: " + "; ".join(lines))


# ---------------------------------------------------------------------------------------------- (g) a NaN stays local
def test_fused_nan_normal_stays_local(gpu):
    """plane_exact with one NaN normal: one fused iteration against the clean run.  (A NaN POSITION is not a state of
    the fused loop: pcd_grid_build refuses non-finite coordinates; pcd_step_csr's NaN-position rows are in the step
    cases above.)  The vote of a NaN pair is `no`, but the tensor sums multiply the weight in (0 * NaN), on the device
    as in the reference: a NaN normal poisons NVT1 of every row that LISTS it (ring 1: their f_n is NaN), and through
    f_n NVT2 of every row that lists one of those (ring 2: NaN eigenvalues, which classify as 0 = flat, NaN being the
    maximum of the argmax).  Every row of this cloud is flat in the clean run too, so the flat selection, and with it
    the global centre and delta (positions only), is the same in both runs, and the edge and feature phases have no
    rows.  The flat step of a row reads f_n of the row and of its first k_update neighbours, all in its list.  So:
    f_n bit-equal outside ring 1; eigenvalues, sums of votes, classes AND the final positions bit-equal outside
    ring 2; inside ring 2 a row either took a NaN step (it keeps its position bit for bit) or saw no NaN among its
    update neighbours (it moves exactly as in the clean run); no position is NaN."""
    from test_gpu_stages import staged_iteration
    k, ku = 16, 8
    pos0, n0 = R.hard_cloud("plane_exact")
    rng = np.random.default_rng(5)
    n0 = n0 + F32(0.1) * rng.standard_normal(n0.shape).astype(F32)
    n0 = (n0 / np.linalg.norm(n0, axis=1, keepdims=True)).astype(F32)
    bad = 1234
    clean = staged_iteration(pos0, n0, 0.05, gpu, k=k, ku=ku)
    n1 = n0.copy()
    n1[bad] = np.nan
    got = staged_iteration(pos0, n1, 0.05, gpu, k=k, ku=ku)
    assert (got["knn"] == clean["knn"]).all()
    lists = clean["knn"][:, :k]
    ring1 = (lists == bad).any(1)
    ring2 = ring1 | ring1[lists].any(1)
    assert ring1[bad] and np.isnan(got["f_n"][ring1]).all(), "a listed NaN normal did not poison f_n"
    assert R.same_bits(got["f_n"][~ring1], clean["f_n"][~ring1]).all()
    assert R.same_bits(got["eig2"][~ring2], clean["eig2"][~ring2]).all()
    assert np.isnan(got["eig2"][ring2, :3]).all(), "a listed NaN f_n did not poison NVT2"
    assert (clean["classes"] == 0).all() and (got["classes"] == 0).all(), \
        (np.bincount(clean["classes"], minlength=3), np.bincount(got["classes"], minlength=3))
    same_pos = R.same_bits(got["pos"], clean["pos"]).all(1)
    assert same_pos[~ring2].all(), np.nonzero(~same_pos & ~ring2)[0][:8]
    stayed = R.same_bits(got["pos"], pos0).all(1)
    nan_upd = ring1[clean["knn"][:, :ku]].any(1) | ring1            # a NaN f_n among the row's update neighbours
    assert (stayed | same_pos)[ring2].all() and stayed[nan_upd].all() and same_pos[ring2 & ~nan_upd].all()
    assert np.isfinite(got["pos"]).all()
    report(f"NaN normal: {int(ring1.sum())} rows list the point (f_n NaN: all of them), {int(ring2.sum())} within two "
           f"rings (NaN eigenvalues, class flat: all of them); {int((~ring2).sum())} rows bit-equal to the clean run in "
           f"f_n, eigenvalues, classes and final positions (bound: all of them); {int(nan_upd.sum())} rows took a NaN "
           f"step and stayed (bound: all of them), 0 positions NaN")
