"""The references of tests/nvt_ref.py checked without a GPU: the vote judge against the golden NVT fixture, and the
host build of the kernels' per-point math (pcd_host_*: the same source the device compiles) against the admissible
candidates on every builder -- so that the GPU tests of test_gpu_nvt_edges.py cannot hide a failure behind a builder
that judges nothing, and so that every row carrying NaN, inf, an empty list or a zero tensor has gone through the
bounded loops of the host build before it is sent to a device."""
import math

import numpy as np
import pytest
import torch

import nvt_ref as R
import pcd_native as nat
from oracle import pcd_oracle as O

F32 = np.float32
KINDS = {"flat": nat.STEP_FLAT, "edge": nat.STEP_EDGE, "feature": nat.STEP_FEATURE, "corner": nat.STEP_CORNER,
         "new": nat.STEP_NEW, "dummy": nat.STEP_DUMMY}


def host_step(kind, c, delta):
    """pcd_host_step_csr on a ragged case (pcd_native.host_step_csr takes dense rows only)."""
    out = np.empty((len(c["ci"]), 3), F32)
    nbr = c["nbr"] if len(c["nbr"]) else np.zeros(1, np.int64)
    nat.check(nat.lib().pcd_host_step_csr(KINDS[kind], c["pos"].ctypes.data, c["n"].ctypes.data, c["ev"].ctypes.data,
                                          c["ci"].ctypes.data, c["off"].ctypes.data, nbr.ctypes.data, len(c["ci"]),
                                          float(delta), c["d"], c["alpha"], out.ctypes.data), "pcd_host_step_csr")
    return out


def oracle_votes(pos, n, ci, nbr, rho):
    """The float32 votes of oracle.better_filtered_nvt (its own expressions) on dense rows."""
    dv = pos[nbr] - pos[ci][:, None, :]
    dn = dv / np.maximum(O.norm3(dv)[..., None], F32(1e-12))
    c = np.abs(np.clip((dn * n[nbr]).sum(-1), -1, 1))
    return np.arccos(c) > F32(rho)


@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("rho_name,rho", [("a5pi12", math.pi * 5 / 12), ("api3", math.pi / 3)])
def test_judge_and_tensor_on_reference_fixture(golden, rho_name, rho, k):
    """The reference's own rows (steps.npz): the judge leaves at most 0.1 % of the pairs undecided, every decided vote
    is the oracle's, and tensor_f32 + O.eigh of those votes is the reference's decomposition bit for bit."""
    s = golden("steps")
    pos, n1 = s["pos"], s["n1"]
    knn = s[f"knn{k}"].astype(np.int64)
    m = len(knn)
    ci, off, nbr = np.arange(m), np.arange(m + 1, dtype=np.int64) * k, knn.reshape(-1)
    state = R.vote_judge(pos, n1, ci, off, nbr, rho)
    w = oracle_votes(pos, n1, ci, knn, rho).reshape(-1)
    und = state == R.UNDECIDED
    print(f"steps {rho_name} k={k}: {und.sum()} of {len(state)} pairs undecided ({und.mean():.2e}; bound 1e-3)")
    assert und.mean() <= 1e-3
    assert ((state == R.FORCED_IN) == w)[~und].all()
    t6, _ = R.tensor_f32(n1, (off, nbr), w)
    ew, ev = O.eigh(R.full3(t6))
    np.testing.assert_array_equal(ew, s[f"nvt_{rho_name}_k{k}_eigval"])
    np.testing.assert_array_equal(ev, s[f"nvt_{rho_name}_k{k}_eigvec"])
    cands = R.admissible_decompositions(n1, (off, nbr), state)
    assert len(cands["unjudged"]) == 0
    R.check_decompositions("fixture", cands, m, s[f"nvt_{rho_name}_k{k}_eigval"], s[f"nvt_{rho_name}_k{k}_eigvec"])


def test_host_votes_on_every_builder():
    """pcd_host_nvt_tensor + pcd_host_eigh3 on every vote builder at every rho: tensor, eigenvalues and eigenvectors
    bit-equal to an admissible candidate on every row; the builders' caps (no unjudged row, undecided pairs only where
    the builder aims at the threshold); an empty row has a NaN tensor and NaN eigenvalues (0 / 0)."""
    total_und = 0
    for label, rho, rows, may in R.vote_cases():
        pos, n, ci, off, nbr = rows
        state, cands = R.judge_rows(rho, rows, may)
        t6 = nat.host_nvt_tensor(pos, n, ci, off, nbr if len(nbr) else np.zeros(1, np.int64), rho)
        w, v = nat.host_eigh3(t6)
        print(R.check_decompositions(label, cands, len(ci), w, v, t6))
        empty = np.diff(off) == 0
        # 0 / 0: a NaN tensor, NaN eigenvalues, and the eigenvectors eigh makes of a NaN tensor (first row (1, 0, 0),
        # the rest NaN: bit-equal to the oracle's, checked above)
        assert np.isnan(t6[empty]).all() and np.isnan(w[empty]).all(), label
        assert (np.isnan(v[empty]).reshape(-1, 9).sum(1) == 6).all(), (label, v[empty])
        if label.startswith("threshold"):
            total_und += (cands["u"] > 0).sum()
            # (at rho = 0.3 two ulps of acosf are less than one ulp of c: the axis rows are all decided there)
            assert (cands["u"][:8] > 0).sum() >= (4 if 1.0 <= rho <= math.pi / 2 else 0), (label, cands["u"][:8])
    assert total_und > 1000


def test_builders_reach_their_branches():
    """The rows aim where they say: threshold rows straddle the threshold, scale rows cross the kernels' guards,
    fallback rows have no voter / one voter / only copies."""
    rho = math.pi * 5 / 12
    pos, n, ci, off, nbr = R.threshold_rows(rho)
    st = R.vote_judge(pos, n, ci, off, nbr, rho).reshape(-1, 32)
    assert ((st[:8] == R.FORCED_IN).any(1) & (st[:8] == R.FORCED_OUT).any(1) & (st[:8] == R.UNDECIDED).any(1)).all()
    pos, n, ci, off, nbr, near = R.scale_rows(rho)
    sq = (pos[nbr].astype(F32) ** 2).sum(1, dtype=F32)
    assert (sq == 0).any() or (sq < 2.0 ** -126).any()
    assert (sq[sq > 0] < 1e-24).any() and (sq >= 1e30).any() and np.isfinite(sq).all() and near.sum() >= 20
    pos, n, ci, off, nbr = R.fallback_rows()
    st = R.vote_judge(pos, n, ci, off, nbr, rho)
    votes = np.bincount(R.segments(off)[st == R.FORCED_IN], minlength=len(ci))
    lens = np.diff(off)
    assert sorted(set(lens)) == [0] + list(R.FALLBACK_LENGTHS) and lens[-1] == 0 and (lens[:-1] == 0).sum() == 1
    assert ((votes == 0) & (lens > 0)).sum() == 8 and ((votes == 1) & (lens > 1)).sum() >= 7
    assert (votes == lens)[lens > 0].sum() >= 8


@pytest.mark.parametrize("rho", R.NORMAL_RHOS)
def test_normal_judge_and_tensors_match_oracle(rho):
    """CPSD: the oracle's normal-filtered NVT and PVT (float32, its own votes) are one admissible candidate of
    normal_vote_judge + normal_tensor_f32 / cov_f32 on every row of normal_rows: voters only past member 64, only
    before it, nowhere, members at the float32 neighbours of cos(rho), empty rows."""
    pos, n, ci, off, nbr = R.normal_rows(rho)
    may = np.zeros(len(nbr), bool)
    c = n[nbr] @ np.array([1, 0, 0], F32)
    may[np.abs(c - F32(math.cos(F32(rho)))) < 1e-6] = True
    for kind, ref in (("normal", lambda: O.normal_filtered_nvt(n, ci, off, nbr, rho)),
                      ("pvt", lambda: O.normal_filtered_pvt(pos, n, ci, off, nbr, rho))):
        state, cands = R.judge_rows(rho, (pos, n, ci, off, nbr), may, kind)
        w, v = ref()
        print(R.check_decompositions(f"oracle {kind} rho={rho}", cands, len(ci), w, v))
        assert (cands["u"] > 0).sum() >= (4 if rho == 0.9 else 0)    # (at 0.3 two ulps of acosf are less than one of c)
    st = R.normal_vote_judge(n, ci, off, nbr, rho)
    seg, t = R.segments(off), np.arange(len(nbr)) - off[R.segments(off)]
    vin = st == R.FORCED_IN
    late_only = [r for r in range(len(ci)) if vin[(seg == r) & (t >= 64)].any() and not vin[(seg == r) & (t < 64)].any()]
    early_only = [r for r in range(len(ci)) if off[r + 1] - off[r] > 64 and vin[(seg == r) & (t < 64)].any()
                  and not (st[(seg == r) & (t >= 64)] != R.FORCED_OUT).any()]
    assert len(late_only) >= 3 and len(early_only) >= 3, (late_only, early_only)


def test_host_eigh_on_eigen_cases():
    """pcd_host_eigh3 returns on every case (NaN, inf, zero, subnormal scales: the QL loop is bounded) and is bit-equal
    to O.eigh, NaN pattern included."""
    names, t6 = R.eigen_cases()
    w, v = nat.host_eigh3(t6)
    rw, rv = O.eigh(R.full3(t6))
    bad = ~(R.same_bits(w, rw).all(1) & R.same_bits(v, rv).reshape(len(w), -1).all(1))
    assert not bad.any(), [(names[i], w[i], rw[i]) for i in np.nonzero(bad)[0][:5]]
    nan_in = np.isnan(t6).any(1)
    assert nan_in.sum() == 2 and np.isnan(rw[nan_in]).any(1).all()


def test_host_vu_smooth_on_vu_cases():
    """pcd_host_vu_smooth bit-equal to O.vu_smoothed_normals on every tie pattern, at tau and its neighbours, on n = 0
    and NaN, and on the exact cancellation (0 / 0: NaN in both)."""
    for name, w, E, n, tau, damp in R.vu_cases():
        with np.errstate(all="ignore"):
            ref = O.vu_smoothed_normals(w, E, n, tau, damp)
        got = nat.host_vu_smooth(w, E, n, tau, damp)
        assert R.same_bits(got, ref).all(), (name, got[:2], ref[:2])
        if name.startswith("cancel") or name == "n_zero":
            assert np.isnan(ref).all(), name
    # the tie cases do depend on the order: reversing the stable order changes the reference's own output
    name, w, E, n, tau, damp = R.vu_cases()[2]
    assert name == "aab_split"
    flipped = O.vu_smoothed_normals(w[:, [1, 0, 2]], E[:, :, [1, 0, 2]], n, tau, damp)
    assert not R.same_bits(flipped, O.vu_smoothed_normals(w, E, n, tau, damp)).all()


def test_oracle_classes_follow_torch_argmax():
    """O.classes (numpy argmax) has torch.argmax's rule on every class case: NaN is the maximum, the first index wins
    ties -- the rule the kernels' classify restates."""
    names, w = R.class_cases()
    for scale in R.CLASS_SCALES:
        with np.errstate(all="ignore"):
            p, l, s = O.nvt_features(w)
            f = np.stack([p * F32(scale), l, s], 1)
            ref = O.classes(w, scale)
        tor = torch.argmax(torch.from_numpy(f), dim=1).numpy()
        assert (ref == tor).all(), [(names[i], f[i], ref[i], tor[i]) for i in np.nonzero(ref != tor)[0][:5]]
    with np.errstate(all="ignore"):
        p, l, s = O.nvt_features(w)
    ties = [i for i, nm in enumerate(names) if "==" in nm]
    assert len(ties) >= 5
    i = names.index("0.2pla==lin#0")
    assert (p[i] * F32(0.2)).astype(F32) == l[i] and O.classes(w[i:i + 1], 0.2)[0] == 0


@pytest.mark.parametrize("kind", R.STEP_KINDS)
def test_host_steps_on_step_cases(kind):
    """pcd_host_step_csr on every step case: edge, feature and corner bit-equal to the oracle (the singular rows keep
    v_i, and the oracle's info mask is False exactly there), the analytic clamp outputs, flat and new within 8 x the
    oracle's own float32 deviation from float64."""
    for c in R.step_cases(kind):
        label = f"{kind}/{c['name']}"
        delta = R.device_delta(c["pos"], c["nbr"])[1] if kind in ("flat", "new") else 0.0
        got = host_step(kind, c, delta)
        ref = R.oracle_step(kind, c)
        vi = c["pos"][c["ci"]]
        if "expect" in c:
            assert R.same_bits(got, c["expect"]).all(), (label, got, c["expect"])
            assert R.same_bits(ref, c["expect"]).all(), (label, ref, c["expect"])
        if kind in ("edge", "feature", "corner"):
            assert R.same_bits(got, ref).all(), (label, np.nonzero(~R.same_bits(got, ref).all(1))[0][:8])
            if c["singular"] is not None:
                ok = R.oracle_ok(kind, c)
                assert (ok == ~c["singular"]).all(), (label, np.nonzero(ok == c["singular"])[0])
                assert R.same_bits(got[c["singular"]], vi[c["singular"]]).all(), label
        elif kind in ("flat", "new"):
            ratio, dev, bound, fin = R.flat_new_allowance(kind, c, got, ref)
            print(f"{label}: host deviation / allowance {ratio:.3f} (bound 1)")
            assert ratio <= 1.0, (label, ratio)
            still = R.same_bits(ref, vi).all(1)
            if "nan_rows" not in c:
                assert R.same_bits(got[still], vi[still]).all(), (label, np.nonzero(still)[0])
        else:
            assert R.same_bits(got, vi).all(), label


@pytest.mark.parametrize("name", R.FUSED_CLOUDS)
def test_fused_cloud_caps(name):
    """The hard clouds of the fused comparison judge enough: at k = 16 and 32 at most 2 % of the rows have an undecided
    pair (NVT1 on the given normals, NVT2 on the smoothed ones) and at most 10 % lack a class margin -- from the
    reference alone, on the brute-force float32 lists."""
    for k in (16, 32):
        u1, u2, nomargin = R.fused_reference_caps(name, k)
        print(f"{name} k={k}: rows with undecided pairs NVT1 {u1:.4f} NVT2 {u2:.4f} (bound 0.02), without a class "
              f"margin {nomargin:.4f} (bound 0.10)")
        assert u1 <= 0.02 and u2 <= 0.02 and nomargin <= 0.10, (name, k, u1, u2, nomargin)
