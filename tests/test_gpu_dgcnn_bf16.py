"""The opt-in bf16-operand inference mode of DGCNN / BetterDGCNN on the device (csrc/dgcnn.hip: gemm_bf16_kernel,
fused_edge_bf16_kernel; include/pcd.h, "bf16 operands").

The yardstick is tests/dgcnn_bf16_ref.py: the float64 restatement with the GEMM operands rounded to bf16 where the
device rounds them.  The kernel is checked exactly on integers, then against the float64 product of CPU-rounded
operands within the project's chain bound; the network is checked stage by stage on the device's own intermediate
tensors (a value on the other side of a bf16 rounding boundary moves the next layer by 2^-8 relative, so nothing is
compared end to end with injected lists), and end to end against the reference's goldens within a multiple of what the
bf16 restatement itself deviates -- computed by dgcnn_bf16_ref.golden_numbers, never a constant.  No patch is excluded.
Measured figures are reported (conftest.report) before they are asserted.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import better_dgcnn_cases as bcases
import dgcnn_bf16_ref as bf
import dgcnn_cases as cases
import dgcnn_train_ref as tref
import patch_cases
from conftest import report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.fixture(scope="module")
def mods(gpu):
    import pcd_native as nat
    from PatchGeneration.Modules.Mesh import Mesh
    from PatchGeneration.Modules.Network.GCNModel import DGCNN, BetterDGCNN
    from PatchGeneration.Modules.PatchCollector import PatchCollector
    return {"nat": nat, "DGCNN": DGCNN, "BetterDGCNN": BetterDGCNN, "Mesh": Mesh, "PatchCollector": PatchCollector,
            "dev": gpu}


def torch_state(state):
    return {key: torch.as_tensor(np.asarray(v)) for key, v in state.items()}


def new_model(mods, k, emb, operands, trainable=False, dropout=0.5):
    m = mods["DGCNN"](k, 17, emb, dropout, trainable=trainable, operands=operands)
    m.load_state_dict(torch_state(cases.make_state(cases.SEED, k, emb)), strict=True)
    return m.to(mods["dev"]).eval()


def model_for(mods, k, emb, operands="bf16"):
    return cached(("model", k, emb, operands), lambda: new_model(mods, k, emb, operands))


def better_model_for(mods, name, operands="bf16"):
    def make():
        t = bcases.Table(name)
        m = mods["BetterDGCNN"](t.l_e, t.l_d, t.l_l, t.sizes, t.k, 17, 0.5, operands=operands)
        m.load_state_dict(torch_state(bcases.make_state(name)), strict=True)
        return m.to(mods["dev"]).eval()
    return cached(("better", name, operands), make)


def fixture(golden, name):
    return cached(("inputs", name), lambda: cases.fixture_inputs(golden, name))


def ellipsoid(mods, golden, n):
    return torch.as_tensor(fixture(golden, "ellipsoid")[0][:n], dtype=torch.float32).to(mods["dev"])


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. exact on integers
SHAPES = [(64, 17, 1), (3, 64, 5), (130, 1024, 2), (512, 256, 33), (128, 40, 1)]


def _int_operands(M, K, b):
    m, k = np.arange(M)[:, None], np.arange(K)[None, :]
    w = ((5 * m + 3 * k + (m * k) % 7) % 7 - 3).astype(np.float32)              # asymmetric, in [-3, 3]
    e = np.arange(b * K * 64).reshape(b, K, 64)
    x = ((e * 7 + e // 5) % 9 - 4).astype(np.float32)                           # integers in [-4, 4]
    s = np.array([0.5, -1.0, 2.0, 1.0, -0.25])[np.arange(M) % 5].astype(np.float32)
    t = ((np.arange(M) * 3) % 11 - 5).astype(np.float32)
    return w, x, s, t


def _lrelu32(v):
    """LeakyReLU(0.2) as float32 computes it, on float64 values that are float32 numbers."""
    return np.where(v > 0, v, (np.float64(np.float32(0.2)) * v).astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("M,K,b", SHAPES)
def test_gemm_bf16_is_exact_on_integers(mods, M, K, b):
    """Small integers are bf16 numbers and every partial sum stays below 2^24: exact in any summation order."""
    nat, dev = mods["nat"], mods["dev"]
    w, x, s, t = _int_operands(M, K, b)
    assert np.array_equal(bf.round_bf16(w), w) and np.array_equal(bf.round_bf16(x), x)
    y = np.einsum("mk,bkn->bmn", w.astype(np.float64), x.astype(np.float64))
    assert np.einsum("mk,bkn->bmn", np.abs(w).astype(np.float64), np.abs(x).astype(np.float64)).max() < 2 ** 24
    affine = s.astype(np.float64)[:, None] * y + t.astype(np.float64)[:, None]  # exact: s is a power of two
    wd, xd, sd, td = (torch.as_tensor(a).to(dev) for a in (w, x, s, t))
    got = {e: nat.dgcnn_gemm_bf16(wd, xd, e, sd, td).cpu().numpy().astype(np.float64)
           for e in (nat.EPI_PLAIN, nat.EPI_AFFINE_LRELU, nat.EPI_AFFINE)}
    np.testing.assert_array_equal(got[nat.EPI_PLAIN], y)
    np.testing.assert_array_equal(got[nat.EPI_AFFINE], affine)
    np.testing.assert_array_equal(got[nat.EPI_AFFINE_LRELU], _lrelu32(affine))
    act = _lrelu32(affine).astype(np.float32)                                   # [b, M, 64]
    # the kernel's order: 4 runs of 16 columns summed in column order, then (q0 + q1) + (q2 + q3)
    q = np.zeros((b, M, 4), np.float32)
    for c in range(16):
        q = q + act.reshape(b, M, 4, 16)[..., c]
    mean = ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) * np.float32(1 / 64)
    pooled = nat.dgcnn_gemm_bf16(wd, xd, nat.EPI_POOL, sd, td).cpu().numpy()
    assert pooled.shape == (b, 2 * M)
    np.testing.assert_array_equal(pooled[:, :M], act.max(-1))
    np.testing.assert_array_equal(pooled[:, M:], mean)


# ------------------------------------------------------------------------------------------------ 2. the rounding
@pytest.mark.parametrize("M,K,b", SHAPES)
def test_gemm_bf16_rounds_as_stated(mods, M, K, b):
    """Random float32 operands, NaN and Inf among them: the device's product is the float64 product of the operands
    rounded on the CPU (nearest even) within the chain bound (K + 16) 2^-24 sum |w~| |x~|, which holds for any order
    of float32 additions of the (exact) products; NaN and Inf land where the float64 product has them."""
    nat, dev = mods["nat"], mods["dev"]
    rng = np.random.default_rng([M, K, b, 2])
    w = (rng.uniform(-1, 1, (M, K)) * np.sqrt(3.0 / K)).astype(np.float32)
    x = rng.normal(0.0, 1.0, (b, K, 64)).astype(np.float32)
    x[0, K // 2, 5] = np.nan                                                    # column 5 of patch 0
    x[b - 1, K - 1, 7] = np.inf                                                 # column 7 of the last patch, last k
    x[b - 1, 0, 9] = -np.inf
    w[M - 1, 0] = np.inf                                                        # the last row, against every column
    wr, xr = bf.round_bf16(w), bf.round_bf16(x)
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.einsum("mk,bkn->bmn", wr, xr)
        mag = np.einsum("mk,bkn->bmn", np.abs(wr), np.abs(xr))
    got = nat.dgcnn_gemm_bf16(torch.as_tensor(w).to(dev), torch.as_tensor(x).to(dev)).cpu().numpy().astype(np.float64)
    finite = np.isfinite(want)
    assert np.isnan(want).any() and np.isinf(want).any() and finite.any()
    ratio = float((np.abs(got - want)[finite] / ((K + 16) * U * mag[finite])).max())
    report(f"gemm_bf16 M={M} K={K} b={b}: max |device - float64 product of the rounded operands| / "
           f"((K + 16) 2^-24 sum |w~||x~|) = {ratio:.4f}")
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])            # Inf with its sign
    assert np.isfinite(got[finite]).all() and ratio <= 1.0


# ------------------------------------------------------------------------------------------------ 3. edge layer
@pytest.mark.parametrize("layer", [1, 3, 4, 6])
@pytest.mark.parametrize("b", [1, 3])
def test_edgeconv_against_bf16_restatement(mods, layer, b):
    nat, dev = mods["nat"], mods["dev"]
    model = model_for(mods, 8, 128)
    assert model.operands == "bf16" and model.native().operands == "bf16"
    state = cases.make_state(cases.SEED, 8, 128)
    cin = cases.EDGE[layer - 1][0]
    rng = np.random.default_rng([layer, b])
    x = rng.normal(0.0, 1.0, (b, cin, 64)).astype(np.float32)
    xd = torch.as_tensor(x).to(dev)
    if layer <= 3:
        lists = rng.integers(0, 64, (b, 64, 3)).astype(np.int32)
    else:
        lists = nat.dgcnn_knn(xd, 8).cpu().numpy()                              # the device's own lists
    ld = torch.as_tensor(lists).to(dev)
    got_d = model.native().edgeconv(layer, xd, ld)
    got = got_d.cpu().numpy().astype(np.float64)
    l64 = lists.astype(np.int64)
    want = bf.edge_layer(state, layer, x, l64, "bf16")
    bound = (2 * cin + 16) * U * bf.edge_bound(state, layer, x, l64, "bf16")
    ratio = float((np.abs(got - want) / bound).max())
    report(f"bf16 edgeconv layer {layer} b={b}: max |device - bf16 restatement| / ((2 Cin + 16) 2^-24 M) = {ratio:.3f}")
    assert got.shape == want.shape and ratio <= 1.0
    f32 = model_for(mods, 8, 128, "fp32").native().edgeconv(layer, xd, ld)
    if layer == 1:                                                              # Cin = 17 stays on the float32 kernel
        assert torch.equal(bits(got_d), bits(f32))
    else:
        assert not torch.equal(bits(got_d), bits(f32))


# ------------------------------------------------------------------------------------------------ 4. fused
@pytest.mark.parametrize("cin,cout,n", [(17, 16, 3), (32, 32, 8), (64, 64, 64)])
@pytest.mark.parametrize("b", [1, 3])
def test_fused_bf16_edge_layer_is_the_two_kernel_path_bit_for_bit(mods, cin, cout, n, b):
    nat, dev = mods["nat"], mods["dev"]
    rng = np.random.default_rng([cin, cout, n, b, 16])
    w = (rng.uniform(-1, 1, (cout, 2 * cin)) * np.sqrt(3.0 / (2 * cin))).astype(np.float32)
    s = (rng.uniform(0.5, 1.5, cout) * np.where(rng.random(cout) < 0.1, -1, 1)).astype(np.float32)
    t = rng.normal(0, 0.2, cout).astype(np.float32)
    x = rng.normal(0.0, 1.0, (b, cin, 64)).astype(np.float32)
    x[b - 1, :, 9] = np.nan                                                     # node 9 of the last patch
    lists = rng.integers(0, 64, (b, 64, n)).astype(np.int32)
    args = [torch.as_tensor(a).to(dev) for a in (w, s, t, x, lists)]
    off = nat.bdgcnn_edgeconv(*args, fused=nat.FUSED_OFF, operands="bf16")
    on = nat.bdgcnn_edgeconv(*args, fused=nat.FUSED_ON, operands="bf16")
    auto = nat.bdgcnn_edgeconv(*args, fused=nat.FUSED_AUTO, operands="bf16")
    scratch = torch.empty(nat.bdgcnn_edgeconv_scratch_bytes(cin, cout, b), dtype=torch.uint8, device=dev)
    for mode in (nat.FUSED_OFF, nat.FUSED_ON):                                  # the float32 entry's scratch size serves
        got = nat.bdgcnn_edgeconv(*args, fused=mode, scratch=scratch, out=torch.empty_like(off), operands="bf16")
        torch.cuda.synchronize()
        assert torch.equal(bits(got), bits(off))
    assert torch.equal(bits(on), bits(off)) and torch.equal(bits(auto), bits(off))      # bits, NaNs included
    assert bool(torch.isnan(off[b - 1]).any()) and bool(torch.isfinite(off[:b - 1]).all())
    # and it is the bf16 product: the restatement's layer with these weights, whatever Cin is
    state = {"conv1.0.weight": w, "bn1.weight": s, "bn1.bias": t, "bn1.running_mean": np.zeros(cout, np.float32),
             "bn1.running_var": np.ones(cout, np.float32) - np.float32(1e-5)}
    ok = np.ones(b, bool)
    ok[b - 1] = False
    l64 = lists.astype(np.int64)
    if ok.any():
        # (s here is gamma / sqrt(var + eps) with var + eps = 1 to float32 rounding: half a unit of the bound's 16)
        want = bf.edge_layer(state, 1, x[ok], l64[ok], "bf16", min_cin=1)
        bound = (2 * cin + 16) * U * bf.edge_bound(state, 1, x[ok], l64[ok], "bf16", min_cin=1)
        assert float((np.abs(off.cpu().numpy()[ok] - want) / bound).max()) <= 1.0


# ------------------------------------------------------------------------------------------------ 5. chained stages
def _check_knn(x, lists, k, what):
    """x [b, C, 64], lists int [b, 64, k] on the device: every row's set is the k nearest within the rounding bound of
    the float32 distances (tests/test_gpu_dgcnn.py's check)."""
    x = x.to(torch.float64)
    d = x[:, :, :, None] - x[:, :, None, :]
    D = (d * d).sum(1)
    norm = torch.linalg.vector_norm(x, dim=1)
    bi = (x.size(1) + 4) * U * ((norm[:, :, None] + norm[:, None, :]) ** 2).amax(-1)
    lists = lists.to(torch.int64)
    assert int(lists.min()) >= 0 and int(lists.max()) <= 63
    member = torch.zeros_like(D, dtype=torch.bool).scatter_(2, lists, True)
    assert bool((member.sum(-1) == k).all()), f"{what}: a row's list does not have {k} distinct members"
    dl = torch.gather(D, 2, lists)
    assert bool((dl[..., :-1] - dl[..., 1:] <= 2 * bi[..., None]).all()), f"{what}: a list is not ascending"
    assert bool(((dl[..., :-1] != dl[..., 1:]) | (lists[..., :-1] < lists[..., 1:])).all()), \
        f"{what}: a tie is not in index order"
    inf = torch.full_like(D, float("inf"))
    over = (torch.where(member, D, -inf).amax(-1) - torch.where(member, inf, D).amin(-1)).clamp_min(0.0)
    return float(torch.where(over > 0, over / (2 * bi).clamp_min(1e-300), over).max())


def _network(mods, golden, which, name):
    """(net, state, model, golden npz, inputs float64 [n, 20, 64]) of a DGCNN or BetterDGCNN configuration."""
    if which == "dgcnn":
        k, emb, fx, _ = cases.CONFIGS[name]
        g = golden(f"dgcnn_{name}")
        return bf.Net.dgcnn(k, emb), cases.make_state(cases.SEED, k, emb), model_for(mods, k, emb), g, \
            fixture(golden, fx)[0][g["rows"]]
    g = golden(f"better_dgcnn_{name}")
    return bf.Net.better(name), bcases.make_state(name), better_model_for(mods, name), g, \
        fixture(golden, bcases.FIXTURE)[0][g["rows"]]


def device_run(mods, golden, which, name):
    """One debug forward in bf16 mode: (out float64, debug dict of numpy arrays, the device's cat and lists)."""
    def make():
        _, _, model, _, x = _network(mods, golden, which, name)
        out, dbg = model(torch.as_tensor(x, dtype=torch.float32).to(mods["dev"]), debug=True)
        torch.cuda.synchronize()
        return out.cpu().numpy().astype(np.float64), {key: v.cpu().numpy() for key, v in dbg.items()}, dbg
    return cached(("run", which, name), make)


def _chunks(n, fn, size=16):
    """fn(slice) over the patches in chunks (the [b, C, 64, k] gathers of an edge layer stay small)."""
    return np.concatenate([fn(slice(s, min(s + size, n))) for s in range(0, n, size)])


CHAINED = [("dgcnn", name) for name in cases.CONFIGS] + [("better", "narrow"), ("better", "default")]


@pytest.mark.parametrize("which,name", CHAINED)
def test_stages_against_bf16_restatement_on_the_devices_own_tensors(mods, golden, which, name):
    net, state, model, g, x = _network(mods, golden, which, name)
    out, dbg, dbg_dev = device_run(mods, golden, which, name)
    x32 = x.astype(np.float32)
    cat = dbg["cat"].astype(np.float64)
    n = len(x)
    worst = {}
    for l in range(net.E):
        xin = net.layer_input(l, x32, cat).astype(np.float64)
        nbr = net.list_of(l, x32, dbg["lists"])
        got = cat[:, net.cat_off[l]:net.cat_off[l + 1]]
        ratio = _chunks(n, lambda c: (np.abs(got[c] - bf.edge_layer(state, l + 1, xin[c], nbr[c], "bf16")) /
                                      ((2 * net.cin[l] + 16) * U * bf.edge_bound(state, l + 1, xin[c], nbr[c], "bf16"))
                                      ).reshape(c.stop - c.start, -1).max(-1))
        worst[f"conv{l + 1}"] = float(ratio.max())
        if l >= net.l_e:                                                        # the search ran on this float32 input
            xd = torch.as_tensor(x32[:, :17]).to(mods["dev"]) if l == 0 else \
                dbg_dev["cat"][:, net.cat_off[l - 1]:net.cat_off[l]]
            slack = _check_knn(xd, dbg_dev["lists"][l - net.l_e], net.k, f"{name} layer {l + 1}")
            worst[f"knn{l + 1}"] = slack
    pooled = dbg["pooled"].astype(np.float64)
    ratio = np.abs(pooled - bf.pooled_layer(state, net.E + 1, cat, "bf16")) / \
        ((net.ccat + 16 + 64) * U * bf.pooled_bound(state, net.E + 1, cat, "bf16"))
    worst["pooled"] = float(ratio.max())
    head_dev = float(np.abs(out - bf.head(net, state, pooled)[0]).max())
    tol = 8.0 * float(g["dev32_stable"])
    report(f"bf16 {which} {name}, {n} patches, each stage on the device's own input and lists: error / bound "
           + ", ".join(f"{key} {v:.3f}" for key, v in worst.items())
           + f"; head max |dout| {head_dev:.2e} (allowed {tol:.2e}), ratio {head_dev / tol:.3f}")
    assert all(v <= 1.0 for v in worst.values()), worst
    assert head_dev <= tol


# ------------------------------------------------------------------------------------------------ 6. end to end
@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_forward_bf16_against_reference_golden(mods, golden, name):
    """Nothing injected.  The maximum over patches may be 8 x the bf16 restatement's on the same rows (the factor the
    project gives a maximum over a discontinuous quantity: the device and the restatement flip different neighbours,
    and one flip costs as much as all the rounding); the median does not see single flips: 2 x."""
    g = golden(f"dgcnn_{name}")
    out, _, _ = device_run(mods, golden, "dgcnn", name)
    numbers = bf.golden_numbers(golden, name)
    dev = np.abs(out - g["out64"]).max(-1)
    angle = bf.angles_deg(out, g["out64"])
    r_max, r_med = float(dev.max()) / numbers["max_dev"], float(np.median(dev)) / numbers["med_dev"]
    report(f"bf16 {name}: device vs the reference's float64 outputs, {len(dev)} patches, nothing injected: |dout| max "
           f"{dev.max():.2e} = {r_max:.2f} x the bf16 restatement's {numbers['max_dev']:.2e} (allowed 8 x), median "
           f"{np.median(dev):.2e} = {r_med:.2f} x its {numbers['med_dev']:.2e} (allowed 2 x); angle max "
           f"{angle.max():.3f} deg median {np.median(angle):.3f} deg (restatement {numbers['max_angle']:.3f} / "
           f"{numbers['med_angle']:.3f})")
    assert r_max <= 8.0
    assert r_med <= 2.0


# ------------------------------------------------------------------------------------------------ 7. invariants
def test_bf16_bits_do_not_depend_on_the_batch(mods, golden):
    model = model_for(mods, 8, 128)
    x = ellipsoid(mods, golden, 33)
    one = model(x[5:6])
    assert torch.equal(model(x[5:6]), one)                                      # run to run
    assert torch.equal(model(torch.cat([x[5:6], x[0:1]]))[0:1], one)            # row 0 of 2
    big = torch.cat([x[:32], x[5:6]])
    got = model(big)
    assert torch.equal(got[32:33], one)                                         # row 32 of 33
    assert torch.equal(got, model(big)) and torch.equal(got[5:6], one)
    assert not torch.equal(one, model_for(mods, 8, 128, "fp32")(x[5:6]))        # (and it is the other arithmetic)
    better = better_model_for(mods, "narrow")                                   # the fused kernel
    one = better(x[5:6])
    assert torch.equal(better(torch.cat([x[:32], x[5:6]]))[32:33], one) and torch.equal(better(x[5:6]), one)


def test_bf16_nan_stays_in_its_patch(mods, golden):
    for model in (model_for(mods, 8, 128), better_model_for(mods, "narrow")):
        x = ellipsoid(mods, golden, 3)
        clean = model(x)
        for bad in (float("nan"), float("inf")):
            y = x.clone()
            y[1, 4, 7] = bad
            out = model(y)
            assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])
            assert not bool(torch.isfinite(out[1]).all())
        assert torch.equal(model(x), clean)


def test_bf16_index_refusal_and_deferred_flag(mods, golden):
    nat, dev = mods["nat"], mods["dev"]
    model = model_for(mods, 8, 128)
    x = ellipsoid(mods, golden, 4)
    clean = model(x)
    y = x.clone()
    y[2, 18, 40] = 64.0
    y[1, 19, 3] = float("nan")
    with pytest.raises(ValueError, match="patch 1 "):
        model(y)
    torch.cuda.synchronize()
    flag = torch.full((1,), nat.DGCNN_NO_BAD_PATCH, dtype=torch.int32, device=dev)
    assert torch.equal(model(x, first_bad=flag, patch_base=100), clean) and int(flag) == nat.DGCNN_NO_BAD_PATCH
    out = model(y, first_bad=flag, patch_base=100)
    assert int(flag) == 101
    assert torch.equal(out[0], clean[0]) and torch.equal(out[3], clean[3]) and bool(torch.isfinite(out).all())
    assert torch.equal(model(x), clean)


# ------------------------------------------------------------------------------------------------ 8. nothing else moves
def test_switching_back_gives_the_fp32_bits(mods, golden):
    x = ellipsoid(mods, golden, 5)
    never = model_for(mods, 8, 128, "fp32")
    want32, want16 = never(x), model_for(mods, 8, 128)(x)
    m = new_model(mods, 8, 128, "fp32")
    assert m.operands == "fp32" and torch.equal(m(x), want32)
    assert m.native().workspace_bytes(5) == never.native().workspace_bytes(5)
    m.set_operands("bf16")
    assert m.operands == "bf16" and m.native().operands == "bf16"
    assert m.native().workspace_bytes(5) == never.native().workspace_bytes(5)
    assert torch.equal(m(x), want16) and not torch.equal(want16, want32)
    m.set_operands("fp32")
    assert torch.equal(m(x), want32)
    m.set_operands("bf16")                                                      # the rounded weights are kept
    assert torch.equal(m(x), want16)
    with pytest.raises(ValueError, match="operands"):
        m.set_operands("fp16")
    assert torch.equal(m(x), want16)
    for name in ("narrow", "default"):                                          # a table from the caller, fused layers
        b16, b32 = better_model_for(mods, name), better_model_for(mods, name, "fp32")
        assert b16.native().workspace_bytes(7) == b32.native().workspace_bytes(7)
        assert not torch.equal(b16(x), b32(x))


def test_bf16_survives_load_state_dict(mods, golden):
    x = ellipsoid(mods, golden, 4)
    m = new_model(mods, 8, 128, "bf16")
    first = m(x)
    other = torch_state(cases.make_state(cases.SEED + 1, 8, 128))
    m.load_state_dict(other, strict=True)
    fresh = mods["DGCNN"](8, 17, 128, 0.5, operands="bf16")
    fresh.load_state_dict(other, strict=True)
    fresh = fresh.to(mods["dev"]).eval()
    got = m(x)
    assert m.operands == "bf16" and m.native().operands == "bf16"
    assert torch.equal(got, fresh(x)) and not torch.equal(got, first)
    fresh.set_operands("fp32")
    assert not torch.equal(fresh(x), got)
    with torch.no_grad():
        m.linear4.bias += 1.0                                                   # an in-place write re-packs, in bf16
    assert m.native().operands == "bf16" and float((m(x) - (got + 1.0)).abs().max()) <= 1e-6
    assert m.cpu().to(mods["dev"]).native().operands == "bf16"


def test_training_ignores_the_setting(mods, golden):
    k, emb, fx = tref.CONFIGS["k1_b2_ellipsoid"][:3]
    g = golden("dgcnn_train_k1_b2_ellipsoid")
    x = torch.as_tensor(fixture(golden, fx)[0][g["rows"]], dtype=torch.float32).to(mods["dev"])
    gt = torch.as_tensor(g["gt"], dtype=torch.float32).to(mods["dev"])
    got = {}
    for operands in ("fp32", "bf16"):
        m = new_model(mods, k, emb, operands, trainable=True, dropout=0.0)
        m(x)                                                                    # eval() first: the bf16 weights exist
        m.train()
        out = m(x)
        ones = torch.ones(len(out), dtype=torch.float32, device=out.device)
        (tref.LOSS_WEIGHTS[0] * F.cosine_embedding_loss(out, gt, ones) + tref.LOSS_WEIGHTS[1] * F.mse_loss(out, gt)).backward()
        torch.cuda.synchronize()
        got[operands] = (out.detach(), {key: p.grad for key, p in m.named_parameters()},
                         {key: v.clone() for key, v in m.named_buffers()})
    (o32, g32, b32), (o16, g16, b16) = got["fp32"], got["bf16"]
    assert torch.equal(o32, o16)
    assert set(g32) == set(g16) and all(g16[key] is not None and torch.equal(g32[key], g16[key]) for key in g32)
    assert set(b32) == set(b16) and all(torch.equal(b32[key], b16[key]) for key in b32)


# ------------------------------------------------------------------------------------------------ 9. pipeline
def test_predict_normals_with_a_bf16_model(mods):
    g = patch_cases.load_golden("ellipsoid")
    res = {}
    for operands in ("fp32", "bf16"):
        mesh = mods["Mesh"](g["v"].copy(), g["f"].copy())
        pc = mods["PatchCollector"](mesh, int(g["k"]))
        res[operands] = pc.predictNormals(model_for(mods, 8, 128, operands), batch_faces=100)
    (n32, f32), (n16, f16) = res["fp32"], res["bf16"]
    assert f16 == f32 and n16.shape == n32.shape == (320, 3) and n16.dtype == torch.float64 and n16.is_cuda
    assert bool((torch.linalg.vector_norm(n16, dim=1) - 1).abs().max() < 1e-12)
    angle = torch.rad2deg(torch.acos((n16 * n32).sum(1).clamp(-1.0, 1.0)))
    report(f"predictNormals on the ellipsoid, bf16 model vs fp32 model, 320 faces, {f16} fallbacks each: angle between "
           f"the normals median {float(angle.median()):.3f} deg, max {float(angle.max()):.3f} deg (not gated)")
    # Mesh.denoise takes them as they are
    mesh = mods["Mesh"](g["v"].copy(), g["f"].copy())
    out = mesh.denoise(guided_normals=n16, normal_iterations=1, vertex_iterations=1)
    assert np.isfinite(np.asarray(out)).all() and np.isfinite(mesh.v).all()
