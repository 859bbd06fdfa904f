"""BetterDGCNN on the device (the runtime layer table of csrc/pcd_dgcnn.h through csrc/dgcnn.hip and
csrc/dgcnn_train.hip, PatchGeneration/Modules/Network/GCNModel.py, NetworkController.py, PatchCollector.py).

As tests/test_gpu_dgcnn.py and tests/test_gpu_dgcnn_train.py: the search in feature space is checked on its own, the
arithmetic with the device's OWN lists handed to the float64 restatement (tests/better_dgcnn_ref.py) within 8 x the
deviation the reference's own float32 run shows from its float64 run, and against the reference's goldens with nothing
injected.  No patch is excluded anywhere.  Measured figures are reported (conftest.report) before they are asserted.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import better_dgcnn_cases as cases
import better_dgcnn_ref as bref
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
    from PatchGeneration.Modules.NetworkController import Network, NetworkTrainer
    from PatchGeneration.Modules.PatchCollector import PatchCollector
    return {"nat": nat, "DGCNN": DGCNN, "BetterDGCNN": BetterDGCNN, "Mesh": Mesh, "PatchCollector": PatchCollector,
            "Network": Network, "NetworkTrainer": NetworkTrainer, "dev": gpu}


def torch_state(state):
    return {key: torch.as_tensor(np.asarray(v)) for key, v in state.items()}


def new_model(mods, name, trainable=False, dropout=0.5, sizes_as_tensor=False):
    t = cases.Table(name)
    sizes = torch.tensor(t.sizes) if sizes_as_tensor else t.sizes
    m = mods["BetterDGCNN"](t.l_e, t.l_d, t.l_l, sizes, t.k, 17, dropout, trainable=trainable)
    m.load_state_dict(torch_state(cases.make_state(name)), strict=True)
    return m.to(mods["dev"])


def model_for(mods, name):
    return cached(("model", name), lambda: new_model(mods, name).eval())


def fixture(golden):
    return cached("inputs", lambda: cases.fixture_inputs(golden))


def device_run(mods, golden, name):
    """One debug forward of a configuration's rows: (x float64 [n, 20, 64], out, debug dict), numpy."""
    def make():
        x = fixture(golden)[0][golden(f"better_dgcnn_{name}")["rows"]]
        out, dbg = model_for(mods, name)(torch.as_tensor(x, dtype=torch.float32).to(mods["dev"]), debug=True)
        torch.cuda.synchronize()
        return x, out.cpu().numpy().astype(np.float64), {key: v.cpu().numpy() for key, v in dbg.items()}
    return cached(("run", name), make)


# ------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_forward_against_restatement_with_device_lists(mods, golden, name):
    t = cases.Table(name)
    g = golden(f"better_dgcnn_{name}")
    x, out, dbg = device_run(mods, golden, name)
    assert dbg["lists"].shape == (t.l_d, len(x), 64, t.k) and dbg["cat"].shape == (len(x), t.ccat, 64)
    want, full = bref.forward(name, cases.make_state(name), x.astype(np.float32), lists=dbg["lists"], full=True)
    tol = 8.0 * float(g["dev32_stable"])
    dev = float(np.abs(out - want).max())
    inner = {key: float(np.abs(dbg[key].astype(np.float64) - full[key]).max()) for key in ("cat", "pooled")}
    hid = {f"h{j}": float(np.abs(dbg[f"h{j}"].astype(np.float64).T - full[f"h{j}"]).max()) for j in range(1, t.l_l)}
    report(f"better_dgcnn {name}: device vs float64 restatement on the device's lists, {len(x)} patches: max |dout| "
           f"{dev:.2e} (allowed {tol:.2e} = 8 x the reference's float32 deviation where no neighbour differs), ratio "
           f"{dev / tol:.3f}; concatenation {inner['cat']:.1e}, pooled {inner['pooled']:.1e}, hidden "
           f"{max(hid.values()):.1e}")
    assert dev <= tol


@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_forward_against_reference_golden(mods, golden, name):
    g = golden(f"better_dgcnn_{name}")
    x, out, dbg = device_run(mods, golden, name)
    dev = np.abs(out - g["out64"]).max(-1)
    differ = bref.lists_differ(name, x, dbg["cat"].astype(np.float64), g["lists64"], dbg["lists"])
    tol, tight = 8.0 * float(g["dev32_all"]), 8.0 * float(g["dev32_stable"])
    agree = float(dev[~differ].max()) if (~differ).any() else 0.0
    report(f"better_dgcnn {name}: device vs the reference's float64 outputs, {len(x)} patches, nothing injected: max "
           f"|dout| {dev.max():.2e} (allowed {tol:.2e}); lists differ from the golden's by distance on "
           f"{int(differ.sum())} patches (the reference's float32 run on the same rows: {int(g['differs32'].sum())}); "
           f"max |dout| where they agree {agree:.2e} (allowed {tight:.2e})")
    assert dev.max() <= tol
    assert agree <= tight


# ------------------------------------------------------------------------------------------------ 2. search
def test_first_search_runs_on_the_input_rows(mods, golden):
    """odd has no static layer: its first lists are the k nearest of rows 0:17 of the input (C = 17, patch stride
    20 x 64), exactly, within test_knn_sets_are_valid's rounding slack; every list ascending in (distance, index)."""
    t = cases.Table("odd")
    x, _, dbg = device_run(mods, golden, "odd")
    xin = torch.as_tensor(x[:, :17].astype(np.float32)).to(torch.float64)       # what the device saw, in float64
    D = ((xin[:, :, :, None] - xin[:, :, None, :]) ** 2).sum(1)
    norm = torch.linalg.vector_norm(xin, dim=1)
    bi = (17 + 4) * U * ((norm[:, :, None] + norm[:, None, :]) ** 2).amax(-1)
    lists = torch.as_tensor(dbg["lists"][0].astype(np.int64))
    assert int(lists.min()) >= 0 and int(lists.max()) <= 63
    member = torch.zeros_like(D, dtype=torch.bool).scatter_(2, lists, True)
    assert bool((member.sum(-1) == t.k).all())
    dl = torch.gather(D, 2, lists)
    assert bool((dl[..., :-1] - dl[..., 1:] <= 2 * bi[..., None]).all()), "a list is not ascending"
    assert bool(((dl[..., :-1] != dl[..., 1:]) | (lists[..., :-1] < lists[..., 1:])).all()), "a tie is not in index order"
    inf = torch.full_like(D, float("inf"))
    over = (torch.where(member, D, -inf).amax(-1) - torch.where(member, inf, D).amin(-1)).clamp_min(0.0)
    slack = float(torch.where(over > 0, over / (2 * bi).clamp_min(1e-300), over).max())
    report(f"better_dgcnn odd: first search on the 17 input rows, max (worst chosen - best left out) / (2 b_i) = {slack:.3f}")
    assert slack <= 1.0
    # the stage entry on the same rows gives the same lists
    again = mods["nat"].dgcnn_knn(torch.as_tensor(x[:, :17].astype(np.float32)).contiguous().to(mods["dev"]), t.k)
    assert np.array_equal(again.cpu().numpy(), dbg["lists"][0])


# ------------------------------------------------------------------------------------------------ 3. shared trunk
def test_default_shares_the_fixed_networks_trunk(mods, golden):
    """The trunk of `default` IS DGCNN(k = 8, emb_dims = 128)'s: the pooled row is the same bits under the same
    weights.  The outputs differ -- the head's slope is 0.01, not 0.2 -- and equal the restatement at 0.01."""
    dev = mods["dev"]
    g = golden("better_dgcnn_default")
    x, out, dbg = device_run(mods, golden, "default")
    state = cases.make_state("default")
    fixed = mods["DGCNN"](8, 17, 128, 0.5)
    fixed.load_state_dict(torch_state(state), strict=True)                      # the same keys and shapes
    fixed = fixed.to(dev).eval()
    fout, fdbg = fixed(torch.as_tensor(x, dtype=torch.float32).to(dev), debug=True)
    assert np.array_equal(fdbg["pooled"].cpu().numpy(), dbg["pooled"])
    assert np.array_equal(fdbg["cat"].cpu().numpy(), dbg["cat"])
    assert np.array_equal(fdbg["lists"].cpu().numpy(), dbg["lists"])
    fout = fout.cpu().numpy().astype(np.float64)
    tol = 8.0 * float(g["dev32_stable"])
    x32 = x.astype(np.float32)
    want = {slope: bref.forward("default", state, x32, lists=dbg["lists"], head_slope=slope) for slope in (0.01, 0.2)}
    gap = float(np.abs(want[0.01] - want[0.2]).max())
    report(f"better_dgcnn default: head slope 0.01 vs 0.2 moves the output by {gap:.2e}; device vs 0.01 "
           f"{np.abs(out - want[0.01]).max():.2e}, DGCNN vs 0.2 {np.abs(fout - want[0.2]).max():.2e} (allowed {tol:.2e})")
    assert gap > 100 * tol
    assert np.abs(out - want[0.01]).max() <= tol
    assert np.abs(fout - want[0.2]).max() <= tol


# ------------------------------------------------------------------------------------------------ 4. invariants
@pytest.mark.parametrize("name", ["narrow", "odd"])
def test_bits_do_not_depend_on_the_batch(mods, golden, name):
    model = model_for(mods, name)
    x = torch.as_tensor(fixture(golden)[0][:33], dtype=torch.float32).to(mods["dev"])
    one = model(x[5:6])
    assert torch.equal(model(x[5:6]), one)                                      # run to run
    assert torch.equal(model(torch.cat([x[5:6], x[0:1]]))[0:1], one)            # row 0 of 2
    big = torch.cat([x[:32], x[5:6]])
    got = model(big)
    assert torch.equal(got[32:33], one)                                         # row 32 of 33
    assert torch.equal(got, model(big)) and torch.equal(got[5:6], one)


@pytest.mark.parametrize("name", ["narrow", "odd"])
def test_nan_stays_in_its_patch(mods, golden, name):
    model = model_for(mods, name)
    x = torch.as_tensor(fixture(golden)[0][:3], dtype=torch.float32).to(mods["dev"])
    clean = model(x)
    for bad in (float("nan"), float("inf")):
        y = x.clone()
        y[1, 4, 7] = bad
        out = model(y)
        assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])
        assert not bool(torch.isfinite(out[1]).all())
    assert torch.equal(model(x), clean)


def test_index_columns(mods, golden):
    nat, dev = mods["nat"], mods["dev"]
    x = torch.as_tensor(fixture(golden)[0][:4], dtype=torch.float32).to(dev)
    y = x.clone()
    y[3, 17, 5] = float("nan")
    y[1, 19, 9] = 1e9
    narrow = model_for(mods, "narrow")
    clean = narrow(x)
    with pytest.raises(ValueError, match="patch 1 "):
        narrow(y)
    flag = torch.full((1,), nat.DGCNN_NO_BAD_PATCH, dtype=torch.int32, device=dev)
    out = narrow(y, first_bad=flag, patch_base=100)
    assert int(flag) == 101
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2]) and bool(torch.isfinite(out).all())
    assert torch.equal(narrow(x), clean)
    # without static layers the index columns are never read: nothing is raised or recorded, the bits are the clean ones
    odd = model_for(mods, "odd")
    clean = odd(x)
    assert torch.equal(odd(y), clean)
    flag.fill_(nat.DGCNN_NO_BAD_PATCH)
    assert torch.equal(odd(y, first_bad=flag, patch_base=100), clean) and int(flag) == nat.DGCNN_NO_BAD_PATCH
    trainable = new_model(mods, "odd", trainable=True, dropout=0.0).train()
    a = trainable(x)
    trainable.load_state_dict(torch_state(cases.make_state("odd")), strict=True)
    assert torch.equal(trainable(y), a)


# ------------------------------------------------------------------------------------------------ 5. stage entry
@pytest.mark.parametrize("cin,cout,n,b", [(17, 64, 3, 5), (64, 64, 8, 3), (32, 32, 4, 2), (17, 16, 3, 1), (33, 33, 5, 2),
                                          (65, 130, 5, 2)])
def test_edge_stage_by_shape(mods, cin, cout, n, b):
    """pcd_bdgcnn_edgeconv against the float64 edge convolution, within the fma-chain bound of
    test_edgeconv_against_restatement."""
    rng = np.random.default_rng([cin, cout, n, b])
    w = (rng.uniform(-1, 1, (cout, 2 * cin)) * np.sqrt(3.0 / (2 * cin))).astype(np.float32)
    s = (rng.uniform(0.5, 1.5, cout) * np.where(rng.random(cout) < 0.1, -1, 1)).astype(np.float32)
    t = rng.normal(0, 0.2, cout).astype(np.float32)
    x = rng.normal(0.0, 1.0, (b, cin, 64)).astype(np.float32)
    lists = rng.integers(0, 64, (b, 64, n)).astype(np.int32)
    dev = mods["dev"]
    got = mods["nat"].bdgcnn_edgeconv(*(torch.as_tensor(a).to(dev) for a in (w, s, t, x, lists)))
    got = got.cpu().numpy().astype(np.float64)
    x64, l64 = x.astype(np.float64), lists.astype(np.int64)
    want = _edge_folded(w, s, t, x64, l64)
    bound = (2 * cin + 16) * U * _edge_bound_folded(w, s, t, x64, l64)
    ratio = float((np.abs(got - want) / bound).max())
    report(f"bdgcnn_edgeconv ({cin}, {cout}) n={n} b={b}: max |device - float64| / ((2 Cin + 16) 2^-24 M) = {ratio:.3f}")
    assert got.shape == want.shape and ratio <= 1.0


@pytest.mark.parametrize("cin,cout,n,b,nan_row", [(17, 64, 3, 5, False), (64, 64, 8, 3, True), (32, 32, 4, 2, False),
                                                  (17, 16, 3, 1, False), (33, 33, 5, 2, False)])
def test_fused_edge_layer_is_the_two_kernel_path_bit_for_bit(mods, cin, cout, n, b, nan_row):
    nat, dev = mods["nat"], mods["dev"]
    rng = np.random.default_rng([cin, cout, n, b, 7])
    w = (rng.uniform(-1, 1, (cout, 2 * cin)) * np.sqrt(3.0 / (2 * cin))).astype(np.float32)
    s = (rng.uniform(0.5, 1.5, cout) * np.where(rng.random(cout) < 0.1, -1, 1)).astype(np.float32)
    t = rng.normal(0, 0.2, cout).astype(np.float32)
    x = rng.normal(0.0, 1.0, (b, cin, 64)).astype(np.float32)
    if nan_row:
        x[1, :, 9] = np.nan                                                     # node 9 of patch 1
    lists = rng.integers(0, 64, (b, 64, n)).astype(np.int32)
    args = [torch.as_tensor(a).to(dev) for a in (w, s, t, x, lists)]
    off = nat.bdgcnn_edgeconv(*args, fused=nat.FUSED_OFF)
    on = nat.bdgcnn_edgeconv(*args, fused=nat.FUSED_ON)
    auto = nat.bdgcnn_edgeconv(*args, fused=nat.FUSED_AUTO)
    # with the caller's scratch (nothing allocated, nothing waited for): the same bits, a short one refused
    need = nat.bdgcnn_edgeconv_scratch_bytes(cin, cout, b)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    for mode in (nat.FUSED_OFF, nat.FUSED_ON):
        got = nat.bdgcnn_edgeconv(*args, fused=mode, scratch=scratch, out=torch.empty_like(off))
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), off.view(torch.int32))
    with pytest.raises(ValueError, match="scratch"):
        nat.bdgcnn_edgeconv(*args, fused=nat.FUSED_OFF, scratch=scratch[:need - 256])
    torch.cuda.synchronize()
    assert torch.equal(on.view(torch.int32), off.view(torch.int32))             # bits, NaNs included
    assert torch.equal(auto.view(torch.int32), off.view(torch.int32))
    if nan_row:
        assert bool(torch.isnan(off[1]).any()) and bool(torch.isfinite(off[0]).all()) and bool(torch.isfinite(off[2]).all())
    else:
        assert bool(torch.isfinite(off).all())


def test_fused_edge_layer_is_refused_above_one_tile(mods):
    nat, dev = mods["nat"], mods["dev"]
    rng = np.random.default_rng(65)
    args = [torch.as_tensor(a).to(dev) for a in (
        rng.normal(size=(65, 34)).astype(np.float32), np.ones(65, np.float32), np.zeros(65, np.float32),
        rng.normal(size=(2, 17, 64)).astype(np.float32), rng.integers(0, 64, (2, 64, 3)).astype(np.int32))]
    with pytest.raises(ValueError, match="fused"):
        nat.bdgcnn_edgeconv(*args, fused=nat.FUSED_ON)
    with pytest.raises(ValueError, match="fused"):
        nat.bdgcnn_edgeconv(*args, fused=3)
    assert torch.equal(nat.bdgcnn_edgeconv(*args, fused=nat.FUSED_AUTO), nat.bdgcnn_edgeconv(*args, fused=nat.FUSED_OFF))


def _split(w):
    w = w.astype(np.float64)
    cin = w.shape[1] // 2
    return w[:, :cin], w[:, cin:] - w[:, :cin]


def _gathered(A, B, nbr):
    b = np.arange(A.shape[0])[:, None, None, None]
    c = np.arange(A.shape[1])[None, :, None, None]
    return A[b, c, nbr[:, None]] + B[:, :, :, None]


def _edge_folded(w, s, t, x, nbr):
    wa, wd = _split(w)
    v = s.astype(np.float64)[None, :, None, None] * _gathered(wa @ x, wd @ x, nbr) + t.astype(np.float64)[None, :, None, None]
    m = v.max(-1)
    return np.where(m > 0, m, 0.2 * m)


def _edge_bound_folded(w, s, t, x, nbr):
    wa, wd = _split(w)
    m = np.abs(s).astype(np.float64)[None, :, None, None] * _gathered(np.abs(wa) @ np.abs(x), np.abs(wd) @ np.abs(x), nbr) \
        + np.abs(t).astype(np.float64)[None, :, None, None]
    return m.max(-1)


# ------------------------------------------------------------------------------------------------ 6. training step
def device_loss(out, gt):
    ones = torch.ones(len(out), dtype=torch.float32, device=out.device)
    return tref.LOSS_WEIGHTS[0] * F.cosine_embedding_loss(out, gt, ones) + tref.LOSS_WEIGHTS[1] * F.mse_loss(out, gt)


def train_case(golden, name):
    g = golden(f"better_dgcnn_train_{name}")
    return g, fixture(golden)[0][g["rows"]]


def one_step(mods, golden, name):
    g, x = train_case(golden, name)
    model = new_model(mods, name, trainable=True, dropout=0.0).train()
    xd = torch.as_tensor(x, dtype=torch.float32).to(mods["dev"])
    gt = torch.as_tensor(g["gt"], dtype=torch.float32).to(mods["dev"])
    out, dbg = model(xd, debug=True)
    assert out.grad_fn is not None and out.dtype == torch.float32 and tuple(out.shape) == (len(x), 3)
    device_loss(out, gt).backward(retain_graph=True)
    return model, out, dbg


def device_step(mods, golden, name):
    """One train() forward + backward on a fresh model: {"out", "lists", "grads", "buffers", "tracked"}, numpy."""
    def make():
        t = cases.Table(name)
        model, out, dbg = one_step(mods, golden, name)
        torch.cuda.synchronize()
        named, sd = dict(model.named_parameters()), model.state_dict()
        assert all(p.grad is not None for p in model.parameters())              # gradients reach every parameter
        return {"out": out.detach().cpu().numpy().astype(np.float64), "lists": dbg["lists"].cpu().numpy(),
                "grads": {key: named[key].grad.cpu().numpy().astype(np.float64) for key in bref.param_names(name)},
                "buffers": {key: sd[key].cpu().numpy().astype(np.float64) for key in bref.buffer_names(name)},
                "tracked": [int(sd[f"bn{i}.num_batches_tracked"]) for i in range(1, t.E + t.l_l + 1)]}
    return cached(("step", name), make)


def check_step(what, name, g, got, want_grads, want_out, want_buffers):
    """test_gpu_dgcnn_train.check_step for a table: the list of misses against 8 x the golden's float32 deviations."""
    worst, fails = 0.0, []

    def one(label, err, tol):
        nonlocal worst
        worst = max(worst, err / tol)
        if not err <= tol:
            fails.append(f"{label}: {err:.3e} > {tol:.3e} ({err / tol:.2f} x the bound)")

    one("out", float(np.abs(got["out"] - want_out).max()), 8 * float(g["outdev32"]) * float(np.abs(want_out).max()))
    for key in bref.param_names(name):
        for label, a, b, weight in want_grads(key, got["grads"][key]):
            one(f"{key} {label}", float(np.abs(a - b).max()),
                8 * float(g[f"gdev32/{key}"]) * float(g[f"gscale/{key}"]) * weight)
    for key in bref.buffer_names(name):
        want = want_buffers[key]
        one(key, float(np.abs(got["buffers"][key] - want).max()),
            8 * float(g[f"bufdev32/{key}"]) * float(np.abs(want).max()))
    report(f"better_dgcnn train {what}: worst error / bound {worst:.3f} over out, {len(bref.param_names(name))} "
           f"gradients, {len(bref.buffer_names(name))} buffers")
    return [f"{what}: {f}" for f in fails]


@pytest.mark.parametrize("name", list(cases.TRAIN))
def test_step_against_restatement_with_device_lists(mods, golden, name):
    """`default` at b = 2 is the sensitive one: linear2.bias, whose gradient is zero in exact arithmetic (bn9 removes a
    constant), came out as 1.9e-6 -- 3.4 x its bound -- while the head's batch norms ran in float32 on the device (the
    reference's CPU batch norm accumulates in double and leaves 6.8e-8); on float64 views of their tensors
    (GCNModel._batch_norm_wide) it is exactly 0."""
    g, x = train_case(golden, name)
    got = device_step(mods, golden, name)
    assert got["tracked"] == [1] * len(got["tracked"])
    want = bref.step(name, cases.make_state(name), x.astype(np.float32), g["gt"].astype(np.float32), got["lists"])
    fails = check_step(f"{name} vs the restatement on the device's lists", name, g, got,
                       lambda key, grad: [("every entry", grad, want["grads"][key], 1.0)], want["out"], want["buffers"])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", list(cases.TRAIN))
def test_step_against_reference_golden(mods, golden, name):
    """Nothing injected.  On all four configurations the device's lists equal the reference's float64 lists by distance
    (asserted: the reference's own float32 run agrees on them too, `differs32`), so the same bounds hold against the
    golden's stored entries."""
    g, x = train_case(golden, name)
    got = device_step(mods, golden, name)
    cat64 = bref.step(name, cases.make_state(name), x, g["gt"], g["lists64"], full=True)["cat"]
    differs = bref.lists_differ(name, x, cat64, g["lists64"], got["lists"])
    report(f"better_dgcnn train {name}: the device's lists differ from the reference's float64 lists by distance on "
           f"{int(differs.sum())} of {len(differs)} patches")
    assert not differs.any(), f"{name}: the device's lists differ from the reference's by distance on {differs.sum()} patches"
    fails = check_step(f"{name} vs the reference's golden, nothing injected", name, g, got,
                       lambda key, grad: tref.golden_views(g, key, grad), g["out64"],
                       {key: g[f"buf/{key}"] for key in bref.buffer_names(name)})
    assert not fails, "\n".join(fails)


def test_training_repeats_bitwise_and_consumes_its_workspace(mods, golden):
    runs = []
    for _ in range(2):
        model, out, _ = one_step(mods, golden, "narrow")
        runs.append((out.detach(), [p.grad.clone() for p in model.parameters()], [b.clone() for b in model.buffers()]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    with pytest.raises(RuntimeError, match="consumed"):
        out.sum().backward()
    # eval() of a trainable model is the inference path, bit for bit
    x = torch.as_tensor(fixture(golden)[0][:3], dtype=torch.float32).to(mods["dev"])
    assert torch.equal(new_model(mods, "narrow", trainable=True).eval()(x), model_for(mods, "narrow")(x))


# ------------------------------------------------------------------------------------------------ 7. module
@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_state_dict_keys_and_shapes(mods, golden, name):
    g = golden(f"better_dgcnn_{name}")
    t = cases.Table(name)
    model = mods["BetterDGCNN"](t.l_e, t.l_d, t.l_l, torch.tensor(t.sizes), t.k, 17, 0.5)
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in g["sd_keys"]]
    assert [",".join(str(int(s)) for s in v.shape) for v in sd.values()] == [str(s) for s in g["sd_shapes"]]
    assert (model.l_e, model.l_d, model.l_l) == (t.l_e, t.l_d, t.l_l)
    assert model.channel_sizes.tolist() == list(t.sizes)
    assert model.cum_sizes.tolist() == [0] + list(np.cumsum(t.sizes))


def test_checkpoint_round_trip_and_repacking(mods, golden, tmp_path):
    dev = mods["dev"]
    model = new_model(mods, "narrow", sizes_as_tensor=True).eval()
    x = torch.as_tensor(fixture(golden)[0][:4], dtype=torch.float32).to(dev)
    first = model(x)
    assert torch.equal(first, model_for(mods, "narrow")(x))                     # a tensor or a tuple of sizes: one model
    net = mods["Network"](model)
    path = str(tmp_path / "nets" / "narrow.t7")
    net.saveModel(path)
    t = cases.Table("narrow")
    other = mods["Network"](mods["BetterDGCNN"](t.l_e, t.l_d, t.l_l, t.sizes, t.k, 17, 0.5).to(dev).eval())
    assert not torch.equal(other.getModel()(x), first)
    other.loadModel(path)
    assert torch.equal(other.getModel()(x), first)
    with pytest.raises(ValueError, match="not a member of DGCNN"):
        mods["Network"](torch.nn.Linear(2, 2))
    with torch.no_grad():
        getattr(model, f"linear{t.l_l}").bias += 1.0                            # in place: the version counter moves
    shifted = model(x)
    assert float((shifted - (first + 1.0)).abs().max()) <= 1e-6 and not torch.equal(shifted, first)
    with torch.no_grad():
        model.bn2.running_mean.add_(0.5)                                        # a buffer, through its alias conv2.1
    assert float((model(x) - shifted).abs().max()) > 1e-5
    model.load_state_dict(torch_state(cases.make_state("narrow")), strict=True)
    assert torch.equal(model(x), first)


def test_trainer_lowers_the_loss_on_the_device(mods, golden):
    nat, dev = mods["nat"], mods["dev"]
    inputs, size = fixture(golden)
    rows = cases.config_rows(size)
    x = torch.as_tensor(np.transpose(inputs[rows], (0, 2, 1)), dtype=torch.float32).to(dev)    # [16, 64, 20] rows
    gt = torch.as_tensor(tref.unit_vectors("better trainer", 16), dtype=torch.float32).to(dev)
    model = new_model(mods, "narrow", trainable=True, dropout=0.0)
    net = mods["Network"](model)
    packs = nat.host_packs
    losses = mods["NetworkTrainer"](net, [(x, gt)]).train(3, Adam_learning_rate=1e-3, loss_based_on_value_loss=0.5)
    assert nat.host_packs == packs                                              # no weight went to the host
    assert len(losses) == 3 and all(np.isfinite(l).all() for l in losses)
    report(f"better_dgcnn trainer (narrow): MSE {losses[0][1]:.4f} -> {losses[-1][1]:.4f}")
    assert losses[-1][1] < losses[0][1]
    assert int(model.bn1.num_batches_tracked) == 3 and int(model.bn4.num_batches_tracked) == 3


# ------------------------------------------------------------------------------------------------ 8. pipeline
def test_predict_normals_on_the_ellipsoid(mods, golden):
    dev = mods["dev"]
    g = patch_cases.load_golden("ellipsoid")
    model = model_for(mods, "narrow")
    mesh = mods["Mesh"](g["v"].copy(), g["f"].copy())
    pc = mods["PatchCollector"](mesh, int(g["k"]))
    normals, fallbacks = pc.predictNormals(model, batch_faces=100)
    assert normals.shape == (320, 3) and normals.dtype == torch.float64 and normals.is_cuda and fallbacks == 0
    ds = pc.collectNetworkInput(256, dtype=np.float32)
    x = torch.as_tensor(np.ascontiguousarray(ds.data_patch.transpose(0, 2, 1))).to(dev)
    by_hand = []
    for s in range(0, len(x), 100):                                             # chunk by chunk: forward, unalign
        by_hand.append(model(x[s:s + 100]).cpu().numpy().astype(np.float64))
    by_hand = ds.unalign(np.concatenate(by_hand))
    by_hand /= np.linalg.norm(by_hand, axis=1, keepdims=True)
    assert np.abs(normals.cpu().numpy() - by_hand).max() <= 1e-14
    a = mods["Mesh"](g["v"].copy(), g["f"].copy())
    a.denoise(guided_normals=normals, normal_iterations=1, vertex_iterations=1)
    assert np.isfinite(a.v).all()


# ------------------------------------------------------------------------------------------------ 9. arguments
def test_arguments(mods, golden):
    B, dev = mods["BetterDGCNN"], mods["dev"]
    ok = dict(l_e=1, l_d=1, l_l=2, channel_sizes=(32, 48, 96, 40), k=4, init_dims=17, dropout=0.5)

    def build(**change):
        return B(**dict(ok, **change))

    build()
    for change, word in (({"l_l": 1, "channel_sizes": (32, 48, 96)}, "l_l"),
                         ({"l_e": 0, "l_d": 0, "channel_sizes": (96, 40)}, "l_e"),
                         ({"channel_sizes": (32, 48, 96)}, "channel_sizes"),
                         ({"channel_sizes": (32, 48, 96, 40, 8)}, "channel_sizes"),
                         ({"channel_sizes": (32, 0, 96, 40)}, r"channel_sizes\[1\]"),
                         ({"channel_sizes": torch.tensor([32, 48, -1, 40])}, r"channel_sizes\[2\]"),
                         ({"channel_sizes": (32, 5000, 96, 40)}, r"channel_sizes\[1\]"),
                         ({"l_e": 9, "l_d": 8, "channel_sizes": (8,) * 19}, "l_e"),
                         ({"k": 0}, "k"), ({"k": 65}, "k"), ({"init_dims": 16}, "init_dims")):
        with pytest.raises(ValueError, match=word):
            build(**change)
    # the library refuses the same tables on its own
    nat = mods["nat"]
    sizes = (nat.ctypes.c_int32 * 3)(32, 48, 96)
    table = nat.DgcnnTableStruct(1, 1, 1, nat.ctypes.cast(sizes, nat._I32P), 4, 17, 3)
    v = nat.c_int64(0)
    with pytest.raises(ValueError, match="l_l"):
        nat.check(nat.lib().pcd_bdgcnn_train_workspace_bytes(nat.ctypes.byref(table), 1, nat.ctypes.byref(v)), "table")
    model = model_for(mods, "narrow")
    x = torch.as_tensor(fixture(golden)[0][:2], dtype=torch.float32).to(dev)
    with pytest.raises(ValueError):
        model(x.cpu())
    with pytest.raises(ValueError):
        model(x[:, :19])
    need = model.native().workspace_bytes(2)
    with pytest.raises(ValueError, match="workspace"):
        model(x, workspace=torch.empty(need - 256, dtype=torch.uint8, device=dev))
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    assert torch.equal(model(x, workspace=ws), model(x))
    with pytest.raises(ValueError, match="aligned"):
        model(x, workspace=ws[4:])
    assert model(x[:0]).shape == (0, 3)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="eval"):
            model(x)
    finally:
        model.eval()
    st = torch_state(cases.make_state("narrow"))
    t = nat.DgcnnTable(1, 1, 2, (32, 48, 96, 40), 4)
    conv = [st[f"conv{i}.0.weight"] for i in range(1, 4)]
    bn = [(st[f"bn{i}.weight"], st[f"bn{i}.bias"], st[f"bn{i}.running_mean"], st[f"bn{i}.running_var"], 1e-5)
          for i in range(1, 5)]
    lin = [(st["linear1.weight"], None), (st["linear2.weight"], st["linear2.bias"])]
    assert torch.equal(nat.BetterDgcnn(t, conv, bn, lin).forward(x), model(x))  # host pointers work too
    with pytest.raises(ValueError, match="conv2"):
        nat.BetterDgcnn(t, [conv[0], conv[0], conv[2]], bn, lin)
    with pytest.raises(ValueError, match="linear1"):
        nat.BetterDgcnn(t, conv, bn, [(lin[0][0], lin[1][1].new_zeros(40)), lin[1]])
    # the training entries: a short workspace writes nothing
    tm = new_model(mods, "narrow", trainable=True, dropout=0.0).train()
    before = {key: v.clone() for key, v in tm.state_dict().items()}
    convd = [getattr(tm, f"conv{i}")[0].weight.detach() for i in range(1, 4)]
    bnd = [(m.weight.detach(), m.bias.detach(), m.running_mean, m.running_var, m.num_batches_tracked, m.eps, m.momentum)
           for m in (tm.bn1, tm.bn2, tm.bn3)]
    need = nat.bdgcnn_train_workspace_bytes(t, 2)
    tws = torch.empty(need, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="workspace"):
        nat.bdgcnn_train_forward(t, convd, bnd, x, tws[:need - 256])
    with pytest.raises(ValueError, match="workspace"):
        nat.bdgcnn_train_backward(t, convd, x, torch.zeros((2, 2 * 96), device=dev), tws[:need - 256])
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[key]) for key, v in tm.state_dict().items())
    assert tuple(nat.bdgcnn_train_forward(t, convd, bnd, x, tws).shape) == (2, 192)
