"""DGCNN training on the device (csrc/dgcnn_train.hip, Network/GCNModel.py with trainable=True, NetworkController.py).

The kernels are checked stage by stage against exact integer products and against the float64 restatement of the
training step (tests/dgcnn_train_ref.py) with the device's OWN neighbour lists handed to it, and the whole step against
the reference's golden run (tests/golden/dgcnn_train_*.npz) where the device's lists agree with the reference's.

Bounds.  Whole-step comparisons take theirs from the golden file: 8 x the deviation the reference's own float32 run
shows from its float64 run, per tensor (gdev32, outdev32, bufdev32), relative to that tensor's scale (gscale) -- the
factor the forward's tests give the reference's float32 deviation.  The edge-layer stage has no reference float32 run,
so its bound is worked out from the number formats: with u = 2^-24, an edge value y = A[j] + B[i] is an fma chain of
K = Cin terms plus one addition, |error| <= (K + 2) u M with M = |W_a| |x_j| + |W_b - W_a| |x_i|; a normalised value
(y - mu) / sigma inherits e = (K + 2) u max(M / sigma) relative to 1; every output of the stage is a sum of L products of
such values with exact cotangents, accumulated in double or (the MFMA) in an fma chain of length L, then rounded to
float32.  So each tensor T is bounded by 16 (e + (L + 2) u) max |T|: one e for each of the up to four normalised
factors in a term (y_hat, 1 / sigma, s, the statistics they are centred with), doubled for the two passes of the batch
norm backward, doubled again for headroom.  Measured figures are reported (conftest.report) before they are asserted.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dgcnn_cases as cases
import dgcnn_ref as ref
import dgcnn_train_ref as tref
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
    from PatchGeneration.Modules.Network.GCNModel import DGCNN
    from PatchGeneration.Modules.NetworkController import Network, NetworkTrainer
    return {"nat": nat, "DGCNN": DGCNN, "Network": Network, "NetworkTrainer": NetworkTrainer, "dev": gpu}


def torch_state(state):
    return {key: torch.as_tensor(np.asarray(v)) for key, v in state.items()}


def new_model(mods, k, emb, trainable=True, dropout=0.0, state=None):
    m = mods["DGCNN"](k, 17, emb, dropout, trainable=trainable)
    m.load_state_dict(torch_state(cases.make_state(cases.SEED, k, emb)) if state is None else state, strict=True)
    return m.to(mods["dev"])


def device_loss(out, gt):
    ones = torch.ones(len(out), dtype=torch.float32, device=out.device)
    return tref.LOSS_WEIGHTS[0] * F.cosine_embedding_loss(out, gt, ones) + tref.LOSS_WEIGHTS[1] * F.mse_loss(out, gt)


def case(golden, name):
    k, emb, fixture = tref.CONFIGS[name][:3]
    g = golden(f"dgcnn_train_{name}")
    x = cases.fixture_inputs(golden, fixture)[0][g["rows"]]
    return g, k, emb, x


def device_step(mods, golden, name):
    """One train() forward + backward of a configuration on a fresh model:
    {"out", "lists", "grads" {name: float64 array}, "buffers", "tracked"}, numpy."""
    def make():
        g, k, emb, x = case(golden, name)
        model = new_model(mods, k, emb).train()
        xd = torch.as_tensor(x, dtype=torch.float32).to(mods["dev"])
        gt = torch.as_tensor(g["gt"], dtype=torch.float32).to(mods["dev"])
        out, dbg = model(xd, debug=True)
        assert out.grad_fn is not None and out.dtype == torch.float32 and tuple(out.shape) == (len(x), 3)
        device_loss(out, gt).backward()
        torch.cuda.synchronize()
        named = dict(model.named_parameters())
        sd = model.state_dict()
        return {"out": out.detach().cpu().numpy().astype(np.float64), "lists": dbg["lists"].cpu().numpy(),
                "grads": {key: named[key].grad.cpu().numpy().astype(np.float64) for key in tref.param_names()},
                "buffers": {key: sd[key].cpu().numpy().astype(np.float64) for key in tref.buffer_names()},
                "tracked": [int(sd[f"bn{i}.num_batches_tracked"]) for i in range(1, 11)]}
    return cached(("step", name), make)


def restated(golden, name, lists):
    """The float64 restatement of a configuration's step on the given lists (computed once per list source)."""
    g, k, emb, x = case(golden, name)
    return tref.step(cases.make_state(cases.SEED, k, emb), x.astype(np.float32), g["gt"].astype(np.float32), lists,
                     full=True)


def check_step(what, g, got, want_grads, want_out, want_buffers):
    """Output, every gradient and every buffer of bn1-10 against `want_*` within 8 x the golden's float32 deviations:
    the list of misses (empty: all within).  want_grads(key, grad) -> [(label, got, want, weight)]
    (dgcnn_train_ref.golden_views' form)."""
    worst, fails = 0.0, []

    def one(label, err, tol):
        nonlocal worst
        worst = max(worst, err / tol)
        if not err <= tol:
            fails.append(f"{label}: {err:.3e} > {tol:.3e} ({err / tol:.2f} x the bound)")

    one("out", float(np.abs(got["out"] - want_out).max()), 8 * float(g["outdev32"]) * float(np.abs(want_out).max()))
    for key in tref.param_names():
        for label, a, b, weight in want_grads(key, got["grads"][key]):
            one(f"{key} {label}", float(np.abs(a - b).max()),
                8 * float(g[f"gdev32/{key}"]) * float(g[f"gscale/{key}"]) * weight)
    for key in tref.buffer_names():
        want = want_buffers[key]
        one(key, float(np.abs(got["buffers"][key] - want).max()),
            8 * float(g[f"bufdev32/{key}"]) * float(np.abs(want).max()))
    report(f"dgcnn train {what}: worst error / bound {worst:.3f} over out, {len(tref.param_names())} gradients, "
           f"{len(tref.buffer_names())} buffers")
    return [f"{what}: {f}" for f in fails]


# ------------------------------------------------------------------------------------------ 1, 2. the two GEMMs
def _ints(shape, mul, mod, off):
    e = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    return ((e * mul + e // 5) % mod - off).astype(np.float32)


WGRAD_SHAPES = [(64, 17, 1), (3, 64, 5), (130, 1024, 2), (512, 256, 33), (64, 17, 13)]


@pytest.mark.parametrize("M,K,b", WGRAD_SHAPES)
def test_weight_gradient_gemm_is_exact(mods, M, K, b):
    nat, dev = mods["nat"], mods["dev"]
    if (M, K, b) == WGRAD_SHAPES[-1]:                   # b x 64 columns are no multiple of the reduction split
        assert b % nat.dgcnn_wgrad_split(b) != 0 and nat.dgcnn_wgrad_split(b) > 1
    dy, x = _ints((b, M, 64), 7, 7, 3), _ints((b, K, 64), 11, 9, 4)     # integers in [-3, 3] and [-4, 4]
    want = np.einsum("bmn,bkn->mk", dy.astype(np.int64), x.astype(np.int64))
    assert np.abs(dy).astype(np.int64).max() * np.abs(x).astype(np.int64).max() * b * 64 < 2 ** 24   # every partial sum exact
    got = nat.dgcnn_wgrad(torch.as_tensor(dy).to(dev), torch.as_tensor(x).to(dev)).cpu().numpy()
    assert got.shape == (M, K)
    np.testing.assert_array_equal(got.astype(np.int64), want)
    np.testing.assert_array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("M,K,b", WGRAD_SHAPES)
def test_add_into_y_epilogue_is_exact(mods, M, K, b):
    nat, dev = mods["nat"], mods["dev"]
    for nodes in (64, 1):
        xs = (b, K, 64) if nodes == 64 else (K, b)
        w1, w2 = _ints((M, K), 5, 7, 3), _ints((M, K), 3, 5, 2)
        x1, x2 = _ints(xs, 7, 9, 4), _ints(xs, 13, 7, 3)
        prod = (lambda w, x: np.einsum("mk,bkn->bmn", w, x)) if nodes == 64 else (lambda w, x: w @ x)
        want = prod(w1.astype(np.int64), x1.astype(np.int64)) + prod(w2.astype(np.int64), x2.astype(np.int64))
        assert 2 * 12 * K < 2 ** 24
        d = lambda a: torch.as_tensor(a).to(dev)
        y = nat.dgcnn_gemm(d(w1), d(x1))
        back = nat.dgcnn_gemm(d(w2), d(x2), nat.EPI_ADD, y=y)
        assert back.data_ptr() == y.data_ptr()
        np.testing.assert_array_equal(y.cpu().numpy().astype(np.int64), want)
    with pytest.raises(ValueError):
        nat.dgcnn_gemm(d(w2), d(x2), nat.EPI_ADD)       # nothing to add into


# ------------------------------------------------------------------------------------------ 3. one edge layer
def _edge_inputs(layer, b, n, seed):
    cin, cout = cases.EDGE[layer - 1]
    rng = np.random.default_rng([seed, layer, b, n])
    x = rng.normal(0.0, 1.0, (b, cin, 64)).astype(np.float32)
    w = (rng.uniform(-1, 1, (cout, 2 * cin)) * np.sqrt(3.0 / (2 * cin))).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, cout) * np.where(rng.random(cout) < 0.1, -1.0, 1.0)).astype(np.float32)
    beta = rng.normal(0.0, 0.2, cout).astype(np.float32)
    lists = rng.integers(0, 64, (b, 64, n))
    lists[:, 5] = lists[:, 5, :1]                       # [j, j, j]: one neighbour in every slot
    lists[:, 6] = 6                                     # ... the row itself in every slot
    lists[:, 60:] = 63                                  # the all-63 rows of a padded patch
    g = rng.normal(0.0, 1.0, (b, cout, 64)).astype(np.float32)
    rm = rng.normal(0.0, 0.1, cout).astype(np.float32)
    rv = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    return x, w, gamma, beta, lists, g, rm, rv


@pytest.mark.parametrize("layer,b,n", [(1, 9, 3), (3, 3, 3), (4, 3, 8), (6, 2, 20), (4, 1, 1)])
def test_edge_layer_against_restatement(mods, layer, b, n):
    nat, dev = mods["nat"], mods["dev"]
    cin, cout = cases.EDGE[layer - 1]
    x, w, gamma, beta, lists, g, rm, rv = _edge_inputs(layer, b, n, 5)
    d = lambda a, dt=torch.float32: torch.as_tensor(a).to(dev, dt)
    rmd, rvd, nbt = d(rm), d(rv), torch.full((), 4, dtype=torch.int64, device=dev)
    momentum = 0.25
    out, arg, stats = nat.dgcnn_edgeconv_train(layer, d(w), d(gamma), d(beta), tref.EPS, d(x), d(lists, torch.int32),
                                               momentum, rmd, rvd, nbt)
    bw = nat.dgcnn_edgeconv_train_backward(layer, d(w), d(gamma), d(beta), tref.EPS, d(x), d(lists, torch.int32), d(g))
    torch.cuda.synchronize()
    # the restatement, float64, on the same float32 numbers
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    leaves = [t64(a).requires_grad_(True) for a in (w, gamma, beta, x)]
    e = tref.edge(leaves[0], leaves[1], leaves[2], leaves[3], torch.as_tensor(lists))
    e["A"].retain_grad()
    e["B"].retain_grad()
    (e["out"] * t64(g)).sum().backward()
    N = b * 64 * n
    assert e["n"] == N
    mu, var = e["mu"].detach().numpy(), e["var"].detach().numpy()
    sigma = np.sqrt(var + tref.EPS)
    wa, wd = np.abs(w[:, :cin]).astype(np.float64), np.abs(w[:, cin:].astype(np.float64) - w[:, :cin])
    ax = np.abs(x).astype(np.float64)
    M = (wa @ ax).max((0, 2)) + (wd @ ax).max((0, 2))                  # [cout]
    ey = (cin + 2) * U * M                                             # |error| of an edge value, per channel
    erel = float((ey / sigma).max())
    got_stats = stats.cpu().numpy()
    figures = []

    def close(label, got, want, tol):
        err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
        figures.append(f"{label} {err:.2e}/{float(np.max(tol)):.2e}")
        assert (np.abs(np.asarray(got, dtype=np.float64) - want) <= tol).all(), f"{label}: {err:.3e} > {np.max(tol):.3e}"

    try:
        close("mean", got_stats[0], mu, ey)
        close("var", got_stats[1], var, 2 * ey * sigma + ey * ey)
        close("1/sigma", got_stats[2], 1 / sigma, 4 * erel / sigma)
        # buffers: the unbiased variance N / (N - 1) goes into running_var (at b = 1, n = 1: 64 / 63)
        close("running_mean", rmd.cpu().numpy(), (1 - momentum) * rm + momentum * mu, momentum * ey + 2 * U * np.abs(rm).max())
        close("running_var", rvd.cpu().numpy(), (1 - momentum) * rv + momentum * var * (N / (N - 1)),
              momentum * 2 * (2 * ey * sigma + ey * ey) + 2 * U * np.abs(rv).max())
        assert int(nbt) == 5
        assert np.array_equal(arg.cpu().numpy(), e["arg"].numpy()), "arg-max slots differ"
        assert (arg.cpu().numpy()[:, :, 5] == 0).all() and (arg.cpu().numpy()[:, :, 60:] == 0).all()   # ties: first slot
        zmax = float(e["out"].detach().abs().max()) / 0.2
        close("out", out.cpu().numpy(), e["out"].detach().numpy(), 16 * (erel + 3 * U) * max(1.0, zmax))
        wants = {"dgamma": (leaves[1].grad.numpy(), b * 64), "dbeta": (leaves[2].grad.numpy(), b * 64),
                 "dw": (leaves[0].grad.numpy(), b * 64), "dx": (leaves[3].grad.numpy(), 2 * cout),
                 "dab": (torch.cat([e["A"].grad, e["B"].grad], 1).numpy(), 64 * n)}
        for key, (want, L) in wants.items():
            close(key, bw[key].cpu().numpy(), want, 16 * (erel + (L + 2) * U) * float(np.abs(want).max()))
    finally:
        report(f"dgcnn train edge layer {layer} b={b} n={n} (error/bound): " + ", ".join(figures))


# ------------------------------------------------------------------------------------------ 4, 5. the whole step
@pytest.mark.parametrize("name", list(tref.CONFIGS))
def test_step_against_restatement_with_device_lists(mods, golden, name):
    """k1_b2_ellipsoid is the sensitive one: with b = 2 the head's batch norms normalise two samples, one channel of
    bn8 has 1 / sigma = 309 (the cap 1 / sqrt(eps) is 316), and the rounding of the pooled features is multiplied by
    that on its way to the output and, through the loss, into every gradient.  With one float32 chain over all of K in
    the forward products it landed at 3.5 x the bound; with chains of 8 k joined in double (gemm_kernel<8>) and the
    edge values and affines formed in double it is at 0.21 x (k8_b5_ellipsoid 0.46 x, k20_b6_shells 0.28 x)."""
    g = case(golden, name)[0]
    got = device_step(mods, golden, name)
    assert got["tracked"] == [1] * 10
    want = restated(golden, name, got["lists"])
    fails = check_step(f"{name} vs the restatement on the device's lists", g, got,
                       lambda key, grad: [("every entry", grad, want["grads"][key], 1.0)], want["out"], want["buffers"])
    assert not fails, "\n".join(fails)


def lists_differ_from_golden(mods, golden, name):
    """[n] bool: the patches whose device lists differ BY DISTANCE from the reference's float64 lists."""
    def make():
        g = case(golden, name)[0]
        cat64 = restated(golden, name, g["lists64"])["cat"]
        lists = device_step(mods, golden, name)["lists"]
        differs = np.zeros(len(g["rows"]), bool)
        for layer, (lo, hi) in enumerate(ref.DYN_INPUT):
            differs |= ref.lists_differ(cat64[:, lo:hi], g["lists64"][layer], lists[layer]).any(-1)
        report(f"dgcnn train {name}: the device's lists differ from the reference's float64 lists by distance on "
               f"{int(differs.sum())} of {len(differs)} patches")
        return differs
    return cached(("differs", name), make)


@pytest.mark.parametrize("name", list(tref.CONFIGS))
def test_step_against_reference_golden(mods, golden, name):
    """Nothing injected: where the device's lists equal the reference's by distance, the same bounds against the
    golden's stored entries (0.46, 0.21 and 0.28 x of them on the three configurations)."""
    g = case(golden, name)[0]
    if lists_differ_from_golden(mods, golden, name).any():
        return                                          # (counted by the next test; the count is reported above)
    fails = check_step(f"{name} vs the reference's golden, nothing injected", g, device_step(mods, golden, name),
                       lambda key, grad: tref.golden_views(g, key, grad), g["out64"],
                       {key: g[f"buf/{key}"] for key in tref.buffer_names()})
    assert not fails, "\n".join(fails)


def test_device_lists_agree_with_the_reference_on_two_of_three(mods, golden):
    agree = [name for name in tref.CONFIGS if not lists_differ_from_golden(mods, golden, name).any()]
    assert len(agree) >= 2, f"the device's lists agree with the reference's by distance on {agree} only"


# ------------------------------------------------------------------------------------------ 6. repeatability, isolation
def test_repeatability_and_isolation(mods, golden):
    g, k, emb, x = case(golden, "k8_b5_ellipsoid")
    xd = torch.as_tensor(x, dtype=torch.float32).to(mods["dev"])
    gt = torch.as_tensor(g["gt"], dtype=torch.float32).to(mods["dev"])
    runs = []
    for _ in range(2):
        model = new_model(mods, k, emb).train()
        out = model(xd)
        device_loss(out, gt).backward()
        runs.append((out.detach(), [p.grad for p in model.parameters()], [b_ for b_ in model.buffers()]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b_) for a, b_ in zip(runs[0][1], runs[1][1]))
    assert all(torch.equal(a, b_) for a, b_ in zip(runs[0][2], runs[1][2]))
    assert all(p.grad is not None for p in model.parameters())                  # gradients reach every parameter
    # eval() of a trainable model is the inference path, bit for bit; its state dict is the plain model's
    plain = new_model(mods, k, emb, trainable=False).eval()
    train = new_model(mods, k, emb, trainable=True).eval()
    assert list(plain.state_dict()) == list(train.state_dict())
    assert torch.equal(plain(xd), train(xd))
    # ... also after training changed its weights and buffers (the packed weights follow)
    plain.load_state_dict(model.state_dict(), strict=True)
    assert torch.equal(plain(xd), model.eval()(xd))
    # a backward consumes the step's workspace
    model.train()
    out = model(xd)
    out.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="consumed"):
        out.sum().backward()
    # the default model in train() still raises
    plain.train()
    with pytest.raises(NotImplementedError, match="eval"):
        plain(xd)


# ------------------------------------------------------------------------------------------ 7. one optimiser step
def _adam_first_step(g, eps=1e-8):
    """Adam's first update direction (bias-corrected m / (sqrt(v) + eps) at step 1)."""
    return g / (np.abs(g) + eps)


def test_one_adam_step(mods, golden):
    """One Adam step on the device against torch.optim.Adam on the restatement's gradients.  Adam's first step moves
    an entry by lr u(g), u(g) = g / (|g| + 1e-8), whatever the size of g: test 4's bound t on a gradient entry is
    carried through that update, lr max |u(g +- t) - u(g)| on the parameter.  Next to it stands float32's own
    arithmetic of the update on the device: the parameter's rounding (2 u |p|) and about ten roundings on the way to
    the step (the two moments, the square, the root, two bias corrections, + eps, the quotient, the step size, the
    subtraction), 16 u lr."""
    name, lr = "k8_b5_ellipsoid", 1e-3
    nat = mods["nat"]
    g, k, emb, x = case(golden, name)
    xd = torch.as_tensor(x, dtype=torch.float32).to(mods["dev"])
    gt = torch.as_tensor(g["gt"], dtype=torch.float32).to(mods["dev"])
    model = new_model(mods, k, emb).train()
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    packs = nat.host_packs
    out, dbg = model(xd, debug=True)
    device_loss(out, gt).backward()
    opt.step()
    want = restated(golden, name, dbg["lists"].cpu().numpy())
    state = cases.make_state(cases.SEED, k, emb)
    ref_params = {key: torch.nn.Parameter(torch.as_tensor(np.asarray(state[key]), dtype=torch.float64))
                  for key in tref.param_names()}
    for key, p in ref_params.items():
        p.grad = torch.as_tensor(want["grads"][key])
    torch.optim.Adam(list(ref_params.values()), lr=lr).step()
    named = dict(model.named_parameters())
    worst = 0.0
    for key in tref.param_names():
        gr = want["grads"][key]
        t = 8 * float(g[f"gdev32/{key}"]) * float(g[f"gscale/{key}"])
        u0 = _adam_first_step(gr)
        bound = lr * np.maximum(np.abs(_adam_first_step(gr + t) - u0), np.abs(_adam_first_step(gr - t) - u0)) \
            + 2 * U * np.abs(ref_params[key].detach().numpy()) + 16 * U * lr
        err = np.abs(named[key].detach().cpu().numpy().astype(np.float64) - ref_params[key].detach().numpy())
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"{key}: {float((err / bound).max()):.2f} x the bound"
        moved = np.abs(named[key].detach().cpu().numpy() - np.asarray(state[key])).max()
        if tref.scale_name(key) == key:                                          # (not the two all-noise biases)
            assert moved > 0.5 * lr, key                                         # every tensor took its step
    # the next forward runs on the new weights, packed on the device
    out2, dbg2 = model(xd, debug=True)
    new_state = dict(state)
    new_state.update({key: named[key].detach().cpu().numpy() for key in tref.param_names()})
    new_state.update({key: v.cpu().numpy() for key, v in model.state_dict().items() if "running" in key})
    # (the buffers of the first step are the second step's starting buffers: only the output is compared here)
    want2 = tref.step(new_state, x.astype(np.float32), g["gt"].astype(np.float32), dbg2["lists"].cpu().numpy())
    err2 = float(np.abs(out2.detach().cpu().numpy() - want2["out"]).max())
    tol2 = 8 * float(g["outdev32"]) * float(np.abs(want2["out"]).max())
    report(f"dgcnn train Adam step: worst parameter error / bound {worst:.3f}; next forward {err2:.2e} (bound {tol2:.2e})")
    assert err2 <= tol2
    assert float((out2.detach() - out.detach()).abs().max()) > 0
    assert nat.host_packs == packs, "a train() step packed weights through the host"


# ------------------------------------------------------------------------------------------ 8. the trainer
def test_trainer_and_checkpoint_round_trip(mods, golden, tmp_path):
    inputs, size = cases.fixture_inputs(golden, "ellipsoid")
    rows = cases.config_rows("k8_emb1024_ellipsoid", size)
    assert len(rows) == 16
    dev = mods["dev"]
    x = torch.as_tensor(np.transpose(inputs[rows], (0, 2, 1)), dtype=torch.float32).to(dev)    # [16, 64, 20] rows
    gt = torch.as_tensor(tref.unit_vectors("trainer", 16), dtype=torch.float32).to(dev)
    model = new_model(mods, 8, 128)
    net = mods["Network"](model)
    losses = mods["NetworkTrainer"](net, [(x, gt)]).train(20, Adam_learning_rate=1e-3, loss_based_on_value_loss=0.5)
    assert len(losses) == 20 and all(np.isfinite(l).all() for l in losses)
    report(f"dgcnn trainer: MSE {losses[0][1]:.4f} -> {losses[-1][1]:.4f}, cosine {losses[0][0]:.4f} -> {losses[-1][0]:.4f}")
    assert losses[-1][1] < losses[0][1]
    assert int(model.bn1.num_batches_tracked) == 20 and int(model.bn9.num_batches_tracked) == 20
    path = str(tmp_path / "nets" / "trained.t7")
    net.saveModel(path)
    with pytest.raises(ValueError):
        net.saveModel(path)                                                     # never over an existing file
    with pytest.raises(ValueError):
        net.saveModel(str(tmp_path / "trained.pt"))
    other = mods["Network"](mods["DGCNN"](8, 17, 128, 0.5).to(dev).eval())      # trainable=False
    other.loadModel(path)
    with pytest.raises(ValueError):
        other.loadModel(str(tmp_path / "missing.t7"))
    xin = x.permute(0, 2, 1).contiguous()
    assert torch.equal(other.getModel()(xin), model.eval()(xin))
    with pytest.raises(ValueError, match="trainable"):
        mods["NetworkTrainer"](other, [(x, gt)]).train(1)


# ------------------------------------------------------------------------------------------ 9. arguments
def test_arguments(mods, golden):
    nat, dev = mods["nat"], mods["dev"]
    g, k, emb, x = case(golden, "k1_b2_ellipsoid")
    xd = torch.as_tensor(x, dtype=torch.float32).to(dev)
    model = new_model(mods, k, emb).train()
    before = {key: v.clone() for key, v in model.state_dict().items()}

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(v, before[key]) for key, v in model.state_dict().items())

    with pytest.raises(ValueError, match="requires_grad"):
        model(xd.clone().requires_grad_(True))
    assert untouched()
    model.bn3.momentum = None
    try:
        with pytest.raises(ValueError, match="momentum"):
            model(xd)
    finally:
        model.bn3.momentum = 0.1
    assert untouched()
    for bad in (64.0, -1.0, float("nan")):
        xb = xd.clone()
        xb[1, 18, 7] = bad
        with pytest.raises(ValueError, match="patch 1 "):
            model(xb)
        assert untouched()
    with pytest.raises(ValueError):
        model(xd[:, :19])
    with pytest.raises(ValueError):
        model(xd.cpu())
    # the native entry: a short or misaligned workspace writes nothing
    conv = [getattr(model, f"conv{i}")[0].weight.detach() for i in range(1, 8)]
    bns = [getattr(model, f"bn{i}") for i in range(1, 8)]
    bn = [(m.weight.detach(), m.bias.detach(), m.running_mean, m.running_var, m.num_batches_tracked, m.eps, m.momentum)
          for m in bns]
    need = nat.dgcnn_train_workspace_bytes(k, emb, len(x))
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="workspace"):
        nat.dgcnn_train_forward(conv, bn, k, emb, xd, ws[:need - 256])
    with pytest.raises(ValueError, match="aligned"):
        nat.dgcnn_train_forward(conv, bn, k, emb, xd, ws[4:])
    with pytest.raises(ValueError, match="workspace"):
        nat.dgcnn_train_forward(conv, bn, k, emb, xd, torch.empty(need, dtype=torch.uint8))
    assert untouched()
    with pytest.raises(ValueError, match="workspace"):
        nat.dgcnn_train_backward(conv, k, emb, xd, torch.zeros((len(x), 2 * emb), device=dev), ws[:need - 256])
    pooled = nat.dgcnn_train_forward(conv, bn, k, emb, xd, ws)
    assert tuple(pooled.shape) == (len(x), 2 * emb) and not untouched()
    with pytest.raises(ValueError):
        nat.dgcnn_wgrad(torch.zeros((2, 4, 64), device=dev), torch.zeros((3, 4, 64), device=dev))
