"""Generate tests/golden/better_dgcnn_*.npz by running the REFERENCE's BetterDGCNN
(PatchGeneration/Modules/Network/GCNModel.py:217-297).

TEST INFRASTRUCTURE ONLY (build container, needs the reference checkout, as make_dgcnn_golden.py does).  The reference
module runs unmodified on the CPU, in float64 and in float32, on the committed ellipsoid patch inputs with the weights
of tests/better_dgcnn_cases.make_state.  The shims are make_dgcnn_golden.py's and make_dgcnn_train_golden.py's: a
`torch` whose device() names the CPU, and a knn wrapper that records the lists or returns injected ones.  One more
setting: BetterDGCNN.forward allocates the concatenation with the default dtype, so the float64 run is constructed and
called under torch.set_default_dtype(torch.float64).

Inference, per configuration of better_dgcnn_cases.CONFIGS one file better_dgcnn_<name>.npz:
  rows            the fixture's input rows the configuration runs
  out64, out32    [n, 3] the reference's float64 and float32 outputs
  lists64         [l_d, n, 64, k] uint8, the float64 run's neighbour lists of the dynamic layers
  differs32       [n] bool: the float32 run picked, somewhere, a neighbour at another distance than the float64 run
  dev32_stable, dev32_all   max |out32 - out64| over the patches where no neighbour differs / over all patches -- of
                  the whole fixture, not only of `rows`
  act_rows        the two rows (one padded, one full) whose float64 activations are stored: pooled, h1 .. and the
                  concatenation `cat` [2, Ccat, 64] (for `default` in better_dgcnn_default_act<0|1>.npz)
  sd_keys, sd_shapes   the reference module's state-dict keys and their shapes ("64,34,1,1")
Training (dropout 0.0, loss weights 0.5 / 0.5), per entry of better_dgcnn_cases.TRAIN one file
better_dgcnn_train_<name>.npz with the fields of make_dgcnn_train_golden.py (rows, gt, out64, loss64, lists64, buf/,
grad/ or sample/ + sum/ + l2/, gscale/, gdev32/, outdev32, bufdev32/, differs32).
The generator asserts that tests/better_dgcnn_ref equals the float64 runs: to 1e-12 on outputs and activations, with
the golden's lists injected and with its own; to 1e-10 gscale on every gradient, and 1e-10 on every buffer.  Every file
stays under 1 MiB.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import better_dgcnn_cases as cases  # noqa: E402
import better_dgcnn_ref as bref  # noqa: E402
import dgcnn_train_ref as tref  # noqa: E402

sys.path.insert(0, REF)
from PatchGeneration.Modules.Network import GCNModel  # noqa: E402


class _CpuTorch:
    """torch, except that device() names the CPU."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def device(*a, **k):
        return torch.device("cpu")


GCNModel.torch = _CpuTorch()
_knn_log, _knn_inject = [], []
_ref_knn = GCNModel.knn


def _wrapped_knn(x, k):
    idx = _knn_inject.pop(0) if _knn_inject else _ref_knn(x, k)
    _knn_log.append(idx.detach().clone())
    return idx


GCNModel.knn = _wrapped_knn


def close(a, b, what):
    tol = 1e-12 * max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    return err


def reldev(a, b, scale=None):
    return float(np.abs(a - b).max() / max(np.abs(b).max() if scale is None else scale, 1e-300))


def build(name, state, dropout, dtype):
    t = cases.Table(name)
    model = GCNModel.BetterDGCNN(t.l_e, t.l_d, t.l_l, torch.tensor(t.sizes), t.k, 17, dropout)
    model.load_state_dict({key: torch.as_tensor(np.asarray(v)) for key, v in state.items()}, strict=True)
    return t, model.to(dtype)


def run_eval(name, state, x, dtype):
    torch.set_default_dtype(dtype)
    try:
        t, model = build(name, state, 0.5, dtype)
        model.eval()
        acts, hooks = {}, []
        for i in range(1, t.E + 1):
            hooks.append(getattr(model, f"conv{i}").register_forward_hook(
                lambda m, a, o, i=i: acts.__setitem__(f"x{i}", o.max(dim=-1)[0].detach())))
        hooks.append(getattr(model, f"conv{t.E + 1}").register_forward_hook(
            lambda m, a, o: acts.__setitem__("y", o.detach())))
        for j in range(1, t.l_l):
            hooks.append(getattr(model, f"bn{t.E + 1 + j}").register_forward_hook(
                lambda m, a, o, j=j: acts.__setitem__(f"h{j}", F.leaky_relu(o.detach()))))
        _knn_log.clear()
        _knn_inject.clear()
        with torch.no_grad():
            out = model(torch.as_tensor(x).to(dtype))
        for h in hooks:
            h.remove()
        sd = [(key, ",".join(str(int(s)) for s in v.shape)) for key, v in model.state_dict().items()]
    finally:
        torch.set_default_dtype(torch.float32)
    lists = np.stack([v.numpy() for v in _knn_log]) if _knn_log else np.zeros((0, len(x), 64, t.k), np.int64)
    assert lists.shape == (t.l_d, len(x), 64, t.k)
    a = {key: v.numpy() for key, v in acts.items()}
    a["cat"] = np.concatenate([a[f"x{i}"] for i in range(1, t.E + 1)], 1)
    a["pooled"] = np.concatenate([a["y"].max(-1), a["y"].mean(-1)], 1)
    return out.numpy(), lists, a, sd


def run_train(name, state, x, gt, dtype, inject=None):
    """One train() forward + backward of the reference: (out, loss, grads, buffers, lists)."""
    torch.set_default_dtype(dtype)
    try:
        t, model = build(name, state, 0.0, dtype)
        model.train()
        _knn_log.clear()
        _knn_inject.clear()
        if inject is not None:
            _knn_inject.extend(torch.as_tensor(np.asarray(l).astype(np.int64)) for l in inject)
        out = model(torch.as_tensor(x).to(dtype))
        gt = torch.as_tensor(gt).to(dtype)
        loss = tref.LOSS_WEIGHTS[0] * F.cosine_embedding_loss(out, gt, torch.ones(len(x), dtype=dtype)) + \
            tref.LOSS_WEIGHTS[1] * F.mse_loss(out, gt)
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    named = dict(model.named_parameters())
    grads = {key: named[key].grad.numpy().astype(np.float64) for key in bref.param_names(name)}
    sd = model.state_dict()
    buffers = {key: sd[key].numpy().astype(np.float64) for key in bref.buffer_names(name)}
    lists = np.stack([v.numpy() for v in _knn_log]) if _knn_log else np.zeros((0, len(x), 64, t.k), np.int64)
    assert lists.shape == (t.l_d, len(x), 64, t.k) and not _knn_inject
    return out.detach().numpy().astype(np.float64), float(loss.detach()), grads, buffers, lists


def load(name):
    return np.load(os.path.join(HERE, name + ".npz"))


def make_eval(name):
    t = cases.Table(name)
    inputs, size = cases.fixture_inputs(load)
    rows = cases.config_rows(size)
    state = cases.make_state(name)
    # both runs over ALL of the fixture's patches: the float32 run's deviation figures are the fixture's
    out64, lists64, a64, sd = run_eval(name, state, inputs, torch.float64)
    out32, lists32, _, _ = run_eval(name, state, inputs.astype(np.float32), torch.float32)
    differs = bref.lists_differ(name, inputs, a64["cat"], lists64, lists32)
    dev = np.abs(out32.astype(np.float64) - out64).max(-1)
    stable = float(dev[~differs].max()) if (~differs).any() else 0.0
    n_differs = int(differs.sum())
    x, out64, out32, lists64, differs = inputs[rows], out64[rows], out32[rows], lists64[:, rows], differs[rows]
    a64 = {key: v[rows] for key, v in a64.items()}
    o_inj, f_inj = bref.forward(name, state, x, lists=lists64, full=True)
    o_own, f_own = bref.forward(name, state, x, full=True)
    e1 = close(o_inj, out64, f"{name}: restatement (lists injected) outputs")
    e2 = close(o_own, out64, f"{name}: restatement (own lists) outputs")
    hidden = [f"h{j}" for j in range(1, t.l_l)]
    for key in ["cat", "pooled"] + hidden:
        close(f_inj[key], a64[key], f"{name}: restatement (lists injected) {key}")
        close(f_own[key], a64[key], f"{name}: restatement (own lists) {key}")
    own_differs = bref.lists_differ(name, x, a64["cat"], lists64, f_own["lists"])
    assert not own_differs.any(), f"{name}: the restatement's own lists differ by distance on {own_differs.sum()}"
    padded, full = np.nonzero(size[rows] < 64)[0], np.nonzero(size[rows] >= 64)[0]
    act_rows = np.array([padded[0] if len(padded) else full[1], full[0]])
    store = dict(rows=rows, out64=out64, out32=out32, lists64=lists64.astype(np.uint8), differs32=differs,
                 dev32_stable=np.float64(stable), dev32_all=np.float64(dev.max()), act_rows=act_rows,
                 sd_keys=np.array([k for k, _ in sd]), sd_shapes=np.array([s for _, s in sd]),
                 **{key: a64[key][act_rows] for key in ["pooled"] + hidden})
    if t.ccat <= 512:
        store["cat"] = a64["cat"][act_rows]
    else:
        for slot, r in enumerate(act_rows):
            np.savez_compressed(os.path.join(HERE, f"better_dgcnn_{name}_act{slot}.npz"), cat=a64["cat"][r])
    np.savez_compressed(os.path.join(HERE, f"better_dgcnn_{name}.npz"), **store)
    print(f"{name}: {len(x)} patches ({int((size[rows] < 64).sum())} padded), |out| max {np.abs(out64).max():.3f}, "
          f"float32 differs on {n_differs} of the fixture's {len(inputs)}, dev32 stable {stable:.2e} all {dev.max():.2e}, "
          f"restatement {e1:.1e} / {e2:.1e}")


def make_train(name):
    inputs, size = cases.fixture_inputs(load)
    rows = cases.train_rows(name, size)
    x = inputs[rows]
    gt = tref.unit_vectors("better_" + name, len(rows))
    state = cases.make_state(name)
    names = bref.param_names(name)
    out64, loss64, g64, b64, lists64 = run_train(name, state, x, gt, torch.float64)
    r = bref.step(name, state, x, gt, lists64, full=True)
    assert reldev(r["out"], out64) <= 1e-10 and abs(r["loss"] - loss64) <= 1e-10 * abs(loss64), name
    worst = 0.0
    scale = {key: float(np.abs(g64[bref.scale_name(name, key)]).max()) for key in names}
    for key in names:
        assert r["grads"][key].shape == g64[key].shape, key
        dev = reldev(r["grads"][key], g64[key], scale[key])
        worst = max(worst, dev)
        assert dev <= 1e-10, (name, key, dev)
    for key in bref.buffer_names(name):
        assert reldev(r["buffers"][key], b64[key]) <= 1e-10, (name, key)
    out32, _, g32, b32, _ = run_train(name, state, x.astype(np.float32), gt, torch.float32, inject=lists64)
    _, _, _, _, own32 = run_train(name, state, x.astype(np.float32), gt, torch.float32)
    differs = bref.lists_differ(name, x, r["cat"], lists64, own32)
    store = {"rows": rows, "gt": gt, "out64": out64, "loss64": np.float64(loss64),
             "lists64": lists64.astype(np.uint8), "outdev32": np.float64(reldev(out32, out64)), "differs32": differs}
    for key in bref.buffer_names(name):
        store[f"buf/{key}"] = b64[key]
        store[f"bufdev32/{key}"] = np.float64(reldev(b32[key], b64[key]))
    for key in names:
        g = g64[key]
        store[f"gscale/{key}"] = np.float64(scale[key])
        store[f"gdev32/{key}"] = np.float64(reldev(g32[key], g, scale[key]))
        if g.size <= tref.FULL_LIMIT:
            store[f"grad/{key}"] = g
        else:
            store[f"sample/{key}"] = g.reshape(-1)[tref.sample_index(key, g.size)]
            store[f"sum/{key}"] = np.float64(g.sum())
            store[f"l2/{key}"] = np.float64(np.sqrt((g * g).sum()))
    path = os.path.join(HERE, f"better_dgcnn_train_{name}.npz")
    np.savez_compressed(path, **store)
    gd = {key: float(store[f"gdev32/{key}"]) for key in names}
    print(f"train {name}: {len(rows)} patches ({int((size[rows] < 64).sum())} padded), loss {loss64:.6f}, restatement "
          f"worst gradient deviation {worst:.1e}, outdev32 {float(store['outdev32']):.2e}, gdev32 "
          f"{min(gd.values()):.2e} .. {max(gd.values()):.2e} ({max(gd, key=gd.get)}), float32's own lists differ "
          f"on {int(differs.sum())} rows, {os.path.getsize(path) >> 10} KiB")


def main(names):
    for name in names:
        if name in cases.CONFIGS:
            make_eval(name)
    for name in names:
        if name in cases.TRAIN:
            make_train(name)
    for fn in os.listdir(HERE):
        if fn.startswith("better_dgcnn_") and fn.endswith(".npz"):
            assert os.path.getsize(os.path.join(HERE, fn)) < 1 << 20, fn


if __name__ == "__main__":
    main(tuple(sys.argv[1:]) or tuple(cases.CONFIGS))
