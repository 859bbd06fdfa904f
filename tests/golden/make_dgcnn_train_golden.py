"""Generate tests/golden/dgcnn_train_*.npz by running the REFERENCE's DGCNN in train() (one forward + backward).

TEST INFRASTRUCTURE ONLY (build container, needs the reference checkout, as make_dgcnn_golden.py does).  The
reference module runs unmodified on the CPU with dropout 0.0, in float64 and in float32, on the committed patch inputs
with the weights of tests/dgcnn_cases.make_state, seeded unit vectors as ground truth and the trainer's loss
(NetworkController.py:124-134) at weights 0.5 / 0.5.  The shims are make_dgcnn_golden.py's: a `torch` whose device()
names the CPU, and a knn wrapper that records the lists -- or, for the float32 run, returns the float64 run's lists,
so that only rounding differs between the two.

Per configuration of dgcnn_train_ref.CONFIGS one file dgcnn_train_<name>.npz:
  rows, gt        the fixture's input rows and the ground-truth normals
  out64, loss64   the float64 run's output [n, 3] and loss
  lists64         [3, n, 64, k] uint8, the float64 run's neighbour lists of layers 4-6
  buf/<name>      the updated running_mean / running_var of bn1-10
  grad/<name>     every gradient of at most 16,384 elements in full; for a larger one sample/<name> (the 4,096 seeded
                  entries of dgcnn_train_ref.sample_index), sum/<name> and l2/<name>
  gscale/<name>   max |g64|, the scale every comparison of that gradient is relative to -- but for linear2.bias and
                  linear3.bias, which a batch norm follows: their gradient is zero in exact arithmetic, what any run
                  returns is rounding noise (1e-17 in float64), and the scale is that of the layer's weight gradient
  gdev32/<name>   max |g32 - g64| / gscale of the float32 run with the float64 lists injected; outdev32 and
                  bufdev32/<name> the same for the output and the buffers (relative to their own max)
  differs32       rows on which the float32 run's OWN search picks a neighbour at another distance than lists64
The generator asserts that tests/dgcnn_train_ref.step equals the float64 run on every element of the output, of
every gradient (to 1e-10 gscale) and of every buffer.  Every file stays under 1 MiB.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import dgcnn_cases as cases  # noqa: E402
import dgcnn_ref as ref  # noqa: E402
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


def run_reference(state, k, emb, x, gt, dtype, inject=None):
    """One train() forward + backward of the reference: (out, loss, grads, buffers, lists)."""
    model = GCNModel.DGCNN(k, 17, emb, 0.0)
    model.load_state_dict({key: torch.as_tensor(np.asarray(v)) for key, v in state.items()}, strict=True)
    model = model.to(dtype).train()
    _knn_log.clear()
    _knn_inject.clear()
    if inject is not None:
        _knn_inject.extend(torch.as_tensor(np.asarray(l).astype(np.int64)) for l in inject)
    out = model(torch.as_tensor(x).to(dtype))
    gt = torch.as_tensor(gt).to(dtype)
    loss = tref.LOSS_WEIGHTS[0] * F.cosine_embedding_loss(out, gt, torch.ones(len(x), dtype=dtype)) + \
        tref.LOSS_WEIGHTS[1] * F.mse_loss(out, gt)
    loss.backward()
    named = dict(model.named_parameters())
    grads = {key: named[key].grad.numpy().astype(np.float64) for key in tref.param_names()}
    sd = model.state_dict()
    buffers = {key: sd[key].numpy().astype(np.float64) for key in tref.buffer_names()}
    lists = np.stack([t.numpy() for t in _knn_log])
    assert lists.shape == (3, len(x), 64, k) and not _knn_inject
    return out.detach().numpy().astype(np.float64), float(loss.detach()), grads, buffers, lists


def reldev(a, b, scale=None):
    return float(np.abs(a - b).max() / max(np.abs(b).max() if scale is None else scale, 1e-300))


def main(names):
    def load(name):
        return np.load(os.path.join(HERE, name + ".npz"))

    for name in names:
        k, emb, fixture = tref.CONFIGS[name][:3]
        inputs, size = cases.fixture_inputs(load, fixture)
        rows = tref.config_rows(name, size)
        x = inputs[rows]
        gt = tref.unit_vectors(name, len(rows))
        state = cases.make_state(cases.SEED, k, emb)
        out64, loss64, g64, b64, lists64 = run_reference(state, k, emb, x, gt, torch.float64)
        # the restatement on the reference's lists: every element of everything
        r = tref.step(state, x, gt, lists64, full=True)
        assert reldev(r["out"], out64) <= 1e-10 and abs(r["loss"] - loss64) <= 1e-10 * abs(loss64), name
        worst = 0.0
        scale = {key: float(np.abs(g64[tref.scale_name(key)]).max()) for key in tref.param_names()}
        for key in tref.param_names():
            assert r["grads"][key].shape == g64[key].shape, key
            dev = reldev(r["grads"][key], g64[key], scale[key])
            worst = max(worst, dev)
            assert dev <= 1e-10, (name, key, dev)
        for key in tref.buffer_names():
            assert reldev(r["buffers"][key], b64[key]) <= 1e-10, (name, key)
        # float32 with the float64 lists injected: only rounding differs
        out32, _, g32, b32, _ = run_reference(state, k, emb, x.astype(np.float32), gt, torch.float32, inject=lists64)
        # float32 with its own search: does it agree with lists64 by distance?
        _, _, _, _, own32 = run_reference(state, k, emb, x.astype(np.float32), gt, torch.float32)
        differs = np.zeros(len(rows), bool)
        for layer, (lo, hi) in enumerate(ref.DYN_INPUT):
            differs |= ref.lists_differ(r["cat"][:, lo:hi], lists64[layer], own32[layer]).any(-1)
        store = {"rows": rows, "gt": gt, "out64": out64, "loss64": np.float64(loss64),
                 "lists64": lists64.astype(np.uint8), "outdev32": np.float64(reldev(out32, out64)),
                 "differs32": differs}
        for key in tref.buffer_names():
            store[f"buf/{key}"] = b64[key]
            store[f"bufdev32/{key}"] = np.float64(reldev(b32[key], b64[key]))
        for key in tref.param_names():
            g = g64[key]
            store[f"gscale/{key}"] = np.float64(scale[key])
            store[f"gdev32/{key}"] = np.float64(reldev(g32[key], g, scale[key]))
            if g.size <= tref.FULL_LIMIT:
                store[f"grad/{key}"] = g
            else:
                store[f"sample/{key}"] = g.reshape(-1)[tref.sample_index(key, g.size)]
                store[f"sum/{key}"] = np.float64(g.sum())
                store[f"l2/{key}"] = np.float64(np.sqrt((g * g).sum()))
        path = os.path.join(HERE, f"dgcnn_train_{name}.npz")
        np.savez_compressed(path, **store)
        assert os.path.getsize(path) < 1 << 20, path
        gd = {key: float(store[f"gdev32/{key}"]) for key in tref.param_names()}
        print(f"{name}: {len(rows)} patches ({int((size[rows] < 64).sum())} padded), loss {loss64:.6f}, restatement "
              f"worst gradient deviation {worst:.1e}, outdev32 {float(store['outdev32']):.2e}, gdev32 "
              f"{min(gd.values()):.2e} .. {max(gd.values()):.2e} ({max(gd, key=gd.get)}), float32's own lists differ "
              f"on {int(differs.sum())} rows, {os.path.getsize(path) >> 10} KiB")


if __name__ == "__main__":
    main(tuple(sys.argv[1:]) or tuple(tref.CONFIGS))
