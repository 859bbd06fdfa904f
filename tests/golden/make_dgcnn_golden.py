"""Generate tests/golden/dgcnn_*.npz by running the REFERENCE's DGCNN (PatchGeneration/Modules/Network/GCNModel.py).

TEST INFRASTRUCTURE ONLY (build container, needs the reference checkout, as make_patch_golden.py does).  The reference
module runs unmodified on the CPU, in float64 (model.double()) and in float32, on the committed patch inputs with the
weights of tests/dgcnn_cases.make_state.  The only shim: get_graph_feature_idx hard-codes torch.device('cuda'), so the
module is handed a `torch` whose device() returns the CPU device.  Its knn is wrapped to record the lists it returns.

Per configuration of dgcnn_cases.CONFIGS one file dgcnn_<name>.npz:
  rows            the fixture's input rows the configuration runs
  out64, out32    [n, 3] the reference's float64 and float32 outputs
  lists64         [3, n, 64, k] uint8, the float64 run's neighbour lists of layers 4-6
  differs32       [n] bool: the float32 run picked, somewhere, a neighbour at another distance than the float64 run
  dev32_stable, dev32_all   max |out32 - out64| over the patches where no neighbour differs / over all patches -- of
                  the whole fixture (both runs take every stored patch of it), not only of `rows`
  act_rows        the two rows (one padded where the fixture has padded patches, one full) whose float64 activations
                  are stored: pooled [2, 2 emb], h1, h2, h3 here, the concatenation [1024, 64] of each in
                  dgcnn_<name>_act<0|1>.npz (half a MiB each, so a file of its own)
The generator asserts that tests/dgcnn_ref.forward equals the float64 run to 1e-12 on every patch, with the golden's
lists injected and without.  Every file stays under 1 MiB.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import dgcnn_cases as cases  # noqa: E402
import dgcnn_ref as ref  # noqa: E402

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
_knn_log = []
_ref_knn = GCNModel.knn


def _logging_knn(x, k):
    idx = _ref_knn(x, k)
    _knn_log.append(idx.detach().clone())
    return idx


GCNModel.knn = _logging_knn


def close(a, b, what):
    tol = 1e-12 * max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    return err


def run_reference(state, k, emb, x, dtype):
    model = GCNModel.DGCNN(k, 17, emb, 0.5)
    model.load_state_dict({key: torch.as_tensor(np.asarray(v)) for key, v in state.items()}, strict=True)
    model = model.to(dtype).eval()
    acts = {}
    hooks = []
    for i in range(1, 7):
        hooks.append(getattr(model, f"conv{i}").register_forward_hook(
            lambda m, a, o, i=i: acts.__setitem__(f"x{i}", o.max(dim=-1)[0].detach())))
    hooks.append(model.conv7.register_forward_hook(lambda m, a, o: acts.__setitem__("y7", o.detach())))
    for i in range(1, 4):
        hooks.append(getattr(model, f"bn{7 + i}").register_forward_hook(
            lambda m, a, o, i=i: acts.__setitem__(f"h{i}", torch.nn.functional.leaky_relu(o.detach(), 0.2))))
    _knn_log.clear()
    with torch.no_grad():
        out = model(torch.as_tensor(x).to(dtype))
    for h in hooks:
        h.remove()
    lists = np.stack([t.numpy() for t in _knn_log])
    assert lists.shape == (3, len(x), 64, k)
    a = {key: v.numpy() for key, v in acts.items()}
    a["cat"] = np.concatenate([a[f"x{i}"] for i in range(1, 7)], 1)
    a["pooled"] = np.concatenate([a["y7"].max(-1), a["y7"].mean(-1)], 1)
    return out.numpy(), lists, a


def main(names):
    def load(name):
        return np.load(os.path.join(HERE, name + ".npz"))

    for name in names:
        k, emb, fixture, _ = cases.CONFIGS[name]
        inputs, size = cases.fixture_inputs(load, fixture)
        rows = cases.config_rows(name, size)
        state = cases.make_state(cases.SEED, k, emb)
        # both runs over ALL of the fixture's patches: the float32 run's deviation figures are the fixture's
        out64, lists64, a64 = run_reference(state, k, emb, inputs, torch.float64)
        out32, lists32, _ = run_reference(state, k, emb, inputs.astype(np.float32), torch.float32)
        # the float32 run against the float64 run, through distances on the float64 layer inputs
        differs = np.zeros(len(inputs), bool)
        for layer, (lo, hi) in enumerate(ref.DYN_INPUT):
            differs |= ref.lists_differ(a64["cat"][:, lo:hi], lists64[layer], lists32[layer]).any(-1)
        dev = np.abs(out32.astype(np.float64) - out64).max(-1)
        stable = float(dev[~differs].max()) if (~differs).any() else 0.0
        n_differs = int(differs.sum())
        # stored and restated: the configuration's rows
        x, out64, out32, lists64, differs = inputs[rows], out64[rows], out32[rows], lists64[:, rows], differs[rows]
        a64 = {key: v[rows] for key, v in a64.items()}
        # the restatement: lists injected, then its own search
        o_inj, f_inj = ref.forward(state, x, k, lists=lists64, full=True)
        o_own, f_own = ref.forward(state, x, k, full=True)
        e1 = close(o_inj, out64, f"{name}: restatement (lists injected) outputs")
        e2 = close(o_own, out64, f"{name}: restatement (own lists) outputs")
        for key in ("cat", "pooled", "h1", "h2", "h3"):
            close(f_inj[key], a64[key], f"{name}: restatement (lists injected) {key}")
            close(f_own[key], a64[key], f"{name}: restatement (own lists) {key}")
        own_differs = np.zeros(len(x), bool)
        for layer, (lo, hi) in enumerate(ref.DYN_INPUT):
            own_differs |= ref.lists_differ(a64["cat"][:, lo:hi], lists64[layer], f_own["lists"][layer]).any(-1)
        assert not own_differs.any(), f"{name}: the restatement's own lists differ by distance on {own_differs.sum()}"
        padded, full = np.nonzero(size[rows] < 64)[0], np.nonzero(size[rows] >= 64)[0]
        act_rows = np.array([padded[0] if len(padded) else full[1], full[0]])
        np.savez_compressed(
            os.path.join(HERE, f"dgcnn_{name}.npz"), rows=rows, out64=out64, out32=out32,
            lists64=lists64.astype(np.uint8), differs32=differs, dev32_stable=np.float64(stable),
            dev32_all=np.float64(dev.max()), act_rows=act_rows,
            **{key: a64[key][act_rows] for key in ("pooled", "h1", "h2", "h3")})
        for slot, r in enumerate(act_rows):
            np.savez_compressed(os.path.join(HERE, f"dgcnn_{name}_act{slot}.npz"), cat=a64["cat"][r])
        print(f"{name}: {len(x)} patches ({int((size[rows] < 64).sum())} padded), |out| max {np.abs(out64).max():.3f}, "
              f"float32 differs on {n_differs} of the fixture's {len(inputs)}, dev32 stable {stable:.2e} all {dev.max():.2e}, "
              f"restatement {e1:.1e} / {e2:.1e}")
    for fn in os.listdir(HERE):
        if fn.startswith("dgcnn_") and fn.endswith(".npz"):
            assert os.path.getsize(os.path.join(HERE, fn)) < 1 << 20, fn


if __name__ == "__main__":
    main(tuple(sys.argv[1:]) or tuple(cases.CONFIGS))
