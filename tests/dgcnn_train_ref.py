"""A float64 restatement of one training step of DGCNN (GCNModel.py:170-215 in train(), the trainer's loss of
NetworkController.py:124-134), the checker of the device's train-mode forward and backward.

Written with torch ops on the CPU in the device's arrangement: the edge weight split into W_a (on x_j) and W_b - W_a
(on x_i), batch statistics over every edge of the batch, the affine before the max (gamma may be negative), arg-max
ties to the first slot.  The gradients are torch's autograd of exactly this forward.  The neighbour lists of the three
dynamic layers are always injected (they are constants of the backward), which takes the one discontinuous step out
of a comparison.
"""
import numpy as np
import torch
import torch.nn.functional as F

import dgcnn_cases as cases

MOMENTUM, EPS, SLOPE = 0.1, 1e-5, 0.2
LOSS_WEIGHTS = (0.5, 0.5)            # (cosine, mse): the trainer's loss_based_on_value_loss = 0.5

# name -> (k, emb_dims, fixture, padded patches, full patches): the smallest that reach every branch
CONFIGS = {
    "k8_b5_ellipsoid": (8, 128, "ellipsoid", 2, 3),
    "k1_b2_ellipsoid": (1, 128, "ellipsoid", 1, 1),
    "k20_b6_shells": (20, 128, "shells", 3, 3),
}
FULL_LIMIT, SAMPLE = 16384, 4096     # gradients above FULL_LIMIT elements are stored as SAMPLE entries + sum + norm


def config_rows(name, size):
    """The fixture rows of a configuration: its padded patches (fewer where the fixture has fewer), then full ones."""
    _, _, _, n_pad, n_full = CONFIGS[name]
    padded, full = np.nonzero(size < 64)[0], np.nonzero(size >= 64)[0]
    n_pad = min(n_pad, len(padded))
    return np.concatenate([padded[:n_pad], full[:CONFIGS[name][3] + n_full - n_pad]])


def unit_vectors(name, n):
    """The seeded ground-truth normals [n, 3] of a configuration."""
    rng = np.random.default_rng([cases.SEED, len(name), n])
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def sample_index(name, numel):
    """The seeded entries of a large gradient tensor that a golden stores."""
    rng = np.random.default_rng([cases.SEED, numel, sum(map(ord, name))])
    return np.sort(rng.choice(numel, SAMPLE, replace=False))


def param_names():
    names = []
    for i in range(1, 8):
        names += [f"conv{i}.0.weight", f"bn{i}.weight", f"bn{i}.bias"]
    for i in range(1, 4):
        names += [f"linear{i}.weight"] + ([f"linear{i}.bias"] if i > 1 else []) + [f"bn{7 + i}.weight", f"bn{7 + i}.bias"]
    return names + ["linear4.weight", "linear4.bias"]


def scale_name(name):
    """The tensor whose largest gradient entry is the scale of `name`'s comparisons: itself, but for the two linear
    biases that a batch norm follows -- their gradient is zero in exact arithmetic (the batch mean removes a constant),
    so what a run returns for them is rounding noise, measured against the layer's weight gradient."""
    return name.replace(".bias", ".weight") if name in ("linear2.bias", "linear3.bias") else name


def buffer_names():
    return [f"bn{i}.{what}" for i in range(1, 11) for what in ("running_mean", "running_var")]


def first_argmax(z):
    """The first maximal slot of the last axis (torch.argmax returns the first of equal values)."""
    return (z == z.max(-1, keepdim=True).values).to(torch.uint8).argmax(-1)


def batch_norm(y, gamma, beta, axes, eps=EPS):
    """Batch-statistic normalisation of y over `axes` (channel axis 1): (z, mean, biased var, count)."""
    shape = [1, -1] + [1] * (y.dim() - 2)
    mu, var = y.mean(axes), y.var(axes, unbiased=False)
    z = (y - mu.reshape(shape)) / torch.sqrt(var + eps).reshape(shape) * gamma.reshape(shape) + beta.reshape(shape)
    return z, mu, var, y.numel() // y.shape[1]


def running(state, i, mu, var, n, momentum=MOMENTUM):
    """nn.BatchNorm's buffer update: the unbiased variance n / (n - 1) goes into running_var."""
    rm = torch.as_tensor(np.asarray(state[f"bn{i}.running_mean"]), dtype=mu.dtype)
    rv = torch.as_tensor(np.asarray(state[f"bn{i}.running_var"]), dtype=mu.dtype)
    return {f"bn{i}.running_mean": (1 - momentum) * rm + momentum * mu.detach(),
            f"bn{i}.running_var": (1 - momentum) * rv + momentum * var.detach() * (n / (n - 1))}


def edge_terms(w, x):
    """(A, B) [b, out, 64] = (W_a x, (W_b - W_a) x) of a conv weight [out, 2 in(, 1, 1)] on x [b, in, 64]."""
    cin = x.shape[1]
    w2 = w.reshape(w.shape[0], -1)
    return w2[:, :cin] @ x, (w2[:, cin:] - w2[:, :cin]) @ x


def edge(w, gamma, beta, x, nbr, eps=EPS):
    """One edge layer in train() on x [b, in, 64] over nbr [b, 64, n] (int64):
    {"out" [b, out, 64], "arg" the first maximal slot, "mu", "var", "n", "A", "B", "y" [b, out, 64, n]}."""
    A, B = edge_terms(w, x)
    b, C = A.shape[:2]
    n = nbr.shape[-1]
    idx = nbr[:, None].expand(b, C, 64, n).reshape(b, C, 64 * n)
    y = torch.gather(A, 2, idx).reshape(b, C, 64, n) + B[..., None]
    z, mu, var, count = batch_norm(y, gamma, beta, (0, 2, 3), eps)
    arg = first_argmax(z)
    out = F.leaky_relu(torch.gather(z, 3, arg[..., None])[..., 0], SLOPE)
    return {"out": out, "arg": arg, "mu": mu, "var": var, "n": count, "A": A, "B": B, "y": y}


def index_lists(inputs):
    """The three index columns as lists [b, 64, 3] int64, truncated as .long() does."""
    return inputs[:, 17:20].long().permute(0, 2, 1).contiguous()


def trainer_loss(out, gt, weights=LOSS_WEIGHTS):
    ones = torch.ones(len(out), dtype=out.dtype)
    return weights[0] * F.cosine_embedding_loss(out, gt, ones) + weights[1] * F.mse_loss(out, gt)


def step(state, inputs, gt, lists, dtype=torch.float64, weights=LOSS_WEIGHTS, full=False):
    """One forward + backward in train() with dropout 0.  state: {key: array} (dgcnn_cases.make_state's keys);
    inputs [b, 20, 64]; gt [b, 3]; lists [3, b, 64, k] for layers 4-6.
    -> {"out" [b, 3], "loss", "grads" {parameter name: array}, "buffers" {bnN.running_mean / running_var: array}};
    full: also "cat" [b, 1024, 64], "pooled" [b, 2 emb] and the leaf tensors "params"."""
    P = {key: torch.as_tensor(np.asarray(state[key])).to(dtype).clone().requires_grad_(True) for key in param_names()}
    inputs = torch.as_tensor(np.asarray(inputs)).to(dtype)
    gt = torch.as_tensor(np.asarray(gt)).to(dtype)
    lists = torch.as_tensor(np.asarray(lists).astype(np.int64))
    x, idx = inputs[:, :17], index_lists(inputs)
    buffers, outs = {}, []
    for i in range(1, 7):
        e = edge(P[f"conv{i}.0.weight"], P[f"bn{i}.weight"], P[f"bn{i}.bias"], x, idx if i <= 3 else lists[i - 4])
        buffers.update(running(state, i, e["mu"], e["var"], e["n"]))
        x = e["out"]
        outs.append(x)
    cat = torch.cat(outs, 1)
    y = P["conv7.0.weight"].reshape(-1, 1024) @ cat
    z, mu, var, n = batch_norm(y, P["bn7.weight"], P["bn7.bias"], (0, 2))
    buffers.update(running(state, 7, mu, var, n))
    a = F.leaky_relu(z, SLOPE)
    first = first_argmax(a)
    pooled = torch.cat([torch.gather(a, 2, first[..., None])[..., 0], a.mean(-1)], 1)
    h = pooled
    for i in range(1, 4):
        h = h @ P[f"linear{i}.weight"].T
        if i > 1:
            h = h + P[f"linear{i}.bias"]
        h, mu, var, n = batch_norm(h, P[f"bn{7 + i}.weight"], P[f"bn{7 + i}.bias"], (0,))
        buffers.update(running(state, 7 + i, mu, var, n))
        h = F.leaky_relu(h, SLOPE)
    out = h @ P["linear4.weight"].T + P["linear4.bias"]
    loss = trainer_loss(out, gt, weights)
    grads = torch.autograd.grad(loss, [P[key] for key in param_names()])
    r = {"out": out.detach().numpy(), "loss": float(loss.detach()),
         "grads": {key: g.numpy() for key, g in zip(param_names(), grads)},
         "buffers": {key: v.numpy() for key, v in buffers.items()}}
    if full:
        r.update(cat=cat.detach().numpy(), pooled=pooled.detach().numpy())
    return r


def loss_only(state, inputs, gt, lists):
    """The loss of `step` alone (finite differences)."""
    return step(state, inputs, gt, lists)["loss"]


def golden_views(g, key, grad):
    """What a golden file stores of gradient `key`, next to the same views of `grad`: [(label, got, want, weight)].
    An error of at most e on every entry moves the sum by at most numel e and the L2 norm by at most sqrt(numel) e:
    `weight` is that factor, so one per-entry bound serves all three."""
    grad = np.asarray(grad, dtype=np.float64)
    if f"grad/{key}" in g.files:
        assert grad.shape == g[f"grad/{key}"].shape, key
        return [("every entry", grad, g[f"grad/{key}"], 1.0)]
    flat = grad.reshape(-1)
    return [("sampled entries", flat[sample_index(key, flat.size)], g[f"sample/{key}"], 1.0),
            ("sum", flat.sum(), float(g[f"sum/{key}"]), float(flat.size)),
            ("L2 norm", np.sqrt((flat * flat).sum()), float(g[f"l2/{key}"]), float(np.sqrt(flat.size)))]
