"""A float64 restatement of BetterDGCNN (GCNModel.py:217-297 of the reference): forward in eval() in numpy, and one
training step (train(), the trainer's loss of NetworkController.py:124-134) with torch ops on the CPU.

Both are dgcnn_ref / dgcnn_train_ref with the layer table of better_dgcnn_cases.Table in place of the fixed one: the
device's arrangement (the edge weight split into W_a and W_b - W_a, the batch norm folded into (s, t) or taken over
every edge of the batch, the affine before the max), the convolutions' LeakyReLU at 0.2 and the head's at 0.01.  The
neighbour lists of the dynamic layers may be injected (they must be, for the training step).
"""
import numpy as np
import torch
import torch.nn.functional as F

import dgcnn_ref as ref
import dgcnn_train_ref as tref
from better_dgcnn_cases import HEAD_SLOPE, Table


def lrelu(v, slope):
    return np.where(v > 0, v, slope * v)


def forward(name, state, inputs, lists=None, full=False, head_slope=HEAD_SLOPE):
    """inputs [b, 20, 64] -> out [b, out_ch] float64.  lists: None, or [l_d, b, 64, k] for the dynamic layers.
    full: also {"cat" [b, Ccat, 64], "lists" [l_d, b, 64, k], "pooled" [b, 2 C], "h1" .. [b, .]}."""
    t = Table(name)
    inputs = np.asarray(inputs, dtype=np.float64)
    if len(inputs) > 16:                               # (the [b, C, 64, 64] differences of knn stay small)
        parts = [forward(name, state, inputs[s:s + 16], None if lists is None else np.asarray(lists)[:, s:s + 16], True,
                         head_slope) for s in range(0, len(inputs), 16)]
        out = np.concatenate([p[0] for p in parts])
        if not full:
            return out
        return out, {key: np.concatenate([p[1][key] for p in parts], 1 if key == "lists" else 0) for key in parts[0][1]}
    x = inputs[:, :17]
    idx = ref.index_lists(inputs) if t.l_e else None   # (never read without static layers)
    outs, used = [], []
    for l in range(t.E):
        if l < t.l_e:
            nbr = idx
        else:
            nbr = ref.knn(x, t.k) if lists is None else np.asarray(lists[l - t.l_e]).astype(np.int64)
            used.append(nbr)
        x = ref.edge(state, l + 1, x, nbr)
        outs.append(x)
    cat = np.concatenate(outs, 1)
    wp = state[f"conv{t.E + 1}.0.weight"].astype(np.float64).reshape(t.emb, t.ccat)
    s, sh = ref.fold(state, t.E + 1)
    y = lrelu(s[None, :, None] * (wp @ cat) + sh[None, :, None], 0.2)
    pooled = np.concatenate([y.max(-1), y.mean(-1)], 1)
    h, hidden = pooled, []
    for j in range(1, t.l_l):
        s, sh = ref.fold(state, t.E + 1 + j, state.get(f"linear{j}.bias"))
        h = lrelu(s * (h @ state[f"linear{j}.weight"].astype(np.float64).T) + sh, head_slope)
        hidden.append(h)
    out = h @ state[f"linear{t.l_l}.weight"].astype(np.float64).T + state[f"linear{t.l_l}.bias"].astype(np.float64)
    if not full:
        return out
    r = {"cat": cat, "lists": np.stack(used) if used else np.zeros((0, len(inputs), 64, t.k), np.int64),
         "pooled": pooled}
    r.update({f"h{j}": v for j, v in enumerate(hidden, start=1)})
    return out, r


def dyn_layer_input(name, inputs, cat, d):
    """The input of dynamic layer d: rows 0:17 of `inputs` [b, 20, 64], or its slice of cat [b, Ccat, 64]."""
    where = Table(name).dyn_input(d)
    return np.asarray(inputs)[:, :17] if where is None else np.asarray(cat)[:, where[0]:where[1]]


def lists_differ(name, inputs, cat, a, b):
    """[b] bool: the patches on which list blocks a and b [l_d, b, 64, k] differ by distance in some dynamic layer."""
    t = Table(name)
    differs = np.zeros(len(inputs), bool)
    for d in range(t.l_d):
        differs |= ref.lists_differ(dyn_layer_input(name, inputs, cat, d), a[d], b[d]).any(-1)
    return differs


# ---------------------------------------------------------------------------------------------------- training
def param_names(name):
    t = Table(name)
    names = []
    for i in range(1, t.E + 2):
        names += [f"conv{i}.0.weight", f"bn{i}.weight", f"bn{i}.bias"]
    for j in range(1, t.l_l):
        names += [f"linear{j}.weight"] + ([f"linear{j}.bias"] if j > 1 else []) + \
            [f"bn{t.E + 1 + j}.weight", f"bn{t.E + 1 + j}.bias"]
    return names + [f"linear{t.l_l}.weight", f"linear{t.l_l}.bias"]


def scale_name(name, key):
    """dgcnn_train_ref.scale_name: a linear bias that a batch norm follows has a zero gradient in exact arithmetic, and
    is measured against the layer's weight gradient."""
    t = Table(name)
    hidden_biases = {f"linear{j}.bias" for j in range(2, t.l_l)}
    return key.replace(".bias", ".weight") if key in hidden_biases else key


def buffer_names(name):
    t = Table(name)
    return [f"bn{i}.{what}" for i in range(1, t.E + t.l_l + 1) for what in ("running_mean", "running_var")]


def step(name, state, inputs, gt, lists, dtype=torch.float64, weights=tref.LOSS_WEIGHTS, full=False,
         head_slope=HEAD_SLOPE):
    """One forward + backward in train() with dropout 0 (dgcnn_train_ref.step for a table).  lists [l_d, b, 64, k].
    -> {"out", "loss", "grads" {parameter name: array}, "buffers" {bnN.running_mean / running_var: array}};
    full: also "cat" and "pooled"."""
    t = Table(name)
    names = param_names(name)
    P = {key: torch.as_tensor(np.asarray(state[key])).to(dtype).clone().requires_grad_(True) for key in names}
    inputs = torch.as_tensor(np.asarray(inputs)).to(dtype)
    gt = torch.as_tensor(np.asarray(gt)).to(dtype)
    lists = torch.as_tensor(np.asarray(lists).astype(np.int64))
    x = inputs[:, :17]
    idx = tref.index_lists(inputs) if t.l_e else None
    buffers, outs = {}, []
    for l in range(t.E):
        i = l + 1
        e = tref.edge(P[f"conv{i}.0.weight"], P[f"bn{i}.weight"], P[f"bn{i}.bias"], x,
                      idx if l < t.l_e else lists[l - t.l_e])
        buffers.update(tref.running(state, i, e["mu"], e["var"], e["n"]))
        x = e["out"]
        outs.append(x)
    cat = torch.cat(outs, 1)
    i = t.E + 1
    y = P[f"conv{i}.0.weight"].reshape(t.emb, t.ccat) @ cat
    z, mu, var, n = tref.batch_norm(y, P[f"bn{i}.weight"], P[f"bn{i}.bias"], (0, 2))
    buffers.update(tref.running(state, i, mu, var, n))
    a = F.leaky_relu(z, 0.2)
    first = tref.first_argmax(a)
    pooled = torch.cat([torch.gather(a, 2, first[..., None])[..., 0], a.mean(-1)], 1)
    h = pooled
    for j in range(1, t.l_l):
        h = h @ P[f"linear{j}.weight"].T
        if j > 1:
            h = h + P[f"linear{j}.bias"]
        h, mu, var, n = tref.batch_norm(h, P[f"bn{i + j}.weight"], P[f"bn{i + j}.bias"], (0,))
        buffers.update(tref.running(state, i + j, mu, var, n))
        h = F.leaky_relu(h, head_slope)
    out = h @ P[f"linear{t.l_l}.weight"].T + P[f"linear{t.l_l}.bias"]
    loss = tref.trainer_loss(out, gt, weights)
    grads = torch.autograd.grad(loss, [P[key] for key in names])
    r = {"out": out.detach().numpy(), "loss": float(loss.detach()),
         "grads": {key: g.numpy() for key, g in zip(names, grads)},
         "buffers": {key: v.numpy() for key, v in buffers.items()}}
    if full:
        r.update(cat=cat.detach().numpy(), pooled=pooled.detach().numpy())
    return r
