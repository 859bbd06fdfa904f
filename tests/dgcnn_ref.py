"""A float64 numpy restatement of DGCNN.forward in eval() (GCNModel.py:170-215), the checker of the device forward.

It computes what the device computes, in the device's arrangement -- the edge weight split into W_a (on x_j) and
W_b - W_a (on x_i), the batch norm folded into (s, t) -- so that the same per-term magnitudes bound the device's
rounding.  Neighbour lists of the three dynamic layers may be injected (`lists`), which takes the one discontinuous
step out of a comparison.
"""
import numpy as np

from dgcnn_cases import EDGE, HEAD


def lrelu(v):
    return np.where(v > 0, v, 0.2 * v)


def fold(state, i, bias=None, eps=1e-5):
    """Batch norm i (and a preceding linear bias) as v -> s v + t."""
    g, be = state[f"bn{i}.weight"].astype(np.float64), state[f"bn{i}.bias"].astype(np.float64)
    mu, var = state[f"bn{i}.running_mean"].astype(np.float64), state[f"bn{i}.running_var"].astype(np.float64)
    s = g / np.sqrt(var + eps)
    shift = (0.0 if bias is None else bias.astype(np.float64)) - mu
    return s, be + s * shift


def split(state, i):
    """conv i's weight as (W_a, W_b - W_a), float64 [out, in] each."""
    w = state[f"conv{i}.0.weight"].astype(np.float64)
    w = w.reshape(w.shape[0], -1)
    cin = w.shape[1] // 2
    return w[:, :cin], w[:, cin:] - w[:, :cin]


def sqdist(x):
    """x [b, C, 64] -> D [b, 64, 64], D(i, j) = |x_i - x_j|^2."""
    d = x[:, :, :, None] - x[:, :, None, :]
    return (d * d).sum(1)


def knn(x, k):
    """[b, 64, k]: the k nearest rows, ascending (distance, index) -- the self entry included."""
    return np.argsort(sqdist(x), axis=-1, kind="stable")[:, :, :k]


def edge_terms(state, i, x):
    """(A [b, out, 64], B [b, out, 64], s, t) of edge layer i on x [b, in, 64]."""
    wa, wd = split(state, i)
    s, t = fold(state, i)
    return wa @ x, wd @ x, s, t


def edge(state, i, x, nbr):
    """Edge convolution i on x [b, in, 64] over nbr [b, 64, n]: [b, out, 64]."""
    A, B, s, t = edge_terms(state, i, x)
    b = np.arange(x.shape[0])[:, None, None, None]
    c = np.arange(A.shape[1])[None, :, None, None]
    v = s[None, :, None, None] * (A[b, c, nbr[:, None]] + B[:, :, :, None]) + t[None, :, None, None]
    return lrelu(v.max(-1))


def edge_bound(state, i, x, nbr):
    """M of the fma-chain bound per output: |s| (|W_a| |x_j| + |W_b - W_a| |x_i|) + |t|, maximised over the list."""
    wa, wd = split(state, i)
    s, t = fold(state, i)
    A, B = np.abs(wa) @ np.abs(x), np.abs(wd) @ np.abs(x)
    b = np.arange(x.shape[0])[:, None, None, None]
    c = np.arange(A.shape[1])[None, :, None, None]
    m = np.abs(s)[None, :, None, None] * (A[b, c, nbr[:, None]] + B[:, :, :, None]) + np.abs(t)[None, :, None, None]
    return m.max(-1)


def index_lists(inputs):
    """The three index columns as lists [b, 64, 3], truncated as .long() does."""
    return np.transpose(np.trunc(inputs[:, 17:20]).astype(np.int64), (0, 2, 1))


def forward(state, inputs, k, lists=None, full=False):
    """inputs [b, 20, 64] -> out [b, out_ch] float64.  lists: None, or [3, b, 64, k] for the dynamic layers.
    full: also {"cat" [b, 1024, 64], "lists" [3, b, 64, k], "pooled" [b, 2 emb], "h1", "h2", "h3" [b, .]}."""
    inputs = np.asarray(inputs, dtype=np.float64)
    if len(inputs) > 16:                               # (the [b, C, 64, 64] differences of knn stay small)
        parts = [forward(state, inputs[s:s + 16], k, None if lists is None else np.asarray(lists)[:, s:s + 16], full)
                 for s in range(0, len(inputs), 16)]
        if not full:
            return np.concatenate(parts)
        return np.concatenate([p[0] for p in parts]), \
            {key: np.concatenate([p[1][key] for p in parts], 1 if key == "lists" else 0) for key in parts[0][1]}
    x = inputs[:, :17]
    idx = index_lists(inputs)
    outs, used = [], []
    for i in range(1, 7):
        if i <= 3:
            nbr = idx
        else:
            nbr = knn(x, k) if lists is None else np.asarray(lists[i - 4]).astype(np.int64)
            used.append(nbr)
        x = edge(state, i, x, nbr)
        outs.append(x)
    cat = np.concatenate(outs, 1)
    w7 = state["conv7.0.weight"].astype(np.float64).reshape(-1, 1024)
    s, t = fold(state, 7)
    y = lrelu(s[None, :, None] * (w7 @ cat) + t[None, :, None])
    pooled = np.concatenate([y.max(-1), y.mean(-1)], 1)
    h, hidden = pooled, []
    for i in range(1, 4):
        s, t = fold(state, 7 + i, state.get(f"linear{i}.bias"))
        h = lrelu(s * (h @ state[f"linear{i}.weight"].astype(np.float64).T) + t)
        hidden.append(h)
    out = h @ state["linear4.weight"].astype(np.float64).T + state["linear4.bias"].astype(np.float64)
    if not full:
        return out
    return out, {"cat": cat, "lists": np.stack(used), "pooled": pooled, "h1": hidden[0], "h2": hidden[1],
                 "h3": hidden[2]}


def lists_differ(x, a, b):
    """Rows whose two neighbour sets differ BY DISTANCE on the layer input x [b, C, 64]: [b, 64] bool.  Index for
    index they may differ freely where distances tie exactly (identical padding rows)."""
    D = sqdist(np.asarray(x, dtype=np.float64))
    da = np.sort(np.take_along_axis(D, np.asarray(a).astype(np.int64), -1), -1)
    db = np.sort(np.take_along_axis(D, np.asarray(b).astype(np.int64), -1), -1)
    return (da != db).any(-1)


# the concatenation's slice holding the INPUT of dynamic layer 4, 5, 6
DYN_INPUT = ((128, 256), (256, 512), (512, 768))
