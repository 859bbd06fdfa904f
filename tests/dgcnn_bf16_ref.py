"""The float64 restatements of DGCNN / BetterDGCNN in eval() (dgcnn_ref, better_dgcnn_ref) with an `operands` switch:
the checker of the device's bf16-operand mode (include/pcd.h, "bf16 operands").

With operands="bf16" the GEMM operands of every edge layer with Cin >= 32 and of the pooled convolution are rounded
where the device rounds them, and nothing else changes:
  activations  the layer's input, a float32 tensor in the device's memory          -> bf16
  weights      the packed float32 [W_a ; W_b - W_a] (the difference formed in double and rounded to float32, as the
               library packs it) and the pooled convolution's float32 weight       -> bf16
The products of the rounded operands are exact in float64 (8 + 8 significant bits) and summed in float64; the folded
batch norms (s, t), LeakyReLU, the max over the lists, the pooling and the head are dgcnn_ref's.  Edge layers with
Cin < 32 (the first, on the 17 feature rows) and the head are not rounded.  With operands="fp32" every function
returns dgcnn_ref's / better_dgcnn_ref's values exactly.

The per-layer functions (edge_layer, pooled_layer, head) take a layer's input and lists and return that layer's
output, so the device is checked stage by stage on its own intermediate tensors: a value that the device's float32
accumulation puts on the other side of a bf16 rounding boundary moves by 2^-8 relative in the next layer, which an
end-to-end comparison could not bound tightly.
"""
import numpy as np
import torch

import better_dgcnn_cases as bcases
import better_dgcnn_ref as bref
import dgcnn_cases as cases
import dgcnn_ref as ref

OPERANDS = ("fp32", "bf16")
MIN_CIN = 32                         # edge layers below it keep the float32 kernel
U = 2.0 ** -24


def check_operands(operands):
    if operands not in OPERANDS:
        raise ValueError(f'operands must be "fp32" or "bf16", got {operands!r}')
    return operands == "bf16"


def round_bf16(a):
    """a -> float64 array of the bf16 numbers nearest (ties to even) to a's float32 values; NaN and Inf are kept."""
    a32 = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    return torch.from_numpy(a32).to(torch.bfloat16).to(torch.float64).numpy()


class Net:
    """The shapes of a network: DGCNN (k, emb) or a BetterDGCNN configuration of better_dgcnn_cases."""

    def __init__(self, l_e, l_d, l_l, cin, cout, emb, k, head_slope):
        self.l_e, self.l_d, self.l_l, self.E = l_e, l_d, l_l, l_e + l_d
        self.cin, self.cout, self.emb, self.k, self.head_slope = tuple(cin), tuple(cout), emb, k, head_slope
        self.cat_off = tuple(int(v) for v in np.concatenate([[0], np.cumsum(self.cout)]))
        self.ccat = self.cat_off[-1]

    @classmethod
    def dgcnn(cls, k, emb):
        return cls(3, 3, 4, [c for c, _ in cases.EDGE], [c for _, c in cases.EDGE], emb, k, 0.2)

    @classmethod
    def better(cls, name):
        t = bcases.Table(name)
        return cls(t.l_e, t.l_d, t.l_l, t.cin, t.cout, t.emb, t.k, bcases.HEAD_SLOPE)

    def layer_input(self, l, inputs, cat):
        """The input of edge layer l (0-based): rows 0:17 of inputs [b, 20, 64] or its slice of cat [b, Ccat, 64]."""
        return np.asarray(inputs)[:, :17] if l == 0 else np.asarray(cat)[:, self.cat_off[l - 1]:self.cat_off[l]]

    def list_of(self, l, inputs, lists):
        """The neighbour lists of edge layer l: the index columns, or block l - l_e of lists [l_d, b, 64, k]."""
        return ref.index_lists(np.asarray(inputs, dtype=np.float64)) if l < self.l_e else \
            np.asarray(lists[l - self.l_e]).astype(np.int64)


def packed_edge(state, i):
    """conv i's weight as the library packs it: float32 (W_a, W_b - W_a), the difference formed in double."""
    w = np.asarray(state[f"conv{i}.0.weight"], dtype=np.float32)
    w = w.reshape(w.shape[0], -1)
    cin = w.shape[1] // 2
    wa = w[:, :cin]
    return wa, (w[:, cin:].astype(np.float64) - wa.astype(np.float64)).astype(np.float32)


def edge_operands(state, i, x, operands="fp32", min_cin=MIN_CIN):
    """(W_a, W_b - W_a, x) as float64, rounded to bf16 where the mode rounds them."""
    x = np.asarray(x, dtype=np.float64)
    if check_operands(operands) and x.shape[1] >= min_cin:
        wa, wd = packed_edge(state, i)
        return round_bf16(wa), round_bf16(wd), round_bf16(x)
    wa, wd = ref.split(state, i)
    return wa, wd, x


def edge_layer(state, i, x, nbr, operands="fp32", min_cin=MIN_CIN):
    """Edge convolution i (1-based) on x [b, Cin, 64] over nbr [b, 64, n] -> [b, Cout, 64] (dgcnn_ref.edge)."""
    x = np.asarray(x, dtype=np.float64)
    if not (check_operands(operands) and x.shape[1] >= min_cin):
        return ref.edge(state, i, x, nbr)
    wa, wd, xr = edge_operands(state, i, x, operands, min_cin)
    s, t = ref.fold(state, i)
    A, B = wa @ xr, wd @ xr
    b = np.arange(x.shape[0])[:, None, None, None]
    c = np.arange(A.shape[1])[None, :, None, None]
    v = s[None, :, None, None] * (A[b, c, nbr[:, None]] + B[:, :, :, None]) + t[None, :, None, None]
    return ref.lrelu(v.max(-1))


def edge_bound(state, i, x, nbr, operands="fp32", min_cin=MIN_CIN):
    """dgcnn_ref.edge_bound on the operands the mode multiplies: |s| (|W_a| |x_j| + |W_b - W_a| |x_i|) + |t|, maximised
    over the list.  [b, Cout, 64]."""
    wa, wd, xr = edge_operands(state, i, x, operands, min_cin)
    s, t = ref.fold(state, i)
    A, B = np.abs(wa) @ np.abs(xr), np.abs(wd) @ np.abs(xr)
    b = np.arange(xr.shape[0])[:, None, None, None]
    c = np.arange(A.shape[1])[None, :, None, None]
    m = np.abs(s)[None, :, None, None] * (A[b, c, nbr[:, None]] + B[:, :, :, None]) + np.abs(t)[None, :, None, None]
    return m.max(-1)


def pooled_operands(state, i, cat, operands="fp32"):
    w = np.asarray(state[f"conv{i}.0.weight"])
    w = w.reshape(w.shape[0], -1)
    cat = np.asarray(cat, dtype=np.float64)
    if check_operands(operands):
        return round_bf16(w), round_bf16(cat)
    return w.astype(np.float64), cat


def pooled_layer(state, i, cat, operands="fp32"):
    """The pooled convolution i = E + 1 on cat [b, Ccat, 64] -> pooled [b, 2 emb] (max, then mean over the nodes)."""
    w, x = pooled_operands(state, i, cat, operands)
    s, t = ref.fold(state, i)
    y = ref.lrelu(s[None, :, None] * (w @ x) + t[None, :, None])
    return np.concatenate([y.max(-1), y.mean(-1)], 1)


def pooled_bound(state, i, cat, operands="fp32"):
    """The edge layers' M for the pooled convolution: |s| |W| |x| + |t| maximised over the 64 nodes, [b, 2 emb] (the
    same for the max and the mean halves).  The device's error is at most (Ccat + 16 + 64) 2^-24 of it: the k chain
    and the affine as in an edge layer, and the mean's 63 float32 additions of terms bounded by M."""
    w, x = pooled_operands(state, i, cat, operands)
    s, t = ref.fold(state, i)
    m = (np.abs(s)[None, :, None] * (np.abs(w) @ np.abs(x)) + np.abs(t)[None, :, None]).max(-1)
    return np.concatenate([m, m], 1)


def head(net, state, pooled):
    """The linears on pooled [b, 2 emb] -> (out [b, out_ch], [h1, ..]): float64, never rounded."""
    h, hidden = np.asarray(pooled, dtype=np.float64), []
    n = net.E + 1
    for j in range(1, net.l_l):
        s, t = ref.fold(state, n + j, state.get(f"linear{j}.bias"))
        v = s * (h @ state[f"linear{j}.weight"].astype(np.float64).T) + t
        h = np.where(v > 0, v, net.head_slope * v)
        hidden.append(h)
    out = h @ state[f"linear{net.l_l}.weight"].astype(np.float64).T + state[f"linear{net.l_l}.bias"].astype(np.float64)
    return out, hidden


def _forward(net, state, inputs, operands, lists, full):
    inputs = np.asarray(inputs, dtype=np.float64)
    if len(inputs) > 16:                               # (dgcnn_ref's chunks: the same arrays, so the same sums)
        parts = [_forward(net, state, inputs[s:s + 16], operands, None if lists is None else np.asarray(lists)[:, s:s + 16],
                          True) for s in range(0, len(inputs), 16)]
        out = np.concatenate([p[0] for p in parts])
        if not full:
            return out
        return out, {key: np.concatenate([p[1][key] for p in parts], 1 if key == "lists" else 0) for key in parts[0][1]}
    x = inputs[:, :17]
    idx = ref.index_lists(inputs) if net.l_e else None
    outs, used = [], []
    for l in range(net.E):
        if l < net.l_e:
            nbr = idx
        else:
            # the search runs on the float32 activations, in either mode
            nbr = ref.knn(x, net.k) if lists is None else np.asarray(lists[l - net.l_e]).astype(np.int64)
            used.append(nbr)
        x = edge_layer(state, l + 1, x, nbr, operands)
        outs.append(x)
    cat = np.concatenate(outs, 1)
    pooled = pooled_layer(state, net.E + 1, cat, operands)
    out, hidden = head(net, state, pooled)
    if not full:
        return out
    r = {"cat": cat, "lists": np.stack(used) if used else np.zeros((0, len(inputs), 64, net.k), np.int64),
         "pooled": pooled}
    r.update({f"h{j}": v for j, v in enumerate(hidden, start=1)})
    return out, r


def forward(state, inputs, k, lists=None, full=False, operands="fp32"):
    """dgcnn_ref.forward with the operands switch (emb is read off conv7's weight)."""
    check_operands(operands)
    return _forward(Net.dgcnn(k, int(np.asarray(state["conv7.0.weight"]).shape[0])), state, inputs, operands, lists, full)


def better_forward(name, state, inputs, lists=None, full=False, operands="fp32"):
    """better_dgcnn_ref.forward with the operands switch."""
    check_operands(operands)
    return _forward(Net.better(name), state, inputs, operands, lists, full)


# ------------------------------------------------------------------------- what the mode costs, on the goldens
def angles_deg(a, b):
    """Angle between the normalised rows of a and b [n, 3], in degrees."""
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    return np.degrees(np.arccos(np.clip((a * b).sum(1), -1.0, 1.0)))


_golden_numbers = {}


def golden_numbers(load, name):
    """The bf16 restatement on a configuration of dgcnn_cases.CONFIGS (the float32 inputs the device gets, nothing
    injected) against the reference's float64 outputs of the golden: {"dev" [n] max |out - out64| per patch,
    "angle" [n] degrees between the normalised outputs, "max_dev", "med_dev", "max_angle", "med_angle", "out"}.
    load(name) -> npz of tests/golden.  Computed once per configuration."""
    if name not in _golden_numbers:
        k, emb, fx, _ = cases.CONFIGS[name]
        g = load(f"dgcnn_{name}")
        x = cases.fixture_inputs(load, fx)[0][g["rows"]].astype(np.float32)
        out = forward(cases.make_state(cases.SEED, k, emb), x, k, operands="bf16")
        dev = np.abs(out - g["out64"]).max(-1)
        ang = angles_deg(out, g["out64"])
        _golden_numbers[name] = {"out": out, "dev": dev, "angle": ang, "max_dev": float(dev.max()),
                                 "med_dev": float(np.median(dev)), "max_angle": float(ang.max()),
                                 "med_angle": float(np.median(ang))}
    return _golden_numbers[name]
