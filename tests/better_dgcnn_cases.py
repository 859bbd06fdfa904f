"""Configurations and weights of the BetterDGCNN tests (numpy only: the same numbers under every torch version).

Weights are never committed: `make_state(name)` draws them as dgcnn_cases.make_state does, under the reference module's
state-dict keys.  The goldens (tests/golden/make_better_dgcnn_golden.py) were made with exactly these states.
"""
import numpy as np

import dgcnn_cases

SEED = dgcnn_cases.SEED
FIXTURE, PATCHES = "ellipsoid", 16

# name -> (l_e, l_d, l_l, channel_sizes, k)
CONFIGS = {
    # the fixed network's shapes; only the head slope differs
    "default": (3, 3, 4, (64, 64, 128, 256, 256, 256, 128, 512, 256, 64), 8),
    # M = 64 and 96; Ccat = 80, a K tail in the pooled convolution; a one-hidden-layer head
    "narrow": (1, 1, 2, (32, 48, 96, 40), 4),
    # l_e = 0, the search on the 17 input rows; M = 66 and 130 across a tile edge; K = 33 and 65; Ccat = 98
    "odd": (0, 2, 3, (33, 65, 130, 64, 20), 5),
    # l_d = 0: no search
    "static": (2, 0, 2, (16, 24, 64, 32), 8),
    # more than six edge layers, a four-deep head
    "deep": (4, 4, 5, (16, 16, 32, 32, 32, 64, 64, 64, 128, 64, 32, 16, 8), 6),
}

# training goldens: name -> (padded patches, full patches).  9 patches cross a chunk of the batch statistics (8) and
# give three runs of the weight gradient's split reduction
TRAIN = {"narrow": (4, 5), "odd": (2, 3), "static": (1, 2), "default": (1, 1)}

HEAD_SLOPE = 0.01                    # F.leaky_relu's default (GCNModel.py:291 of the reference)


class Table:
    """The shapes a configuration implies."""

    def __init__(self, name):
        self.name = name
        self.l_e, self.l_d, self.l_l, self.sizes, self.k = CONFIGS[name]
        E = self.E = self.l_e + self.l_d
        self.cin = (17,) + tuple(self.sizes[:E - 1])
        self.cout = tuple(self.sizes[:E])
        self.cat_off = tuple(int(v) for v in np.concatenate([[0], np.cumsum(self.cout)]))
        self.ccat = self.cat_off[-1]
        self.emb = self.sizes[E]
        self.head = tuple(self.sizes[E + 1:])

    def dyn_input(self, d):
        """Where dynamic layer d (0-based) reads: None for rows 0:17 of the input, else the (lo, hi) slice of the
        concatenation."""
        l = self.l_e + d
        return None if l == 0 else (self.cat_off[l - 1], self.cat_off[l])


def make_state(name, output_channels=3):
    """{state-dict key: float32 array}, the distributions of dgcnn_cases.make_state.  The draw depends on the name."""
    t = Table(name)
    rng = np.random.default_rng([SEED, sum(map(ord, name)), len(t.sizes)])
    st = {}

    def weight(key, shape, fan_in):
        st[key] = (rng.uniform(-1.0, 1.0, shape) * np.sqrt(3.0 / fan_in)).astype(np.float32)

    def bn(i, n, alias):
        vals = {"running_mean": rng.normal(0.0, 0.1, n), "running_var": rng.uniform(0.5, 1.5, n),
                "weight": rng.uniform(0.5, 1.5, n) * np.where(rng.random(n) < 0.1, -1.0, 1.0),
                "bias": rng.normal(0.0, 0.2, n)}
        for key, v in vals.items():
            st[f"bn{i}.{key}"] = v.astype(np.float32)
        st[f"bn{i}.num_batches_tracked"] = np.int64(0)
        if alias:
            for key in list(vals) + ["num_batches_tracked"]:
                st[f"{alias}.{key}"] = st[f"bn{i}.{key}"]

    for i, (cin, cout) in enumerate(zip(t.cin, t.cout), start=1):
        weight(f"conv{i}.0.weight", (cout, 2 * cin, 1, 1), 2 * cin)
        bn(i, cout, f"conv{i}.1")
    weight(f"conv{t.E + 1}.0.weight", (t.emb, t.ccat, 1), t.ccat)
    bn(t.E + 1, t.emb, f"conv{t.E + 1}.1")
    width = 2 * t.emb
    for j, out in enumerate(t.head, start=1):
        weight(f"linear{j}.weight", (out, width), width)
        if j > 1:
            st[f"linear{j}.bias"] = rng.normal(0.0, 0.2, out).astype(np.float32)
        bn(t.E + 1 + j, out, None)
        width = out
    weight(f"linear{t.l_l}.weight", (output_channels, width), width)
    st[f"linear{t.l_l}.bias"] = rng.normal(0.0, 0.2, output_channels).astype(np.float32)
    return st


def fixture_inputs(load):
    return dgcnn_cases.fixture_inputs(load, FIXTURE)


def config_rows(size, patches=PATCHES):
    """The fixture rows every configuration runs: `patches` of them, the first half padded ones."""
    padded, full = np.nonzero(size < 64)[0], np.nonzero(size >= 64)[0]
    half = min(patches // 2, len(padded))
    return np.concatenate([padded[:half], full[:patches - half]])


def train_rows(name, size):
    n_pad, n_full = TRAIN[name]
    padded, full = np.nonzero(size < 64)[0], np.nonzero(size >= 64)[0]
    n_pad = min(n_pad, len(padded))
    return np.concatenate([padded[:n_pad], full[:sum(TRAIN[name]) - n_pad]])
