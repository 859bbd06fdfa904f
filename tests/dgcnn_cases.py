"""Weights and configurations of the DGCNN tests (numpy only: the same numbers under every torch version).

Weights are never committed (conv7 and linear1 are 4 MB each at emb = 1024): `make_state(seed, k, emb_dims)` draws
them, under the reference module's state-dict keys.  The goldens (tests/golden/make_dgcnn_golden.py) were made with
exactly these states.
"""
import numpy as np

EDGE = ((17, 64), (64, 64), (64, 128), (128, 256), (256, 256), (256, 256))   # (in, out) of conv1-6
HEAD = (512, 256, 64)
SEED = 11

# name -> (k, emb_dims, fixture, patches): patches None = all of the fixture's stored inputs, else that many, half of
# them padded below 64 rows where the fixture has padded ones
CONFIGS = {
    "k8_emb1024_ellipsoid": (8, 1024, "ellipsoid", 16),
    "k8_emb128_ellipsoid": (8, 128, "ellipsoid", None),
    "k8_emb128_shells": (8, 128, "shells", None),
    "k20_emb128_ellipsoid": (20, 128, "ellipsoid", 16),
    "k1_emb128_ellipsoid": (1, 128, "ellipsoid", 16),
}


def make_state(seed, k, emb_dims, output_channels=3):
    """{state-dict key: float32 array}.  Convolution / linear weights U(-1, 1) * sqrt(3 / fan_in) (unit gain); batch
    norm running mean N(0, 0.1), running var U(0.5, 1.5), gamma U(0.5, 1.5) with about one in ten negated, beta
    N(0, 0.2); linear biases N(0, 0.2).  The draw depends on (seed, k, emb_dims)."""
    rng = np.random.default_rng([int(seed), int(k), int(emb_dims)])
    st = {}

    def weight(name, shape, fan_in):
        st[name] = (rng.uniform(-1.0, 1.0, shape) * np.sqrt(3.0 / fan_in)).astype(np.float32)

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

    for i, (cin, cout) in enumerate(EDGE, start=1):
        weight(f"conv{i}.0.weight", (cout, 2 * cin, 1, 1), 2 * cin)
        bn(i, cout, f"conv{i}.1")
    weight("conv7.0.weight", (emb_dims, 1024, 1), 1024)
    bn(7, emb_dims, "conv7.1")
    width = 2 * emb_dims
    for i, out in enumerate(HEAD, start=1):
        weight(f"linear{i}.weight", (out, width), width)
        if i > 1:
            st[f"linear{i}.bias"] = rng.normal(0.0, 0.2, out).astype(np.float32)
        bn(7 + i, out, None)
        width = out
    weight("linear4.weight", (output_channels, width), width)
    st["linear4.bias"] = rng.normal(0.0, 0.2, output_channels).astype(np.float32)
    return st


def fixture_inputs(load, fixture):
    """(inputs [n, 20, 64] float64 channels first, patch_size [n]) of a committed patch fixture; load(name) -> npz."""
    g = load(f"patch_{fixture}")
    size = np.diff(g["off"])[g["input_faces"]]
    if fixture == "shells":                            # the first of its three input files: 147 patches
        x = load("patch_shells_inputs_0")["inputs"]
        size = size[:len(x)]
    else:
        x = g["inputs"]
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1))).astype(np.float64), size


def config_rows(name, size):
    """The fixture rows a configuration runs: all, or `patches` of them, the first half padded ones where there are."""
    patches = CONFIGS[name][3]
    if patches is None:
        return np.arange(len(size))
    padded, full = np.nonzero(size < 64)[0], np.nonzero(size >= 64)[0]
    half = min(patches // 2, len(padded))
    return np.concatenate([padded[:half], full[:patches - half]])
