"""The float64 restatement of BetterDGCNN (tests/better_dgcnn_ref.py) against the reference's own float64 runs in
eval() and train() (tests/golden/better_dgcnn_*.npz, made by tests/golden/make_better_dgcnn_golden.py).  No GPU."""
import numpy as np
import pytest

import better_dgcnn_cases as cases
import better_dgcnn_ref as bref
import dgcnn_train_ref as tref

REL = 1e-10


def _close(a, b, what):
    tol = 1e-12 * max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def _cat(golden, name, g):
    if "cat" in g.files:
        return g["cat"]
    return np.stack([golden(f"better_dgcnn_{name}_act{slot}")["cat"] for slot in (0, 1)])


@pytest.mark.parametrize("name", list(cases.CONFIGS))
@pytest.mark.parametrize("own_lists", [False, True])
def test_forward_equals_reference_float64(golden, name, own_lists):
    g = golden(f"better_dgcnn_{name}")
    t = cases.Table(name)
    inputs, size = cases.fixture_inputs(golden)
    assert np.array_equal(g["rows"], cases.config_rows(size))
    assert (size[g["rows"]] < 64).sum() == 8 and len(g["rows"]) == 16
    assert g["lists64"].shape == (t.l_d, 16, 64, t.k)
    x = inputs[g["rows"]]
    out, full = bref.forward(name, cases.make_state(name), x, None if own_lists else g["lists64"], full=True)
    _close(out, g["out64"], f"{name}: outputs")
    at = g["act_rows"]
    _close(full["cat"][at], _cat(golden, name, g), f"{name}: concatenation")
    for key in ["pooled"] + [f"h{j}" for j in range(1, t.l_l)]:
        _close(full[key][at], g[key], f"{name}: {key}")
    if own_lists:
        assert not bref.lists_differ(name, x, full["cat"], g["lists64"], full["lists"]).any()


def test_golden_deviations_are_sane(golden):
    """Every configuration has a non-zero float32 allowance of the size float32 rounding gives."""
    for name in cases.CONFIGS:
        g = golden(f"better_dgcnn_{name}")
        assert 1e-8 < float(g["dev32_stable"]) < 1e-5, name
        assert float(g["dev32_stable"]) <= float(g["dev32_all"]) < 1e-3, name
        dev = np.abs(g["out32"].astype(np.float64) - g["out64"]).max(-1)
        assert (dev[~g["differs32"]] <= float(g["dev32_stable"])).all(), name


def test_head_slope_is_the_default_one(golden):
    """At slope 0.2 in the head the restatement does NOT give the reference's output: line 291 passes no slope."""
    g = golden("better_dgcnn_default")
    inputs, _ = cases.fixture_inputs(golden)
    out = bref.forward("default", cases.make_state("default"), inputs[g["rows"]], g["lists64"], head_slope=0.2)
    assert np.abs(out - g["out64"]).max() > 1e-3


def test_state_dict_keys_of_the_drawn_states(golden):
    for name in cases.CONFIGS:
        g = golden(f"better_dgcnn_{name}")
        state = cases.make_state(name)
        assert sorted(state) == sorted(str(k) for k in g["sd_keys"]), name
        for key, shape in zip(g["sd_keys"], g["sd_shapes"]):
            want = tuple(int(s) for s in str(shape).split(",") if s)
            assert tuple(np.shape(state[str(key)])) == want, (name, key)


def _train_case(golden, name):
    g = golden(f"better_dgcnn_train_{name}")
    inputs, size = cases.fixture_inputs(golden)
    assert np.array_equal(g["rows"], cases.train_rows(name, size))
    assert np.array_equal(g["gt"], tref.unit_vectors("better_" + name, len(g["rows"])))
    assert ((size[g["rows"]] < 64).sum(), (size[g["rows"]] >= 64).sum()) == cases.TRAIN[name]
    return g, cases.make_state(name), inputs[g["rows"]]


@pytest.mark.parametrize("name", list(cases.TRAIN))
def test_step_equals_reference_float64(golden, name):
    g, state, x = _train_case(golden, name)
    r = bref.step(name, state, x, g["gt"], g["lists64"])
    assert np.abs(r["out"] - g["out64"]).max() <= REL * np.abs(g["out64"]).max()
    assert abs(r["loss"] - float(g["loss64"])) <= REL * abs(float(g["loss64"]))
    assert set(r["buffers"]) == set(bref.buffer_names(name))
    for key in bref.buffer_names(name):
        want = g[f"buf/{key}"]
        assert np.abs(r["buffers"][key] - want).max() <= REL * np.abs(want).max(), key
    assert set(r["grads"]) == set(bref.param_names(name))
    for key in bref.param_names(name):                                # no tensor is left out
        scale = float(g[f"gscale/{key}"])
        for label, got, want, weight in tref.golden_views(g, key, r["grads"][key]):
            err = float(np.abs(got - want).max())
            assert err <= REL * scale * weight, f"{name} {key} {label}: {err:.3e} > {REL * scale * weight:.3e}"


def test_step_with_own_lists(golden):
    """The training restatement on lists the forward restatement finds itself (odd: the search on the input rows)."""
    g, state, x = _train_case(golden, "odd")
    t = cases.Table("odd")
    lists = []
    cur = x[:, :17]
    import dgcnn_ref as ref
    import torch
    for d in range(t.l_d):                             # each layer's search on the train-mode activations before it
        nbr = ref.knn(cur, t.k)
        lists.append(nbr)
        i = d + 1
        e = tref.edge(torch.as_tensor(state[f"conv{i}.0.weight"].astype(np.float64)),
                      torch.as_tensor(state[f"bn{i}.weight"].astype(np.float64)),
                      torch.as_tensor(state[f"bn{i}.bias"].astype(np.float64)), torch.as_tensor(cur),
                      torch.as_tensor(nbr))
        cur = e["out"].numpy()
    lists = np.stack(lists)
    r = bref.step("odd", state, x, g["gt"], lists, full=True)
    assert not bref.lists_differ("odd", x, r["cat"], g["lists64"], lists).any()
    assert np.abs(r["out"] - g["out64"]).max() <= REL * np.abs(g["out64"]).max()
