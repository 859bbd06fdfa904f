"""The float64 restatement of the DGCNN training step (tests/dgcnn_train_ref.py) against the reference's own float64
run in train() (tests/golden/dgcnn_train_*.npz, made by tests/golden/make_dgcnn_train_golden.py) and against central
finite differences of its own loss.  No GPU."""
import numpy as np
import pytest

import dgcnn_cases as cases
import dgcnn_train_ref as tref

REL = 1e-10


def _case(golden, name):
    k, emb, fixture = tref.CONFIGS[name][:3]
    g = golden(f"dgcnn_train_{name}")
    inputs, size = cases.fixture_inputs(golden, fixture)
    assert np.array_equal(g["rows"], tref.config_rows(name, size))
    assert np.array_equal(g["gt"], tref.unit_vectors(name, len(g["rows"])))
    return g, cases.make_state(cases.SEED, k, emb), inputs[g["rows"]]


@pytest.mark.parametrize("name", list(tref.CONFIGS))
def test_restatement_equals_reference_float64(golden, name):
    g, state, x = _case(golden, name)
    r = tref.step(state, x, g["gt"], g["lists64"])
    assert np.abs(r["out"] - g["out64"]).max() <= REL * np.abs(g["out64"]).max()
    assert abs(r["loss"] - float(g["loss64"])) <= REL * abs(float(g["loss64"]))
    for key in tref.buffer_names():
        want = g[f"buf/{key}"]
        assert np.abs(r["buffers"][key] - want).max() <= REL * np.abs(want).max(), key
    assert set(r["grads"]) == set(tref.param_names())
    for key in tref.param_names():                                    # no tensor is left out
        scale = float(g[f"gscale/{key}"])
        for label, got, want, weight in tref.golden_views(g, key, r["grads"][key]):
            err = float(np.abs(got - want).max())
            assert err <= REL * scale * weight, f"{name} {key} {label}: {err:.3e} > {REL * scale * weight:.3e}"


def test_golden_configurations(golden):
    size = cases.fixture_inputs(golden, "ellipsoid")[1]
    g = golden("dgcnn_train_k8_b5_ellipsoid")
    assert (size[g["rows"]] < 64).sum() == 2 and (size[g["rows"]] >= 64).sum() == 3
    assert len(golden("dgcnn_train_k1_b2_ellipsoid")["rows"]) == 2 and len(golden("dgcnn_train_k20_b6_shells")["rows"]) == 6
    # the reference's float32 run, searching on its own, agrees with lists64 by distance on at least two of the three
    assert sum(not golden(f"dgcnn_train_{name}")["differs32"].any() for name in tref.CONFIGS) >= 2


@pytest.mark.parametrize("key", ["conv1.0.weight", "conv5.0.weight", "bn4.weight"])
def test_autograd_gradient_against_central_differences(golden, key):
    """Step 1e-6 on the entry with the largest gradient, the lists held fixed: agreement to 1e-6 relative."""
    g, state, x = _case(golden, "k8_b5_ellipsoid")
    state = {k_: np.asarray(v, dtype=np.float64) if k_ in tref.param_names() else v for k_, v in state.items()}
    grad = tref.step(state, x, g["gt"], g["lists64"])["grads"][key]
    at = np.unravel_index(np.abs(grad).argmax(), grad.shape)
    h = 1e-6
    loss = []
    for sign in (1.0, -1.0):
        moved = dict(state)
        moved[key] = state[key].copy()
        moved[key][at] += sign * h
        loss.append(tref.loss_only(moved, x, g["gt"], g["lists64"]))
    fd = (loss[0] - loss[1]) / (2 * h)
    assert abs(fd - grad[at]) <= 1e-6 * abs(grad[at]), f"{key}{at}: central difference {fd:.9e}, autograd {grad[at]:.9e}"
