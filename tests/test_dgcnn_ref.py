"""The float64 restatement of the DGCNN forward (tests/dgcnn_ref.py) against the reference's own float64 run
(tests/golden/dgcnn_*.npz, made by tests/golden/make_dgcnn_golden.py) and against known answers.  No GPU."""
import numpy as np
import pytest

import dgcnn_cases as cases
import dgcnn_ref as ref


def _close(a, b, what):
    tol = 1e-12 * max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


@pytest.fixture(scope="module")
def ellipsoid(golden):
    return cases.fixture_inputs(golden, "ellipsoid")


@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_restatement_equals_reference_float64(golden, name):
    k, emb, fixture, _ = cases.CONFIGS[name]
    g = golden(f"dgcnn_{name}")
    inputs, size = cases.fixture_inputs(golden, fixture)
    assert np.array_equal(g["rows"], cases.config_rows(name, size))
    x = inputs[g["rows"]]
    state = cases.make_state(cases.SEED, k, emb)
    for lists in (g["lists64"], None):
        what = f"{name} ({'lists injected' if lists is not None else 'own lists'})"
        out, full = ref.forward(state, x, k, lists=lists, full=True)
        _close(out, g["out64"], what + " outputs")                    # every patch
        for slot, r in enumerate(g["act_rows"]):
            _close(full["cat"][r], golden(f"dgcnn_{name}_act{slot}")["cat"], what + f" concatenation of row {r}")
            for key in ("pooled", "h1", "h2", "h3"):
                _close(full[key][r], g[key][slot], what + f" {key} of row {r}")
        if lists is None:                                             # the same neighbours, by distance
            for layer, (lo, hi) in enumerate(ref.DYN_INPUT):
                assert not ref.lists_differ(full["cat"][:, lo:hi], g["lists64"][layer], full["lists"][layer]).any()


def test_k1_sees_only_itself(ellipsoid):
    inputs, size = ellipsoid
    rows = np.concatenate([np.nonzero(size < 64)[0][:2], np.nonzero(size >= 64)[0][:2]])
    x = inputs[rows]
    state = cases.make_state(cases.SEED, 1, 128)
    own = np.broadcast_to(np.arange(64)[None, None, :, None], (3, len(x), 64, 1))
    out, full = ref.forward(state, x, 1, full=True)
    # (among a padded patch's identical rows the search may name another of them: the same features, and the same
    # output up to the rounding of a matrix product whose equal columns need not be summed in one order)
    assert np.array_equal(full["lists"][:, 2:], own[:, 2:])
    want = ref.forward(state, x, 1, lists=own)
    assert np.allclose(out, want, rtol=1e-13, atol=1e-13)


def test_negated_gamma_turns_max_into_min(ellipsoid):
    x = ellipsoid[0][:4]
    state = cases.make_state(cases.SEED, 8, 128)
    nbr = ref.index_lists(x)
    A, B, s, t = ref.edge_terms(state, 1, x[:, :17])
    Aj = np.stack([A[p][:, nbr[p]] for p in range(len(x))])           # [b, out, 64, 3]: A of each row's neighbours
    v = s[None, :, None, None] * (Aj + B[:, :, :, None]) + t[None, :, None, None]
    flipped = dict(state)
    flipped["bn1.weight"] = -state["bn1.weight"]                     # s -> -s
    flipped["bn1.bias"] = -state["bn1.bias"]                         # and t = beta - s mean -> -t
    got = ref.edge(flipped, 1, x[:, :17], nbr)
    assert np.allclose(got, ref.lrelu(-v.min(-1)), rtol=1e-13, atol=1e-13)
    assert (state["bn1.weight"] < 0).any()                           # (the fixtures hold negative gammas as they are)
    assert np.allclose(ref.edge(state, 1, x[:, :17], nbr), ref.lrelu(v.max(-1)), rtol=1e-13, atol=1e-13)


def test_index_columns_63_see_row_63(ellipsoid):
    x = ellipsoid[0][:4].copy()
    x[:, 17:20] = 63.0
    state = cases.make_state(cases.SEED, 8, 128)
    A, B, s, t = ref.edge_terms(state, 1, x[:, :17])
    want = ref.lrelu(s[None, :, None] * (A[:, :, 63:64] + B) + t[None, :, None])
    got = ref.edge(state, 1, x[:, :17], ref.index_lists(x))
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13)


def test_make_state_fits_the_layer_table():
    st = cases.make_state(cases.SEED, 8, 128)
    assert st["conv1.0.weight"].shape == (64, 34, 1, 1) and st["conv7.0.weight"].shape == (128, 1024, 1)
    assert st["linear1.weight"].shape == (512, 256) and "linear1.bias" not in st and st["linear4.bias"].shape == (3,)
    assert st["conv3.1.weight"] is st["bn3.weight"]
    neg = np.mean([(st[f"bn{i}.weight"] < 0).mean() for i in range(1, 11)])
    assert 0.03 < neg < 0.2
    assert all(v.dtype == np.float32 for key, v in st.items() if not key.endswith("num_batches_tracked"))
