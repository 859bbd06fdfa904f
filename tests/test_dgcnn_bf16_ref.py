"""tests/dgcnn_bf16_ref.py, the yardstick of the bf16-operand mode, checked on the CPU: with operands="fp32" it is the
float64 restatements it is built from, its rounding is round-to-nearest-even on the bits, and what the mode costs on
the goldens is computed (and reported) by the function the device tests take their allowances from.
"""
import numpy as np
import pytest

import better_dgcnn_cases as bcases
import better_dgcnn_ref as bref
import dgcnn_bf16_ref as bf
import dgcnn_cases as cases
import dgcnn_ref as ref
from conftest import report


def _rne_on_the_bits(a32):
    """float32 -> the nearest bf16 (ties to the even mantissa) as float32, by integer arithmetic on the bit pattern.
    NaN is kept a NaN (the carry could otherwise turn its mantissa to zero); Inf has no low bits and stays."""
    bits = a32.view(np.uint32).astype(np.uint64)
    low, keep = bits & 0xFFFF, bits >> 16
    up = (low > 0x8000) | ((low == 0x8000) & ((keep & 1) == 1))
    out = ((keep + up.astype(np.uint64)) << 16).astype(np.uint32)
    nan = np.isnan(a32)
    out[nan] = (bits[nan].astype(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x00400000)
    return out.view(np.float32)


def test_rounding_helper_is_nearest_even():
    rng = np.random.default_rng(5)
    smallest_normal = np.float32(2.0 ** -126)
    rand = (rng.normal(0.0, 1.0, 20000) * 10.0 ** rng.integers(-20, 20, 20000)).astype(np.float32)
    pattern = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    # exact ties: a bf16 number plus half its last place, on even and odd mantissas, both signs
    base = (rng.integers(0x0080, 0x7F7F, 4000, dtype=np.uint64).astype(np.uint32) << np.uint32(16))
    ties = np.concatenate([base | np.uint32(0x8000), base | np.uint32(0x80008000)]).view(np.float32)
    near = np.concatenate([base | np.uint32(0x7FFF), base | np.uint32(0x8001)]).view(np.float32)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 3.3895314e38, -3.3895314e38,
                        3.4028235e38], np.float32)               # bf16's largest, and float32's, which rounds to Inf
    a = np.concatenate([rand, pattern, ties, near, special])
    a = a[np.isnan(a) | (np.abs(a) >= smallest_normal) | (a == 0)]      # subnormals are left out
    got = bf.round_bf16(a)
    want = _rne_on_the_bits(a).astype(np.float64)
    assert got.dtype == np.float64 and got.shape == a.shape
    assert np.array_equal(np.isnan(got), np.isnan(a))
    ok = ~np.isnan(a)
    assert np.array_equal(got[ok], want[ok])
    assert np.array_equal(np.signbit(got[ok]), np.signbit(a[ok]))           # -0 stays -0
    assert np.isposinf(bf.round_bf16(np.float32(np.inf))) and np.isneginf(bf.round_bf16(np.float32(-np.inf)))
    # ties go to the even neighbour: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert bf.round_bf16(np.float32(1 + 2.0 ** -8)) == 1.0 and bf.round_bf16(np.float32(1 + 3 * 2.0 ** -8)) == 1 + 2.0 ** -6
    # a float64 argument is taken at its float32 value first
    assert bf.round_bf16(np.float64(1 + 2.0 ** -8 + 2.0 ** -40)) == 1.0


def test_fp32_is_the_restatement_exactly(golden):
    x, size = cases.fixture_inputs(golden, "ellipsoid")
    rows = cases.config_rows("k8_emb1024_ellipsoid", size)[:4]
    for k, emb in ((8, 128), (1, 128)):
        state = cases.make_state(cases.SEED, k, emb)
        want, wfull = ref.forward(state, x[rows], k, full=True)
        got, gfull = bf.forward(state, x[rows], k, full=True, operands="fp32")
        assert np.array_equal(got, want)
        assert set(gfull) == set(wfull) and all(np.array_equal(gfull[key], wfull[key]) for key in wfull)
        assert np.array_equal(bf.forward(state, x[rows], k, lists=wfull["lists"]), want)
    x17 = x[:17]                                                                # more than one chunk of 16
    state = cases.make_state(cases.SEED, 8, 128)
    assert np.array_equal(bf.forward(state, x17, 8), ref.forward(state, x17, 8))
    for name in ("narrow", "odd", "static"):
        state = bcases.make_state(name)
        want, wfull = bref.forward(name, state, x[rows], full=True)
        got, gfull = bf.better_forward(name, state, x[rows], full=True)
        assert np.array_equal(got, want)
        assert set(gfull) == set(wfull) and all(np.array_equal(gfull[key], wfull[key]) for key in wfull)
    with pytest.raises(ValueError):
        bf.forward(state, x[rows], 8, operands="fp16")


def test_layer_functions_chain_to_the_forward(golden):
    """The per-layer functions applied to the forward's own intermediates give the forward's next tensor, in both
    modes; in bf16 mode only layers with Cin >= 32 and the pooled convolution move."""
    x, size = cases.fixture_inputs(golden, "ellipsoid")
    x = x[cases.config_rows("k8_emb1024_ellipsoid", size)[:3]].astype(np.float32)
    state = cases.make_state(cases.SEED, 8, 128)
    net = bf.Net.dgcnn(8, 128)
    f32, full32 = bf.forward(state, x, 8, full=True)
    for operands in bf.OPERANDS:
        out, full = bf.forward(state, x, 8, full=True, operands=operands)
        for l in range(net.E):
            got = bf.edge_layer(state, l + 1, net.layer_input(l, x, full["cat"]), net.list_of(l, x, full["lists"]), operands)
            assert np.array_equal(got, full["cat"][:, net.cat_off[l]:net.cat_off[l + 1]])
        assert np.array_equal(bf.pooled_layer(state, 7, full["cat"], operands), full["pooled"])
        assert np.array_equal(bf.head(net, state, full["pooled"])[0], out)
    # layer 1 (Cin = 17) is not rounded; layer 2 is, by about 2^-9 of its bound
    assert np.array_equal(full["cat"][:, :64], full32["cat"][:, :64])
    nbr = net.list_of(1, x, None)
    d = np.abs(bf.edge_layer(state, 2, full32["cat"][:, :64], nbr, "bf16") - full32["cat"][:, 64:128])
    m = bf.edge_bound(state, 2, full32["cat"][:, :64], nbr, "bf16")
    assert 0 < (d / m).max() <= 2.0 ** -7                                        # two operands, 2^-9 each at most
    assert np.array_equal(bf.edge_layer(state, 2, full32["cat"][:, :64], nbr, "bf16", min_cin=65), full32["cat"][:, 64:128])


@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_what_the_mode_costs_on_the_goldens(golden, name):
    n = bf.golden_numbers(golden, name)
    g = golden(f"dgcnn_{name}")
    report(f"{name}: bf16 restatement vs the reference's float64 outputs, {len(n['dev'])} patches, nothing injected: "
           f"|dout| max {n['max_dev']:.2e} median {n['med_dev']:.2e}; angle between the normalised outputs max "
           f"{n['max_angle']:.3f} deg median {n['med_angle']:.3f} deg (the reference's own float32 run: max |dout| "
           f"{float(g['dev32_all']):.2e})")
    assert n["dev"].shape == (len(g["rows"]),) and np.isfinite(n["dev"]).all() and np.isfinite(n["angle"]).all()
    assert bf.golden_numbers(golden, name) is n                                 # computed once
    # rounding two operands to 8 bits cannot beat float32, and stays a perturbation: the outputs are O(1)
    assert 0 < n["med_dev"] <= n["max_dev"] < 0.25
