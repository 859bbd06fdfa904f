"""The DGCNN forward on the device (csrc/dgcnn.hip, PatchGeneration/Modules/Network/GCNModel.py), stage by stage.

The neighbour search in feature space is the one discontinuous step: a rounding-sized change of a distance can swap a
neighbour and move the output by far more than rounding.  So the search is checked on its own (its chosen set is valid
within the rounding of the distances), the arithmetic is checked with the device's OWN lists handed to the float64
restatement (tests/dgcnn_ref.py), and only the last test compares against the reference's golden outputs with nothing
injected -- within 8 x the deviation the reference's own float32 run shows from its float64 run on that fixture.
No patch is excluded anywhere.  Measured figures are reported (conftest.report) before they are asserted.
"""
import numpy as np
import pytest
import torch

import dgcnn_cases as cases
import dgcnn_ref as ref
import patch_cases
from conftest import report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.fixture(scope="module")
def mods(gpu):
    import pcd_native as nat
    from PatchGeneration.Modules.Mesh import Mesh
    from PatchGeneration.Modules.Network.GCNModel import DGCNN
    from PatchGeneration.Modules.PatchCollector import PatchCollector, PatchDataset
    return {"nat": nat, "DGCNN": DGCNN, "Mesh": Mesh, "PatchCollector": PatchCollector, "PatchDataset": PatchDataset,
            "dev": gpu}


def torch_state(state):
    return {key: torch.as_tensor(np.asarray(v)) for key, v in state.items()}


def model_for(mods, k, emb):
    def make():
        m = mods["DGCNN"](k, 17, emb, 0.5)
        m.load_state_dict(torch_state(cases.make_state(cases.SEED, k, emb)), strict=True)
        return m.to(mods["dev"]).eval()
    return cached(("model", k, emb), make)


def fixture(golden, name):
    return cached(("inputs", name), lambda: cases.fixture_inputs(golden, name))


def device_run(mods, golden, name):
    """One debug forward of a configuration's rows: (x float64 [n, 20, 64], out, debug dict), numpy."""
    def make():
        k, emb, fx, _ = cases.CONFIGS[name]
        x = fixture(golden, fx)[0][golden(f"dgcnn_{name}")["rows"]]
        out, dbg = model_for(mods, k, emb)(torch.as_tensor(x, dtype=torch.float32).to(mods["dev"]), debug=True)
        torch.cuda.synchronize()
        return x, out.cpu().numpy().astype(np.float64), {key: v.cpu().numpy() for key, v in dbg.items()}
    return cached(("run", name), make)


def sqdist_dev(x):
    """x [b, C, 64] (device) -> float64 D [b, 64, 64]."""
    x = x.to(torch.float64)
    d = x[:, :, :, None] - x[:, :, None, :]
    return (d * d).sum(1)


# ------------------------------------------------------------------------------------------------ 1. GEMM edges
def _int_operands(M, K, b, nodes):
    m, k = np.arange(M)[:, None], np.arange(K)[None, :]
    w = ((5 * m + 3 * k + (m * k) % 7) % 7 - 3).astype(np.float32)              # asymmetric, in [-3, 3]
    shape = (b, K, 64) if nodes == 64 else (K, b)
    e = np.arange(int(np.prod(shape))).reshape(shape)
    x = ((e * 7 + e // 5) % 9 - 4).astype(np.float32)                           # integers in [-4, 4]
    s = np.array([0.5, -1.0, 2.0, 1.0, -0.25])[np.arange(M) % 5].astype(np.float32)
    t = ((np.arange(M) * 3) % 11 - 5).astype(np.float32)
    return w, x, s, t


def _lrelu32(v):
    """LeakyReLU(0.2) as float32 computes it, on float64 values that are float32 numbers (the product is exact in
    float64, so its one rounding is float32's)."""
    return np.where(v > 0, v, (np.float64(np.float32(0.2)) * v).astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("M,K,b", [(64, 17, 1), (3, 64, 5), (130, 1024, 2), (512, 256, 33)])
def test_gemm_edges_are_exact(mods, M, K, b):
    nat, dev = mods["nat"], mods["dev"]
    for nodes in (64, 1):
        w, x, s, t = _int_operands(M, K, b, nodes)
        y = np.einsum("mk,bkn->bmn", w.astype(np.float64), x.astype(np.float64)) if nodes == 64 else \
            w.astype(np.float64) @ x.astype(np.float64)
        assert np.abs(y).max() < 2 ** 24
        sb = s.astype(np.float64)[:, None]
        tb = t.astype(np.float64)[:, None]
        affine = sb * y + tb                                                    # exact: s is a power of two
        wd, xd, sd, td = (torch.as_tensor(a).to(dev) for a in (w, x, s, t))
        got = {e: nat.dgcnn_gemm(wd, xd, e, sd, td).cpu().numpy().astype(np.float64)
               for e in (nat.EPI_PLAIN, nat.EPI_AFFINE_LRELU, nat.EPI_AFFINE)}
        assert np.array_equal(got[nat.EPI_PLAIN], y), (M, K, b, nodes, "plain")
        assert np.array_equal(got[nat.EPI_AFFINE], affine), (M, K, b, nodes, "affine")
        assert np.array_equal(got[nat.EPI_AFFINE_LRELU], _lrelu32(affine)), (M, K, b, nodes, "affine + lrelu")
        if nodes == 64:
            act = _lrelu32(affine).astype(np.float32)                           # [b, M, 64]
            # the kernel's order: 4 runs of 16 columns summed in column order, then (q0 + q1) + (q2 + q3)
            q = np.zeros((b, M, 4), np.float32)
            for c in range(16):
                q = q + act.reshape(b, M, 4, 16)[..., c]
            mean = ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) * np.float32(1 / 64)
            pooled = nat.dgcnn_gemm(wd, xd, nat.EPI_POOL, sd, td).cpu().numpy()
            assert pooled.shape == (b, 2 * M)
            assert np.array_equal(pooled[:, :M], act.max(-1)), (M, K, b, "pooled max")
            assert np.array_equal(pooled[:, M:], mean), (M, K, b, "pooled mean")


# ------------------------------------------------------------------------------------------------ 2. edge convolution
@pytest.mark.parametrize("layer", [1, 3, 4, 6])
@pytest.mark.parametrize("b", [1, 3])
def test_edgeconv_against_restatement(mods, layer, b):
    nat, dev = mods["nat"], mods["dev"]
    model = model_for(mods, 8, 128)
    state = cases.make_state(cases.SEED, 8, 128)
    cin = cases.EDGE[layer - 1][0]
    rng = np.random.default_rng([layer, b])
    x = rng.normal(0.0, 1.0, (b, cin, 64)).astype(np.float32)
    xd = torch.as_tensor(x).to(dev)
    if layer <= 3:
        lists = rng.integers(0, 64, (b, 64, 3)).astype(np.int32)
    else:
        lists = nat.dgcnn_knn(xd, 8).cpu().numpy()                              # the device's own lists
    got = model.native().edgeconv(layer, xd, torch.as_tensor(lists).to(dev)).cpu().numpy().astype(np.float64)
    x64, l64 = x.astype(np.float64), lists.astype(np.int64)
    want = ref.edge(state, layer, x64, l64)
    bound = (2 * cin + 16) * U * ref.edge_bound(state, layer, x64, l64)
    ratio = float((np.abs(got - want) / bound).max())
    report(f"edgeconv layer {layer} b={b}: max |device - float64| / ((2 Cin + 16) 2^-24 M) = {ratio:.3f}")
    assert got.shape == want.shape and ratio <= 1.0


# ------------------------------------------------------------------------------------------------ 3. k-NN validity
def _check_knn(x, lists, k, what):
    """x [b, C, 64], lists int [b, 64, k] on the device: every row's set is the k nearest within the rounding bound."""
    D = sqdist_dev(x)
    norm = torch.linalg.vector_norm(x.to(torch.float64), dim=1)                 # [b, 64]
    bi = (x.size(1) + 4) * U * ((norm[:, :, None] + norm[:, None, :]) ** 2).amax(-1)
    lists = lists.to(torch.int64)
    assert int(lists.min()) >= 0 and int(lists.max()) <= 63
    member = torch.zeros_like(D, dtype=torch.bool).scatter_(2, lists, True)
    assert bool((member.sum(-1) == k).all()), f"{what}: a row's list does not have {k} distinct members"
    # the list is ascending in (distance, index): non-decreasing within the distances' rounding, and where two
    # consecutive entries are at exactly one distance (identical padding rows) the lower index comes first
    dl = torch.gather(D, 2, lists)
    assert bool((dl[..., :-1] - dl[..., 1:] <= 2 * bi[..., None]).all()), f"{what}: a list is not ascending"
    assert bool(((dl[..., :-1] != dl[..., 1:]) | (lists[..., :-1] < lists[..., 1:])).all()), \
        f"{what}: a tie is not in index order"
    inf = torch.full_like(D, float("inf"))
    worst_in = torch.where(member, D, -inf).amax(-1)
    best_out = torch.where(member, inf, D).amin(-1)
    if k == 64:
        return 0.0
    over = (worst_in - best_out).clamp_min(0.0)                                 # 0: the set is exactly the k nearest
    slack = torch.where(over > 0, over / (2 * bi).clamp_min(1e-300), over)      # <= 1 is valid
    return float(slack.max())


@pytest.mark.parametrize("k,fx", [(8, "ellipsoid"), (8, "shells"), (1, "ellipsoid"), (1, "shells"),
                                  (20, "ellipsoid"), (20, "shells"), (64, "ellipsoid")])
def test_knn_sets_are_valid(mods, golden, k, fx):
    x = fixture(golden, fx)[0]
    if k == 64:
        x = x[:2]
    model = model_for(mods, k, 128)
    _, dbg = model(torch.as_tensor(x, dtype=torch.float32).to(mods["dev"]), debug=True)
    worst = max(_check_knn(dbg["cat"][:, lo:hi], dbg["lists"][layer], k, f"k={k} {fx} layer {layer + 4}")
                for layer, (lo, hi) in enumerate(ref.DYN_INPUT))
    report(f"k-NN k={k} on {len(x)} {fx} patches: max (worst chosen - best left out) / (2 b_i) = {worst:.3f}")
    assert worst <= 1.0
    # the stage entry gives the same lists
    again = mods["nat"].dgcnn_knn(dbg["cat"][:, 128:256].contiguous(), k)
    assert torch.equal(again, dbg["lists"][0])


# ------------------------------------------------------------------------------------------------ 4. lists injected
@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_forward_against_restatement_with_device_lists(mods, golden, name):
    k, emb, _, _ = cases.CONFIGS[name]
    g = golden(f"dgcnn_{name}")
    x, out, dbg = device_run(mods, golden, name)
    state = cases.make_state(cases.SEED, k, emb)
    want, full = ref.forward(state, x.astype(np.float32), k, lists=dbg["lists"], full=True)
    tol = 8.0 * float(g["dev32_stable"])
    dev = float(np.abs(out - want).max())
    inner = {key: float(np.abs(dbg[key].astype(np.float64) - full[key]).max()) for key in ("cat", "pooled")}
    hid = {key: float(np.abs(dbg[key].astype(np.float64).T - full[key]).max()) for key in ("h1", "h2", "h3")}
    report(f"{name}: device vs float64 restatement on the device's lists, {len(x)} patches: max |dout| {dev:.2e} "
           f"(allowed {tol:.2e} = 8 x the reference's float32 deviation where no neighbour differs); "
           f"concatenation {inner['cat']:.1e}, pooled {inner['pooled']:.1e}, hidden {max(hid.values()):.1e}")
    assert dev <= tol


# ------------------------------------------------------------------------------------------------ 5. against the golden
@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_forward_against_reference_golden(mods, golden, name):
    k, emb, _, _ = cases.CONFIGS[name]
    g = golden(f"dgcnn_{name}")
    x, out, dbg = device_run(mods, golden, name)
    dev = np.abs(out - g["out64"]).max(-1)
    differ = np.zeros(len(x), bool)
    cat = torch.as_tensor(dbg["cat"]).to(mods["dev"])
    for layer, (lo, hi) in enumerate(ref.DYN_INPUT):
        D = sqdist_dev(cat[:, lo:hi])
        pick = lambda l: torch.sort(torch.gather(D, 2, torch.as_tensor(l.astype(np.int64)).to(D.device)), -1)[0]
        differ |= (pick(dbg["lists"][layer]) != pick(g["lists64"][layer])).any(-1).any(-1).cpu().numpy()
    tol, tight = 8.0 * float(g["dev32_all"]), 8.0 * float(g["dev32_stable"])
    agree = float(dev[~differ].max()) if (~differ).any() else 0.0
    report(f"{name}: device vs the reference's float64 outputs, {len(x)} patches, nothing injected: max |dout| "
           f"{dev.max():.2e} (allowed {tol:.2e} = 8 x the reference's own float32 run on the fixture); lists differ "
           f"from the golden's by distance on {int(differ.sum())} patches (the reference's float32 run on the same "
           f"rows: {int(g['differs32'].sum())}); max |dout| where they agree {agree:.2e} (allowed {tight:.2e} = 8 x the "
           f"reference's float32 deviation where no neighbour differs)")
    assert dev.max() <= tol
    # where the device chose the golden's neighbours (by distance) only rounding is left: test 4's allowance
    assert agree <= tight


# ------------------------------------------------------------------------------------------------ 6. invariants
def test_bits_do_not_depend_on_the_batch(mods, golden):
    dev = mods["dev"]
    model = model_for(mods, 8, 128)
    x = torch.as_tensor(fixture(golden, "ellipsoid")[0][:33], dtype=torch.float32).to(dev)
    one = model(x[5:6])
    assert torch.equal(model(x[5:6]), one)                                      # run to run
    assert torch.equal(model(torch.cat([x[5:6], x[0:1]]))[0:1], one)            # row 0 of 2
    big = torch.cat([x[:32], x[5:6]])
    got = model(big)
    assert torch.equal(got[32:33], one)                                         # row 32 of 33
    assert torch.equal(got, model(big))
    assert torch.equal(got[5:6], one)


def test_nan_stays_in_its_patch(mods, golden):
    model = model_for(mods, 8, 128)
    x = torch.as_tensor(fixture(golden, "ellipsoid")[0][:3], dtype=torch.float32).to(mods["dev"])
    clean = model(x)
    for bad in (float("nan"), float("inf")):
        y = x.clone()
        y[1, 4, 7] = bad
        out = model(y)
        assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])
        assert not bool(torch.isfinite(out[1]).all())
    assert torch.equal(model(x), clean)


@pytest.mark.parametrize("bad", [64.0, -1.0, float("nan"), 1e30])
def test_bad_index_column_is_refused(mods, golden, bad):
    model = model_for(mods, 8, 128)
    x = torch.as_tensor(fixture(golden, "ellipsoid")[0][:3], dtype=torch.float32).to(mods["dev"])
    clean = model(x)
    y = x.clone()
    y[2, 18, 40] = bad
    y[1, 19, 3] = bad
    with pytest.raises(ValueError, match="patch 1 "):
        model(y)
    y[1, 19, 3] = 63.9                                                          # truncates to 63, as .long() does
    with pytest.raises(ValueError, match="patch 2 "):
        model(y)
    torch.cuda.synchronize()
    assert torch.equal(model(x), clean)                                         # and nothing faulted


def test_deferred_index_check(mods, golden):
    """Without the host wait: a bad index column is recorded, clamped and faults nothing; the other patches' bits stay."""
    nat, dev = mods["nat"], mods["dev"]
    model = model_for(mods, 8, 128)
    x = torch.as_tensor(fixture(golden, "ellipsoid")[0][:4], dtype=torch.float32).to(dev)
    clean = model(x)
    flag = torch.full((1,), nat.DGCNN_NO_BAD_PATCH, dtype=torch.int32, device=dev)
    assert torch.equal(model(x, first_bad=flag, patch_base=100), clean) and int(flag) == nat.DGCNN_NO_BAD_PATCH
    y = x.clone()
    y[3, 17, 5] = float("nan")
    y[1, 19, 9] = 1e9
    out = model(y, first_bad=flag, patch_base=100)
    assert int(flag) == 101
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2]) and bool(torch.isfinite(out).all())
    model(x, first_bad=flag, patch_base=0)                                      # the flag keeps the lowest
    assert int(flag) == 101
    with pytest.raises(ValueError, match="first_bad"):
        model(x, first_bad=flag.cpu())
    with pytest.raises(ValueError, match="first_bad"):
        model(x, first_bad=flag.to(torch.int64))
    assert torch.equal(model(x), clean)


def test_arguments(mods, golden):
    model = model_for(mods, 8, 128)
    x = torch.as_tensor(fixture(golden, "ellipsoid")[0][:2], dtype=torch.float32).to(mods["dev"])
    need = model.native().workspace_bytes(2)
    short = torch.empty(need - 256, dtype=torch.uint8, device=mods["dev"])
    with pytest.raises(ValueError, match="workspace"):
        model(x, workspace=short)
    ws = torch.empty(need + 64, dtype=torch.uint8, device=mods["dev"])
    assert torch.equal(model(x, workspace=ws), model(x))
    with pytest.raises(ValueError, match="workspace"):                          # a host tensor is no device address
        model(x, workspace=torch.empty(need, dtype=torch.uint8))
    with pytest.raises(ValueError, match="aligned"):
        model(x, workspace=ws[4:])
    with pytest.raises(ValueError, match="workspace"):
        model(x, workspace=ws[::2])
    assert torch.equal(model(x.to(torch.float64)), model(x))                    # float64 is cast
    with pytest.raises(ValueError):
        model(x.cpu())
    with pytest.raises(ValueError):
        model(x[:, :19])
    assert model(x[:0]).shape == (0, 3)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="eval"):
            model(x)
    finally:
        model.eval()
    with pytest.raises(ValueError):
        mods["DGCNN"](8, 16, 128, 0.5)
    st = torch_state(cases.make_state(cases.SEED, 8, 128))
    conv = [st[f"conv{i}.0.weight"] for i in range(1, 8)]
    bn = [(st[f"bn{i}.weight"], st[f"bn{i}.bias"], st[f"bn{i}.running_mean"], st[f"bn{i}.running_var"], 1e-5)
          for i in range(1, 11)]
    lin = [(st[f"linear{i}.weight"], st.get(f"linear{i}.bias")) for i in range(1, 5)]
    nat = mods["nat"]
    assert torch.equal(nat.Dgcnn(conv, bn, lin, 8, 17, 128).forward(x), model(x))    # host pointers work too
    with pytest.raises(ValueError, match="conv3"):
        nat.Dgcnn(conv[:2] + [conv[1]] + conv[3:], bn, lin, 8, 17, 128)
    with pytest.raises(ValueError, match="init_dims"):
        nat.Dgcnn(conv, bn, lin, 8, 16, 128)
    with pytest.raises(ValueError, match="linear1"):
        nat.Dgcnn(conv, bn, [(lin[0][0], lin[1][1])] + lin[1:], 8, 17, 128)
    with pytest.raises(ValueError):
        nat.Dgcnn(conv, bn, lin, 65, 17, 128)


# ------------------------------------------------------------------------------------------------ 7. module
class _TorchLayout(torch.nn.Module):
    """The layer table as plain torch modules (each batch norm registered on its own and inside its convolution's
    Sequential): the state-dict layout a checkpoint of the network has."""

    def __init__(self, emb, out_ch=3):
        super().__init__()
        nn = torch.nn
        for i, (cin, cout) in enumerate(cases.EDGE, start=1):
            bn = nn.BatchNorm2d(cout)
            setattr(self, f"bn{i}", bn)
            setattr(self, f"conv{i}", nn.Sequential(nn.Conv2d(2 * cin, cout, 1, bias=False), bn, nn.LeakyReLU(0.2)))
        self.bn7 = nn.BatchNorm1d(emb)
        self.conv7 = nn.Sequential(nn.Conv1d(1024, emb, 1, bias=False), self.bn7, nn.LeakyReLU(0.2))
        width = 2 * emb
        for i, out in enumerate(cases.HEAD, start=1):
            setattr(self, f"linear{i}", nn.Linear(width, out, bias=i > 1))
            setattr(self, f"bn{7 + i}", nn.BatchNorm1d(out))
            width = out
        self.linear4 = nn.Linear(width, out_ch)


def test_module_state_dict_and_repacking(mods, golden):
    dev = mods["dev"]
    torch.manual_seed(3)
    plain = _TorchLayout(128)
    for name, buf in plain.named_buffers():
        if name.endswith("running_var"):
            buf.uniform_(0.5, 1.5)
        elif name.endswith("running_mean"):
            buf.normal_(0.0, 0.1)
    sd = plain.state_dict()
    assert set(sd) == set(cases.make_state(cases.SEED, 8, 128))                 # the fixtures' keys are torch's
    model = mods["DGCNN"](8, 17, 128, 0.5)
    model.load_state_dict(sd, strict=True)
    back = model.state_dict()
    assert sorted(back) == sorted(sd) and all(torch.equal(back[key], sd[key]) for key in sd)
    model = model.to(dev).eval()
    x = torch.as_tensor(fixture(golden, "ellipsoid")[0][:4], dtype=torch.float32).to(dev)
    first = model(x)
    want = ref.forward({key: v.numpy() for key, v in sd.items()}, x.cpu().numpy(), 8,
                       lists=model(x, debug=True)[1]["lists"].cpu().numpy())
    assert np.abs(first.cpu().numpy() - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    assert torch.equal(model(x), first)
    with torch.no_grad():
        model.linear4.bias += 1.0                                               # in place: the version counter moves
    shifted = model(x)
    assert float((shifted - (first + 1.0)).abs().max()) <= 1e-6 and not torch.equal(shifted, first)
    with torch.no_grad():
        model.bn3.running_mean.add_(0.5)                                        # a buffer, through its alias conv3.1
    moved = model(x)
    assert float((moved - shifted).abs().max()) > 1e-4
    model.load_state_dict(sd, strict=True)
    assert torch.equal(model(x), first)
    assert torch.equal(model.cpu().to(dev)(x), first)                           # .to() re-packs


# ------------------------------------------------------------------------------------------------ 8. pipeline
def test_predict_normals_on_the_ellipsoid(mods, golden):
    dev = mods["dev"]
    g = patch_cases.load_golden("ellipsoid")
    model = model_for(mods, 8, 128)
    mesh = mods["Mesh"](g["v"].copy(), g["f"].copy())
    pc = mods["PatchCollector"](mesh, int(g["k"]))
    normals, fallbacks = pc.predictNormals(model, batch_faces=100)
    assert normals.shape == (320, 3) and normals.dtype == torch.float64 and normals.is_cuda and fallbacks == 0
    # the same chunks by hand: model, unalign (R^T o), normalise
    ds = pc.collectNetworkInput(256, dtype=np.float32)
    x = torch.as_tensor(np.ascontiguousarray(ds.data_patch.transpose(0, 2, 1))).to(dev)
    o = model(x).cpu().numpy().astype(np.float64)
    by_hand = ds.unalign(o)
    by_hand /= np.linalg.norm(by_hand, axis=1, keepdims=True)
    assert np.abs(normals.cpu().numpy() - by_hand).max() <= 1e-14
    one, _ = pc.predictNormals(model, batch_faces=4096, faces=[7, 300, 11])
    assert float((one - normals[[7, 300, 11]]).abs().max()) <= 1e-14
    # and from the reference's own inputs and rotations, where its middle axis has this project's sign (a patch
    # with the other sign is a mirrored input, to which the network owes no mirrored answer)
    faces = g["input_faces"]
    same = np.einsum("ni,ni->n", g["rot"][faces][:, 1], ds.data_rotations[faces][:, 1]) > 0
    xg = torch.as_tensor(fixture(golden, "ellipsoid")[0], dtype=torch.float32).to(dev)
    og = model(xg).cpu().numpy().astype(np.float64)
    want = np.einsum("nij,ni->nj", g["rot"][faces], og)
    scale = np.linalg.norm(want, axis=1)
    want /= scale[:, None]
    # (on these patches the device's float32 input is the golden's, so no neighbour can differ: the allowance is the
    # one for rounding alone)
    tol = 8.0 * float(golden("dgcnn_k8_emb128_ellipsoid")["dev32_stable"])
    dev_n = np.abs(normals.cpu().numpy()[faces] - want).max(-1) * scale          # back on the output's scale
    report(f"predictNormals vs model on the golden inputs + R^T: {int(same.sum())} of {len(faces)} stored patches "
           f"carry the golden's middle-axis sign; max deviation there {dev_n[same].max():.2e} (allowed {tol:.2e})")
    assert int(same.sum()) == 78 and len(faces) == 127                         # what the fixture has
    assert dev_n[same].max() <= tol


def test_predict_normals_fallback_and_denoise(mods):
    dev = mods["dev"]
    model = model_for(mods, 8, 128)
    v, f, needle = patch_cases.needle_far()
    mesh = mods["Mesh"](v.copy(), f.copy())
    normals, fallbacks = mods["PatchCollector"](mesh).predictNormals(model)
    assert fallbacks == 1 and normals.shape == (len(f), 3)
    own = torch.as_tensor(mesh.getFaceNormals()).to(dev)
    assert float((normals[needle] - own[needle]).abs().max()) <= 1e-12      # the needle's own normal
    assert bool((torch.linalg.vector_norm(normals, dim=1) - 1).abs().max() < 1e-12)
    # Mesh.denoise takes the device tensor as it takes the same values from numpy
    g = patch_cases.load_golden("ellipsoid")
    a, b = mods["Mesh"](g["v"].copy(), g["f"].copy()), mods["Mesh"](g["v"].copy(), g["f"].copy())
    guide, _ = mods["PatchCollector"](a).predictNormals(model)
    na = a.denoise(guided_normals=guide, normal_iterations=2, vertex_iterations=3)
    nb = b.denoise(guided_normals=guide.cpu().numpy(), normal_iterations=2, vertex_iterations=3)
    assert np.array_equal(na, nb) and np.array_equal(a.v, b.v)
