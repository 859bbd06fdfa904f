#!/usr/bin/env python3
"""Time BetterDGCNN on the device: the fused narrow edge layer against the two-kernel path, a 4096-patch eval() chunk
and one training step of two networks, each next to the same network as torch-eager modules on the same device.

  python tools/better_dgcnn_probe.py [--chunk 4096] [--train-batch 256] [--repeat 5] [--eager-repeat 3]
                                     [--operands fp32|bf16]

Everything is timed between HIP events on the current stream: one warm-up, then --repeat runs; median and spread
(max - min of the runs).
  fused      pcd_bdgcnn_edgeconv with fused off / on at (Cin, Cout, list length) = (17, 64, 3), (64, 64, 3),
             (64, 64, 8), (32, 32, 8), (17, 16, 3) and, for the dispatch rule's edges, longer lists and wider inputs,
             b = --chunk.  The scratch (packed weight, the product P) and the output are allocated once, outside: a
             call launches the weight pack and the layer's kernels and nothing else, as the forward does from its
             workspace.  A timed window is --inner calls; the two arms alternate window by window; ms per call.
             "wins" where the slowest fused window beats the fastest two-kernel window.
  eval       BetterDGCNN.forward in eval() on --chunk patches: the table-default network (DGCNN's widths, emb 128) and
             a narrow one (every convolution <= 64 wide), one workspace, index check deferred
  train      one step (forward, the trainer's loss, backward) of each at --train-batch patches
  eager      the same modules as plain torch ops (the edge tensors [b, 2 C, 64, n] materialised)
The inputs are random features with valid index columns and the weights torch's default initialisation: the time
does not depend on them.  One JSON line.
--operands bf16 runs the fused comparison and eval() in the opt-in bf16-operand mode (pcd_bdgcnn_edgeconv_bf16, the
models built with operands="bf16"); train() is float32 whatever it says.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "normal-guided-pointcloud-denoiser_amd"))

import pcd_native as nat  # noqa: E402
from PatchGeneration.Modules.Network.GCNModel import BetterDGCNN  # noqa: E402

FUSED_SHAPES = ((17, 64, 3), (64, 64, 3), (64, 64, 8), (32, 32, 8), (17, 16, 3),
                (64, 64, 20), (64, 64, 64), (17, 16, 64), (256, 64, 8), (1024, 64, 8), (1024, 64, 64))
NETWORKS = {
    "default": (3, 3, 4, (64, 64, 128, 256, 256, 256, 128, 512, 256, 64), 8),
    "narrow": (3, 3, 4, (32, 32, 64, 64, 64, 64, 64, 128, 64, 32), 8),
}


def timed(fn):
    """(result, ms) of fn() between two events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
            "spread": round(max(ts) - min(ts), 4)}


def measure(fn, repeat):
    """{"median", "min", "max", "spread"} in ms: one warm-up, then `repeat` runs."""
    fn()
    return summary([timed(fn)[1] for _ in range(repeat)])


def measure_alternating(fns, repeat, inner):
    """One summary per function, ms per call: a warm-up window of each, then `repeat` rounds of one window of `inner`
    calls of each function in turn."""
    def window(fn):
        for _ in range(inner):
            fn()
    ts = [[] for _ in fns]
    for r in range(repeat + 1):
        for i, fn in enumerate(fns):
            ms = timed(lambda: window(fn))[1] / inner
            if r:
                ts[i].append(ms)
    return [summary(t) for t in ts]


def random_inputs(b, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((b, 20, 64), generator=g)
    x[:, 17:20] = torch.randint(0, 64, (b, 3, 64), generator=g).to(torch.float32)
    return x.to(dev)


def build(name, dev, trainable, operands="fp32"):
    l_e, l_d, l_l, sizes, k = NETWORKS[name]
    torch.manual_seed(0)
    model = BetterDGCNN(l_e, l_d, l_l, sizes, k, 17, 0.0, trainable=trainable, operands=operands)
    for key, buf in model.named_buffers():
        if key.endswith("running_var"):
            buf.uniform_(0.5, 1.5)
        elif key.endswith("running_mean"):
            buf.normal_(0.0, 0.1)
    return model.to(dev)


def eager(model, x):
    """The network as plain torch ops on the module's own layers."""
    t = model.table
    static_nbr = x[:, 17:20].to(torch.int64).transpose(1, 2)           # [b, 64, 3]

    def edge_tensor(h, nbr):                                           # h [b, C, 64], nbr [b, 64, n]
        b, c, rows = h.shape
        n = nbr.size(2)
        centre = h[:, :, :, None].expand(b, c, rows, n)
        picked = torch.gather(centre, 2, nbr[:, None].expand(b, c, rows, n))
        return torch.cat([picked - centre, centre], dim=1)

    def nearest(h):
        gram = h.transpose(1, 2) @ h
        n2 = (h * h).sum(1)
        return torch.topk(2 * gram - n2[:, :, None] - n2[:, None, :], t.k, dim=2).indices

    h, layers = x[:, :17], []
    for i in range(1, t.n_edge + 1):
        nbr = static_nbr if i <= t.l_e else nearest(h.detach())
        h = getattr(model, f"conv{i}")(edge_tensor(h, nbr)).amax(dim=3)
        layers.append(h)
    y = getattr(model, f"conv{t.n_edge + 1}")(torch.cat(layers, dim=1))
    h = torch.cat([y.amax(dim=2), y.mean(dim=2)], dim=1)
    for j in range(1, t.l_l):
        h = F.leaky_relu(getattr(model, f"bn{t.n_edge + 1 + j}")(getattr(model, f"linear{j}")(h)))
    return getattr(model, f"linear{t.l_l}")(h)


def trainer_loss(out, gt):
    ones = torch.ones(len(out), dtype=torch.float32, device=out.device)
    return 0.5 * F.cosine_embedding_loss(out, gt, ones) + 0.5 * F.mse_loss(out, gt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--train-batch", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--eager-repeat", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window of the fused comparison")
    ap.add_argument("--operands", choices=("fp32", "bf16"), default="fp32")
    a = ap.parse_args()
    dev = nat.device()
    res = {"build": nat.build_id(), "operands": a.operands, "chunk": a.chunk, "train_batch": a.train_batch,
           "repeat": a.repeat, "fused": [], "eval": {}, "train": {}}

    g = torch.Generator(device="cpu").manual_seed(1)
    for cin, cout, n in FUSED_SHAPES:
        w = (torch.rand((cout, 2 * cin), generator=g) * 2 - 1).to(dev)
        s, t = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
        x = torch.randn((a.chunk, cin, 64), generator=g).to(dev)
        lists = torch.randint(0, 64, (a.chunk, 64, n), generator=g).to(torch.int32).to(dev)
        scratch = torch.empty(nat.bdgcnn_edgeconv_scratch_bytes(cin, cout, a.chunk), dtype=torch.uint8, device=dev)
        outs = [torch.empty((a.chunk, cout, 64), dtype=torch.float32, device=dev) for _ in range(2)]
        off, on = measure_alternating(
            [lambda: nat.bdgcnn_edgeconv(w, s, t, x, lists, nat.FUSED_OFF, scratch, outs[0], a.operands),
             lambda: nat.bdgcnn_edgeconv(w, s, t, x, lists, nat.FUSED_ON, scratch, outs[1], a.operands)],
            a.repeat, a.inner)
        same = torch.equal(outs[0], outs[1])
        del scratch, outs, x, lists
        res["fused"].append({"cin": cin, "cout": cout, "list_len": n, "two_kernels_ms": off, "fused_ms": on,
                             "speedup": round(off["median"] / on["median"], 3), "same_bits": same,
                             "wins": on["max"] < off["min"]})

    for name in NETWORKS:
        model = build(name, dev, False, a.operands).eval()
        x = random_inputs(a.chunk, dev)
        ws = model.native().workspace(a.chunk)
        flag = torch.full((1,), nat.DGCNN_NO_BAD_PATCH, dtype=torch.int32, device=dev)
        hip = measure(lambda: model(x, workspace=ws, first_bad=flag), a.repeat)
        with torch.no_grad():
            eg = measure(lambda: eager(model, x), a.eager_repeat)
            diff = float((eager(model, x) - model(x, workspace=ws)).abs().median())
        res["eval"][name] = {"hip_ms": hip, "eager_ms": eg, "eager_over_hip": round(eg["median"] / hip["median"], 2),
                             "workspace_MB": round(ws.numel() / 2 ** 20, 1), "eager_vs_hip_median_abs": diff}
        del ws

        model = build(name, dev, True).train()
        xt = random_inputs(a.train_batch, dev, seed=2)
        gt = F.normalize(torch.randn((a.train_batch, 3), generator=g), dim=1).to(dev)

        def step(forward):
            model.zero_grad(set_to_none=True)
            trainer_loss(forward(xt), gt).backward()

        hip = measure(lambda: step(model), a.repeat)
        eg = measure(lambda: step(lambda v: eager(model, v)), a.eager_repeat)
        res["train"][name] = {"hip_ms": hip, "eager_ms": eg, "eager_over_hip": round(eg["median"] / hip["median"], 2),
                              "workspace_MB": round(nat.bdgcnn_train_workspace_bytes(model.table, a.train_batch) / 2 ** 20, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
