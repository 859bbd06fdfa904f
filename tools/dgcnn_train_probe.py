#!/usr/bin/env python3
"""Time one DGCNN training step on the device (train-mode forward, backward, and the whole step with Adam), and the
same network as torch-eager modules in train() on the same device.

  python tools/dgcnn_train_probe.py [--mesh data/stanford_bunny_mesh.npz] [--batches 256,4096] [--k 8] [--emb 1024]
                                    [--repeat 5] [--no-eager] [--once]

Per batch size b (the first b patches of the mesh from PatchCollector.iterNetworkInput, float32, channels first;
seeded unit vectors as ground truth; the trainer's loss at weights 0.5 / 0.5; dropout 0.5), between HIP events on the
current stream, one warm-up and then the median of --repeat:
  forward   model(inputs) in train(): the trunk on the kernels of csrc/dgcnn_train.hip, the head in torch
  backward  loss.backward()
  step      zero_grad, forward, loss, backward, Adam step
  eager_*   the same three for the layer table as plain torch ops on the same modules (edge tensors materialised,
            torch's autograd): the comparison, never the code under test
and the three kinds of GEMM on conv7's shapes through the stage entries: forward W X, data gradient W^T dY added into
a buffer, weight gradient dY X^T.  TFLOP/s counts 2 x the multiply-adds of the GEMMs after the edge-weight split: 182
MFLOP a patch forward at emb = 1024, twice that backward (data and weight gradients; layer 1 has no data gradient).
--once runs a single step per batch size and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`
for per-kernel times.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "normal-guided-pointcloud-denoiser_amd"))

import pcd_native as nat  # noqa: E402
from PatchGeneration.Modules.Mesh import Mesh  # noqa: E402
from PatchGeneration.Modules.Network.GCNModel import DGCNN  # noqa: E402
from PatchGeneration.Modules.PatchCollector import PatchCollector  # noqa: E402

EDGE = ((17, 64), (64, 64), (64, 128), (128, 256), (256, 256), (256, 256))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def trunk_macs(emb):
    return 64 * (sum(2 * cout * cin for cin, cout in EDGE) + 1024 * emb)


def eager(model, x):
    """The network as plain torch ops on the module's own layers (tools/dgcnn_probe.py's layout), in the module's mode."""
    static_nbr = x[:, 17:20].to(torch.int64).transpose(1, 2)

    def edge_tensor(h, nbr):
        b, c, rows = h.shape
        n = nbr.size(2)
        centre = h[:, :, :, None].expand(b, c, rows, n)
        picked = torch.gather(centre, 2, nbr[:, None].expand(b, c, rows, n))
        return torch.cat([picked - centre, centre], dim=1)

    def nearest(h):
        with torch.no_grad():
            gram = h.transpose(1, 2) @ h
            n2 = (h * h).sum(1)
            return torch.topk(2 * gram - n2[:, :, None] - n2[:, None, :], model.k, dim=2).indices

    h, layers = x[:, :17], []
    for i in range(1, 7):
        nbr = static_nbr if i <= 3 else nearest(h)
        h = getattr(model, f"conv{i}")(edge_tensor(h, nbr)).amax(dim=3)
        layers.append(h)
    y = model.conv7(torch.cat(layers, dim=1))
    h = torch.cat([y.amax(dim=2), y.mean(dim=2)], dim=1)
    for i in range(1, 4):
        h = F.leaky_relu(getattr(model, f"bn{7 + i}")(getattr(model, f"linear{i}")(h)), 0.2)
        if i < 3:
            h = getattr(model, f"dp{i}")(h)
    return model.linear4(h)


def loss_of(out, gt):
    ones = torch.ones(len(out), dtype=torch.float32, device=out.device)
    return 0.5 * F.cosine_embedding_loss(out, gt, ones) + 0.5 * F.mse_loss(out, gt)


def measure(model, forward, x, gt, repeat):
    """Median ms of forward, backward and the whole step (with Adam) of `forward(model, x)`."""
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    model.train()

    def step():
        opt.zero_grad()
        loss = loss_of(forward(model, x), gt)
        loss.backward()
        opt.step()
        return loss

    step()                                                              # warm-up: code objects, Adam's state
    fw, bw, st = [], [], []
    for _ in range(repeat):
        opt.zero_grad()
        out, ms = timed(lambda: forward(model, x))
        fw.append(ms)
        loss = loss_of(out, gt)
        bw.append(timed(loss.backward)[1])
        del out, loss
        st.append(timed(step)[1])
    return {"forward_ms": round(statistics.median(fw), 3), "backward_ms": round(statistics.median(bw), 3),
            "step_ms": round(statistics.median(st), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default=os.path.join(ROOT, "data", "stanford_bunny_mesh.npz"))
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--emb", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    dev = nat.device()
    d = np.load(a.mesh)
    mesh = Mesh(np.asarray(d["v"], dtype=np.float64), np.asarray(d["f"], dtype=np.int64))
    pc = PatchCollector(mesh)
    res = {"mesh": os.path.basename(a.mesh), "k": a.k, "emb": a.emb, "repeat": a.repeat, "batches": {}}
    for b in (int(v) for v in a.batches.split(",")):
        x = next(pc.iterNetworkInput(b, np.arange(b), "reference", np.float32, channels_first=True)).inputs
        rng = np.random.default_rng(b)
        gt = rng.normal(size=(b, 3))
        gt = torch.as_tensor(gt / np.linalg.norm(gt, axis=1, keepdims=True), dtype=torch.float32).to(dev)
        torch.manual_seed(0)
        model = DGCNN(a.k, 17, a.emb, 0.5, trainable=True).to(dev)
        hip = lambda m, x_: m(x_)
        if a.once:
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=1e-4)
            for _ in range(2):                                          # the second step is the one to read
                opt.zero_grad()
                loss_of(hip(model, x), gt).backward()
                opt.step()
            torch.cuda.synchronize()
            continue
        r = measure(model, hip, x, gt, a.repeat)
        r["workspace_MB"] = round(nat.dgcnn_train_workspace_bytes(a.k, a.emb, b) / 2 ** 20, 1)
        macs = trunk_macs(a.emb) * b
        r["forward_TFLOPs"] = round(2 * macs / (r["forward_ms"] * 1e-3) / 1e12, 2)
        r["backward_TFLOPs"] = round(4 * macs / (r["backward_ms"] * 1e-3) / 1e12, 2)
        # the three GEMM kinds on conv7's shapes
        cat = torch.randn((b, 1024, 64), device=dev)
        dy = torch.randn((b, a.emb, 64), device=dev)
        w7 = model.conv7[0].weight.detach().reshape(a.emb, 1024)
        w7t = w7.t().contiguous()
        dcat = torch.zeros((b, 1024, 64), device=dev)
        flop = 2 * 1024 * a.emb * 64 * b
        for name, fn in (("gemm_forward", lambda: nat.dgcnn_gemm(w7, cat)),
                         ("gemm_data_gradient", lambda: nat.dgcnn_gemm(w7t, dy, nat.EPI_ADD, y=dcat)),
                         ("gemm_weight_gradient", lambda: nat.dgcnn_wgrad(dy, cat))):
            fn()
            ms = statistics.median(timed(fn)[1] for _ in range(a.repeat))
            r[name + "_ms"], r[name + "_TFLOPs"] = round(ms, 3), round(flop / (ms * 1e-3) / 1e12, 2)
        del cat, dy, dcat
        if not a.no_eager:
            torch.manual_seed(0)
            plain = DGCNN(a.k, 17, a.emb, 0.5, trainable=True).to(dev)
            e = measure(plain, eager, x, gt, a.repeat)
            r.update({"eager_" + key: v for key, v in e.items()})
            r["eager_over_hip_step"] = round(e["step_ms"] / r["step_ms"], 2)
            del plain
        res["batches"][str(b)] = r
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
