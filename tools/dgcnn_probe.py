#!/usr/bin/env python3
"""Time the DGCNN forward over every patch of a mesh (default: the Stanford bunny, 69,451 faces), and the same chunk
through a plain torch-eager statement of the network on the same device.

  python tools/dgcnn_probe.py [--mesh data/stanford_bunny_mesh.npz] [--faces N] [--chunk 4096] [--k 8] [--emb 1024]
                              [--repeat 5] [--eager-repeat 3] [--operands fp32|bf16]

Per pass over the faces, each stage between HIP events on the current stream (one warm-up pass first, then --repeat
passes; best and median):
  input      PatchCollector.iterNetworkInput (float32, channels first)
  forward    DGCNN.forward (pcd_dgcnn_forward), one workspace for all chunks
  unalign    R^T o, normalisation, fallback (what predictNormals adds)
and, on the first chunk alone, the forward's parts through the stage entries (pcd_dgcnn_knn / _edgeconv / _gemm) fed
with the forward's own debug tensors, and the eager network.  TFLOP/s counts 182 MFLOP per patch at emb = 1024 (the 91 M
multiply-adds of the GEMMs after splitting the edge weight, the searches not counted; the eager network does 240 M).  The weights are random (torch's default
initialisation, random running statistics): the time does not depend on them.  One JSON line.
--operands bf16 times the opt-in mode (bf16 GEMM operands, float32 accumulation): the model, the edge layers and the
pooled convolution's stage entry (pcd_dgcnn_gemm_bf16) then run the bf16 kernel; the eager network stays float32, so
eager_vs_hip_* then shows what the mode costs in precision.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "normal-guided-pointcloud-denoiser_amd"))

import pcd_native as nat  # noqa: E402
from PatchGeneration.Modules.Mesh import Mesh  # noqa: E402
from PatchGeneration.Modules.Network.GCNModel import DGCNN  # noqa: E402
from PatchGeneration.Modules.PatchCollector import PatchCollector  # noqa: E402


def timed(fn):
    """(result, ms) of fn() between two events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def flops_per_patch(emb):
    """2 x the multiply-adds of the GEMMs after the edge-weight split (182 MFLOP at emb = 1024); the neighbour
    searches and the max over neighbours are not counted."""
    edge = sum(2 * cout * cin for cin, cout in ((17, 64), (64, 64), (64, 128), (128, 256), (256, 256), (256, 256)))
    macs = 64 * (edge + 1024 * emb) + 2 * emb * 512 + 512 * 256 + 256 * 64 + 64 * 3
    return 2 * macs


def eager(model, x):
    """The network as plain torch ops on the module's own layers, the edge tensors [b, 2 C, 64, n] materialised."""
    act = model.conv7[2]
    static_nbr = x[:, 17:20].to(torch.int64).transpose(1, 2)           # [b, 64, 3]

    def edge_tensor(h, nbr):                                           # h [b, C, 64], nbr [b, 64, n]
        b, c, rows = h.shape
        n = nbr.size(2)
        centre = h[:, :, :, None].expand(b, c, rows, n)
        picked = torch.gather(centre, 2, nbr[:, None].expand(b, c, rows, n))   # h[b, c, nbr[b, r, j]]
        return torch.cat([picked - centre, centre], dim=1)

    def nearest(h):                                                    # the k rows with the smallest |h_i - h_j|^2
        gram = h.transpose(1, 2) @ h
        n2 = (h * h).sum(1)
        score = 2 * gram - n2[:, :, None] - n2[:, None, :]
        return torch.topk(score, model.k, dim=2).indices

    h, layers = x[:, :17], []
    for i in range(1, 7):
        nbr = static_nbr if i <= 3 else nearest(h)
        h = getattr(model, f"conv{i}")(edge_tensor(h, nbr)).amax(dim=3)
        layers.append(h)
    y = model.conv7(torch.cat(layers, dim=1))
    h = torch.cat([y.amax(dim=2), y.mean(dim=2)], dim=1)
    for i in range(1, 4):
        h = act(getattr(model, f"bn{7 + i}")(getattr(model, f"linear{i}")(h)))
    return model.linear4(h)


def one_pass(pc, model, fis, chunk, ws, fn):
    t = {"input": 0.0, "forward": 0.0, "unalign": 0.0}
    it = pc.iterNetworkInput(chunk, fis, "reference", np.float32, channels_first=True)
    # as predictNormals runs it: a bad index column is recorded on the device, no chunk waits for the host
    first_bad = torch.full((1,), nat.DGCNN_NO_BAD_PATCH, dtype=torch.int32, device=fn.device)
    done = 0
    while True:
        b, ms = timed(lambda: next(it, None))
        if b is None:
            break
        t["input"] += ms
        o, ms = timed(lambda: model(b.inputs, workspace=ws, first_bad=first_bad, patch_base=done))
        t["forward"] += ms
        done += b.inputs.size(0)

        def back():
            g = torch.einsum("nij,ni->nj", b.rotations, o.to(torch.float64))
            norm = torch.linalg.vector_norm(g, dim=1, keepdim=True)
            bad = (b.patch_size <= 0) | (b.centre_index < 0) | ~torch.isfinite(g).all(1) | ~(norm[:, 0] > 0)
            return torch.where(bad[:, None], fn[b.faces], g / norm)
        _, ms = timed(back)
        t["unalign"] += ms
    assert int(first_bad) == nat.DGCNN_NO_BAD_PATCH
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default=os.path.join(ROOT, "data", "stanford_bunny_mesh.npz"))
    ap.add_argument("--faces", type=int, default=0, help="number of faces (0: all), the first N")
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--emb", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--eager-repeat", type=int, default=3)
    ap.add_argument("--operands", choices=("fp32", "bf16"), default="fp32")
    a = ap.parse_args()
    dev = nat.device()
    d = np.load(a.mesh)
    v, f = np.asarray(d["v"], dtype=np.float64), np.asarray(d["f"], dtype=np.int64)
    mesh = Mesh(v, f)
    n = len(f) if a.faces <= 0 else min(a.faces, len(f))
    fis = np.arange(n)
    torch.manual_seed(0)
    model = DGCNN(a.k, 17, a.emb, 0.5, operands=a.operands)
    for name, buf in model.named_buffers():
        if name.endswith("running_var"):
            buf.uniform_(0.5, 1.5)
        elif name.endswith("running_mean"):
            buf.normal_(0.0, 0.1)
    model = model.to(dev).eval()
    pc = PatchCollector(mesh)
    chunk = min(a.chunk, n)
    ws = model.native().workspace(chunk)
    fn = mesh._geometry()[6].to(torch.float64)
    one_pass(pc, model, fis, chunk, ws, fn)                            # warm-up: code objects, caches, the topology
    runs = [one_pass(pc, model, fis, chunk, ws, fn) for _ in range(a.repeat)]
    res = {"build": nat.build_id(), "operands": a.operands, "mesh": os.path.basename(a.mesh), "faces": len(f),
           "patches": n, "chunk": chunk, "k": a.k, "emb": a.emb,
           "repeat": a.repeat, "workspace_MB": round(ws.numel() / 2 ** 20, 1)}
    for stage in ("input", "forward", "unalign"):
        ts = [r[stage] for r in runs]
        res[f"{stage}_ms_best"], res[f"{stage}_ms_median"] = round(min(ts), 3), round(statistics.median(ts), 3)
    fwd = statistics.median([r["forward"] for r in runs])
    res["forward_us_per_patch_median"] = round(1e3 * fwd / n, 3)
    res["forward_TFLOPs_median"] = round(flops_per_patch(a.emb) * n / (fwd * 1e-3) / 1e12, 2)
    res["forward_TFLOPs_best"] = round(flops_per_patch(a.emb) * n / (min(r["forward"] for r in runs) * 1e-3) / 1e12, 2)

    # the first chunk: the forward's parts through the stage entries, and the eager network
    b = next(pc.iterNetworkInput(chunk, fis[:chunk], "reference", np.float32, channels_first=True))
    x = b.inputs
    native = model.native()
    out, dbg = model(x, workspace=ws, debug=True)
    cat, cin_off = dbg["cat"], (None, 0, 64, 128, 256, 512)
    parts = {}

    def part(name, fn_):
        fn_()
        ts = [timed(fn_)[1] for _ in range(a.repeat)]
        parts[name + "_ms_best"], parts[name + "_ms_median"] = round(min(ts), 3), round(statistics.median(ts), 3)

    idx3 = x[:, 17:20].to(torch.int32).permute(0, 2, 1).contiguous()
    for layer in range(1, 7):
        xin = x[:, :17].contiguous() if layer == 1 else \
            cat[:, cin_off[layer - 1]:cin_off[layer - 1] + nat.DGCNN_CIN[layer - 1]].contiguous()
        lists = idx3 if layer <= 3 else dbg["lists"][layer - 4]
        if layer > 3:
            part(f"knn{layer}", lambda: nat.dgcnn_knn(xin, a.k))
        part(f"edgeconv{layer}", lambda: native.edgeconv(layer, xin, lists))
    w7 = model.conv7[0].weight.detach().reshape(a.emb, 1024)
    one = torch.ones(a.emb, device=dev)
    conv7 = nat.dgcnn_gemm_bf16 if a.operands == "bf16" else nat.dgcnn_gemm
    part("conv7_pool", lambda: conv7(w7, cat, nat.EPI_POOL, one, one))
    part("forward_chunk", lambda: model(x, workspace=ws))
    flag = torch.full((1,), nat.DGCNN_NO_BAD_PATCH, dtype=torch.int32, device=dev)
    part("forward_chunk_deferred", lambda: model(x, workspace=ws, first_bad=flag))
    res["chunk_parts"] = parts
    res["conv7_TFLOPs_best"] = round(2 * 1024 * a.emb * 64 * chunk / (parts["conv7_pool_ms_best"] * 1e-3) / 1e12, 2)
    with torch.no_grad():
        ref = eager(model, x)
        ts = [timed(lambda: eager(model, x))[1] for _ in range(a.eager_repeat)]
    res["eager_chunk_ms_best"], res["eager_chunk_ms_median"] = round(min(ts), 3), round(statistics.median(ts), 3)
    res["eager_over_hip_median"] = round(statistics.median(ts) / parts["forward_chunk_ms_median"], 2)
    res["eager_vs_hip_max_abs"] = float((ref - out).abs().max())
    res["eager_vs_hip_median_abs"] = float((ref - out).abs().median())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
