#!/usr/bin/env python3
"""Time the three device stages of the network-input pipeline on a mesh (default: the Stanford bunny).

  python tools/patch_probe.py [--mesh data/stanford_bunny_mesh.npz] [--faces N] [--chunk 16384] [--dtype float32]
                              [--repeat 5] [--golden tests/golden/patch_ellipsoid.npz]

Stages, per chunk of faces, each timed with a host clock around work that ends in a device synchronise:
  radius     pcd_patch_radius (+ the libm pow round trip of pcd_native.patch_radius)
  select     pcd_patch_select_count over the grid's cells, the prefix sum, pcd_patch_select_fill
  inputs     pcd_patch_inputs: alignment, eigen-solve, 64 x 20 rows (its bytes written / its time = write bandwidth)
The first pass over the faces is a warm-up; the best and the median of --repeat passes are printed as one JSON
line, next to the reference's recorded seconds per patch (from the golden, measured on a 320-face mesh: a lower
bound on its cost here, which grows with the vertex count).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "normal-guided-pointcloud-denoiser_amd"))

import pcd_native as nat  # noqa: E402
from PatchGeneration.Modules.Mesh import Mesh  # noqa: E402


def one_pass(mesh, fis_d, k, chunk, dt):
    t = {"radius": 0.0, "select": 0.0, "inputs": 0.0}
    vd, fd, vfd, nid, tt, grid, vmax, _ = mesh._patch_state()
    rows_total = 0
    for s in range(0, fis_d.size(0), chunk):
        part = fis_d[s:s + chunk].contiguous()
        n = part.size(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        centre, r = nat.patch_radius(vd, fd, tt, part, k)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        off, rows = nat.patch_select(grid, 4e-7 * vmax, vd, fd, vfd, nid, centre, r)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out = nat.patch_inputs(vd, fd, tt, vfd, nid, part, off, rows, False, dt, False)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        t["radius"] += t1 - t0
        t["select"] += t2 - t1
        t["inputs"] += t3 - t2
        rows_total += rows.numel()
        del out
    return t, rows_total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default=os.path.join(ROOT, "data", "stanford_bunny_mesh.npz"))
    ap.add_argument("--faces", type=int, default=0, help="number of faces (0: all), the first N")
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--dtype", choices=["float32", "float64"], default="float32")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--golden", default=os.path.join(ROOT, "tests", "golden", "patch_ellipsoid.npz"))
    a = ap.parse_args()
    d = np.load(a.mesh)
    v, f = np.asarray(d["v"], dtype=np.float64), np.asarray(d["f"], dtype=np.int64)
    mesh = Mesh(v, f)
    n = len(f) if a.faces <= 0 else min(a.faces, len(f))
    fis_d = mesh._faces_arg(np.arange(n))
    dt = torch.float32 if a.dtype == "float32" else torch.float64
    one_pass(mesh, fis_d, a.k, a.chunk, dt)                       # warm-up: code objects, caches, the topology
    runs = [one_pass(mesh, fis_d, a.k, a.chunk, dt) for _ in range(a.repeat)]
    rows_total = runs[0][1]
    out_bytes = n * 64 * 20 * (4 if dt == torch.float32 else 8) + n * (72 + 8 + 24)
    res = {"mesh": os.path.basename(a.mesh), "vertices": len(v), "faces": len(f), "patches": n, "chunk": a.chunk,
           "dtype": a.dtype, "mean_patch_faces": round(rows_total / max(n, 1), 1), "repeat": a.repeat}
    for stage in ("radius", "select", "inputs"):
        ts = [r[0][stage] for r in runs]
        res[f"{stage}_ms_best"] = round(1e3 * min(ts), 3)
        res[f"{stage}_ms_median"] = round(1e3 * statistics.median(ts), 3)
    tot = [sum(r[0].values()) for r in runs]
    res["total_ms_best"] = round(1e3 * min(tot), 3)
    res["total_ms_median"] = round(1e3 * statistics.median(tot), 3)
    res["us_per_patch_median"] = round(1e6 * statistics.median(tot) / max(n, 1), 3)
    res["inputs_write_GBps_median"] = round(out_bytes / statistics.median([r[0]["inputs"] for r in runs]) / 1e9, 1)
    if os.path.exists(a.golden):
        ref = float(np.load(a.golden)["seconds_per_patch"])
        res["reference_ms_per_patch_320_faces"] = round(1e3 * ref, 3)
        res["speedup_lower_bound"] = round(ref / (statistics.median(tot) / max(n, 1)), 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
