"""Timing of Mesh.denoise's loop (DESIGN.md §3 "Guided bilateral normal filtering of meshes"; informational).

HIP events around pcd_mesh_denoise(_f32) on the noisy bunny mesh and on a noisy n x n grid mesh (default 1001: 2.0M
faces): milliseconds per normal iteration for the filter step alone (face geometry, sigma_s, one pass) and with its 16
vertex sweeps, fp64 and fp32 alternating within every repetition; the one-time neighbourhood build (host clock around
the synchronising call); and the numpy restatement (tests/mesh_filter_ref.py) on the bunny.  Prints one JSON line per
mesh; --out FILE also writes them all.

    python tools/mesh_denoise_probe.py [--grid 1001] [--reps 5] [--no-numpy] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "normal-guided-pointcloud-denoiser_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import mesh_filter_ref as R  # noqa: E402
import pcd_native as nat  # noqa: E402
from PatchGeneration.Modules.Mesh import Mesh  # noqa: E402


def grid_mesh(n, noise=0.1, seed=1):
    """mesh_filter_ref.grid(n, n, noise) without the Python loop over the cells."""
    xs, ys = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    v = np.stack([xs.ravel(), ys.ravel(), np.zeros(n * n)], 1)
    v += np.random.default_rng(seed).uniform(-noise, noise, v.shape)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a, b, c, d = (i * n + j).ravel(), ((i + 1) * n + j).ravel(), ((i + 1) * n + j + 1).ravel(), (i * n + j + 1).ravel()
    return v, np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3).astype(np.int64)


def measure(v, f, iterations, reps):
    dev = nat.device()
    res = {"faces": int(len(f)), "vertices": int(len(v))}
    mesh = Mesh(v.copy(), f.copy())
    for first in (True, False):
        mesh.f = mesh.f                                        # drops the cached topology and neighbourhoods
        mesh._topology(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        off, nbr, extra = mesh._neighbourhoods("radius", 2, None)
        torch.cuda.synchronize()
        res["neighbourhood_build_ms" + ("_first" if first else "")] = (time.perf_counter() - t0) * 1e3
    res["row_mean"] = nbr.numel() / len(f)
    off32, nbr32 = Mesh._csr32(off, nbr, extra)
    keys = [(fp32, vi) for fp32 in (False, True) for vi in (0, 16)]
    samples = {k: [] for k in keys}
    for rep in range(reps + 1):                                # the first repetition warms every shape up
        for fp32, vi in keys:
            fd, vfd, nid = mesh._topology(fp32)
            vd = torch.from_numpy(v).to(dev).to(torch.float32 if fp32 else torch.float64).contiguous()
            o, n = (off32, nbr32) if fp32 else (off, nbr)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            nat.mesh_denoise(vd, fd, vfd, nid, o, n, None, iterations, vi, 0.3, 1.0)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                samples[(fp32, vi)].append(e0.elapsed_time(e1) / iterations)
    for (fp32, vi), ts in samples.items():
        res[f"{'fp32' if fp32 else 'fp64'}_{'with_16_sweeps' if vi else 'filter_step'}_ms"] = {
            "median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1001)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {}
    d = np.load(os.path.join(ROOT, "data", "stanford_bunny_mesh.npz"))
    bf = d["f"].astype(np.int64)
    bv = R.gaussian_noise(d["v"].astype(np.float64), bf, 0.2)
    out["bunny"] = measure(bv, bf, 12, a.reps)
    print("bunny", json.dumps(out["bunny"]), flush=True)
    out["grid"] = measure(*grid_mesh(a.grid), 4, a.reps)
    print("grid", json.dumps(out["grid"]), flush=True)
    if not a.no_numpy:
        t0 = time.perf_counter()
        csr = R.default_neighbourhoods(bv, bf)[:2]
        t1 = time.perf_counter()
        R.denoise(bv, bf, None, 2, 16, csr=csr)
        t2 = time.perf_counter()
        R.denoise(bv, bf, None, 2, 0, csr=csr)
        t3 = time.perf_counter()
        out["bunny_numpy"] = {"neighbourhood_build_ms": (t1 - t0) * 1e3, "with_16_sweeps_ms": (t2 - t1) * 500,
                              "filter_step_ms": (t3 - t2) * 500}
        print("bunny_numpy", json.dumps(out["bunny_numpy"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
