"""The exact NVT2 mode through the spatial slabs (`SlabDenoiser(..., exact_nvt2=True)`): one rank, and two ranks
sharing the GPU over libpcd's host-callback transport on a gloo group, against the one-GPU fused loop with
`pcd_denoiser_set_exact_nvt2` on -- bit for bit.  All NVT2 launches of the slabs go through the same stage as the fused
loop's, so the switch is one denoiser field on every rank."""
import os
import time

import numpy as np
import pytest
import torch

import pcd_native as nat
from pcd_slab import LocalTransport, SlabDenoiser, TorchTransport, gather_global
from conftest import report
from test_gpu_slab import ITERS, K, KU, _cloud, _d, _free_port

SPAWN_TIMEOUT_S = 240


def _fused_exact(pos, nrm, d):
    fd = nat.FusedDenoiser(nat.Grid(pos, k_hint=K), max(K, KU))
    fd.set_exact_nvt2(True)
    fd.load(pos, nrm)
    fd.iterate(nat.make_params(k=K, k_update=KU, d=d), ITERS)
    p, n = torch.empty_like(pos), torch.empty_like(nrm)
    fd.store(p, n)
    return p.cpu().numpy(), n.cpu().numpy()


@pytest.mark.gpu
def test_exact_slab_world1_is_the_exact_fused_loop(gpu):
    pos, nrm = _cloud(gpu)
    d = _d(pos)
    sd = SlabDenoiser(pos, nrm, max(K, KU), transport=LocalTransport(), k_hint=K, exact_nvt2=True)
    sd.iterate(nat.make_params(k=K, k_update=KU, d=d), ITERS)
    sd.check()
    p, n = gather_global(sd.owned_state(), pos.size(0), sd.t)
    rp, rn = _fused_exact(pos, nrm, d)
    np.testing.assert_array_equal(p.cpu().numpy(), rp)
    np.testing.assert_array_equal(n.cpu().numpy(), rn)
    # and the switch reached the engine: the default slab run differs in some edge-step row
    sd0 = SlabDenoiser(pos, nrm, max(K, KU), transport=LocalTransport(), k_hint=K)
    sd0.iterate(nat.make_params(k=K, k_update=KU, d=d), ITERS)
    p0, _ = gather_global(sd0.owned_state(), pos.size(0), sd0.t)
    assert (p0.cpu().numpy() != rp).any()


def _worker(rank, world, port, out_path, cloud_path, d):
    """One rank of the two-rank run (modelled on test_gpu_slab._worker): Gauss-Seidel, exact NVT2 on every rank."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pos = nrm = None
        if rank == 0:                   # only the coordinator holds the cloud
            c = np.load(cloud_path)
            pos, nrm = torch.from_numpy(c["pos"]).to(dev), torch.from_numpy(c["n"]).to(dev)
        tr = TorchTransport(rccl=False)
        sd = SlabDenoiser(pos, nrm, max(K, KU), transport=tr, k_hint=K, step_bound=d, horizon=ITERS, exact_nvt2=True)
        assert sd.comm.info() == {"world": world, "rank": rank, "transport": "host"}
        sd.iterate(nat.make_params(k=K, k_update=KU, d=d), ITERS)
        sd.check()
        p, n = gather_global(sd.owned_state(), sd.n_total, tr)
        if rank == 0:
            np.savez(out_path, pos=p.numpy(), n=n.numpy(), halo=sd.halo_points, replans=sd.replans)
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_exact_slab_world2_matches_one_gpu_bitwise(gpu, tmp_path):
    """Two spawned ranks on one GPU over the gloo host transport, 60k points, 3 Gauss-Seidel iterations, exact on: the
    gathered positions / normals are the one-GPU exact run's, bit for bit.  The spawn has a time limit, and a rank
    that exits non-zero fails the test (ProcessContext.join raises)."""
    import torch.multiprocessing as mp
    pos, nrm = _cloud(gpu)
    d = _d(pos)
    out, cloud = str(tmp_path / "slab2_exact.npz"), str(tmp_path / "cloud.npz")
    np.savez(cloud, pos=pos.cpu().numpy(), n=nrm.cpu().numpy())
    ctx = mp.spawn(_worker, args=(2, _free_port(), out, cloud, d), nprocs=2, join=False)
    deadline = time.monotonic() + SPAWN_TIMEOUT_S
    done = False
    try:
        while not done and time.monotonic() < deadline:
            done = ctx.join(timeout=5)                  # raises if a rank exited non-zero
    finally:
        if not done:
            for pr in ctx.processes:
                if pr.is_alive():
                    pr.kill()
    assert done, f"the two ranks did not finish within {SPAWN_TIMEOUT_S} s"
    res = np.load(out)
    assert int(res["halo"]) > 0
    rp, rn = _fused_exact(pos, nrm, d)
    bbox = float(np.linalg.norm(rp.max(0) - rp.min(0)))
    report(f"exact NVT2, 2 ranks vs one GPU: max |dp| / bbox {float(np.abs(res['pos'] - rp).max() / bbox):.3g}, "
           f"max |dn| {float(np.abs(res['n'] - rn).max()):.3g}, rows differing {int((res['pos'] != rp).any(1).sum())}")
    np.testing.assert_array_equal(res["pos"], rp)
    np.testing.assert_array_equal(res["n"], rn)
