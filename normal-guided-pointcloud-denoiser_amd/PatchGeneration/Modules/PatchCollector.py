"""The GCN network input on the device (drop-in for the in-memory half of PatchGeneration/Modules/PatchCollector.py).

`PatchCollector(mesh, k).collectNetworkInput(max_batch_size)` is the reference's collectNetworkInput
(PatchCollector.py:161-166): per face one patch (Mesh.selectPaperPatch), aligned (Patch.alignPatch, RotationMatrix),
turned into graph rows (Patch.toGraph) and padded / truncated to 64 rows with three index columns
(FileDataset.file2input) -- here three device stages per chunk of faces instead of a Python loop over faces:
pcd_patch_radius, the grid query + pcd_patch_select_*, pcd_patch_inputs (csrc/patch.hip).  `iterNetworkInput` yields the
chunks as device tensors, so a large mesh never holds all of its 10 KB-per-face input at once.

`predictNormals(model)` takes those chunks through the network (Network/GCNModel.py, csrc/dgcnn.hip) and back to the
mesh's frame, ready for Mesh.denoise(guided_normals=...).

The file-system half of the reference class (savePatches, .mat files, directory scanning) is not part of this
package; PatchDataset.trainingBatches hands NetworkController.NetworkTrainer its batches.  INTEGRATION.md lists where the output differs from the reference's on purpose
(boundary faces, non-manifold edges, degenerate faces, the sign of the middle axis).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

import pcd_native as _nat

from .Mesh import Mesh

ROWS, COLS = 64, 20
_NEIGHBOURS = ("reference", "adjacency")

# one chunk of iterNetworkInput, every member a device tensor: faces int64 [b], inputs [b,64,20] (or [b,20,64]),
# rotations float64 [b,3,3], centre_index int64 [b], patch_size int64 [b], radius float64 [b]
PatchBatch = namedtuple("PatchBatch", "faces inputs rotations centre_index patch_size radius")


def _torch_dtype(dtype):
    if dtype in (torch.float64, torch.float32):
        return dtype
    dt = np.dtype(dtype)
    if dt == np.float64:
        return torch.float64
    if dt == np.float32:
        return torch.float32
    raise ValueError(f"PatchCollector: dtype must be float64 or float32, got {dtype!r}")


class PatchDataset(torch.utils.data.Dataset):
    """The reference's PatchDataset (Network/DataUtils.py:100-142) plus what only the device pipeline knows.

    data_patch      [n, 64, 20] network rows: centroid 3, normal 3, area, edge-neighbours in the patch, corners 9,
                    index columns 3; the first 64 faces of the patch in face-index order, zero-padded
    data_rotations  [n, 3, 3] the alignment applied (Patch.lastRotationApplied)
    centre_index    [n] the row of the patch's own face; >= 64 when it fell outside the window, -1 if it is not in
                    its patch at all (a degenerate face)
    patch_size      [n] faces in the whole patch (before the window)
    radius          [n] the selection radius
    status          {"degenerate_faces": zero-area faces in the mesh, "centre_outside_window": patches whose own face
                    is not among the 64 rows, "centre_missing": patches that do not hold their own face}
    batch_size      getPreferredBatchSize(n, max_batch_size), as the reference's
    """

    def __init__(self, data_patch, data_rotations, max_batch_size, num_workers=8, centre_index=None, patch_size=None,
                 radius=None, status=None):
        if type(data_patch) != np.ndarray or len(data_patch.shape) != 3:
            raise ValueError(f"data_patch is not a valid 3-dimensional ndarray! Currently it is {data_patch}")
        if type(data_rotations) != np.ndarray or len(data_rotations.shape) != 3:
            raise ValueError(f"data_rotations is not a valid 3-dimensional ndarray! Currently it is {data_rotations}")
        if data_patch.shape[0] != data_rotations.shape[0]:
            raise ValueError("data_patch and data_rotations do not have the same amount of patches that they represent! "
                             f"Currently it is:\npatches: {data_patch.shape[0]}\nrotations: {data_rotations.shape[0]}")
        if not isinstance(max_batch_size, int) or max_batch_size < 1:
            raise ValueError(f"max_batch_size should be an integer bigger than zero. Currently it is {max_batch_size}")
        super().__init__()
        n = len(data_patch)
        self.batch_size = self.getPreferredBatchSize(n, max_batch_size) if n else 0
        self.num_workers = num_workers
        self.data_patch = data_patch
        self.data_rotations = data_rotations
        self.centre_index = centre_index
        self.patch_size = patch_size
        self.radius = radius
        self.status = status if status is not None else {}
        self.SIZE = n

    def __len__(self):
        return self.SIZE

    def __getitem__(self, index):
        return self.data_patch[index]

    @classmethod
    def getPreferredBatchSize(cls, n, m):
        """The largest factor of n below m (DataUtils.py:130-138, its strict `<` kept)."""
        if not isinstance(n, int) or not isinstance(m, int):
            raise ValueError(f"n and m should be integers to calculate preferred batch size.\nm = {m}\nn = {n}")
        r = np.arange(1, int(n ** 0.5) + 1)
        f = n % r == 0
        factors = np.append(r[f], np.flip(n / r[f]))
        return int(np.max(factors[factors < m]))

    def getDataloader(self):
        return torch.utils.data.DataLoader(dataset=self, batch_size=self.batch_size, shuffle=False,
                                           num_workers=self.num_workers, pin_memory=True, drop_last=True)

    def unalign(self, outputs):
        """R^T o per patch: the inverse of the alignment that was applied (the rows of R are the patch's axes, so
        aligned = R x), which takes a normal predicted in the aligned frame back to the mesh's frame, ready for
        Mesh.denoise(guided_normals=...).  Note that the reference's NetworkController.py:257 computes R o instead."""
        o = np.asarray(outputs, dtype=np.float64)
        if o.shape != (self.SIZE, 3):
            raise ValueError(f"PatchDataset: outputs must have shape ({self.SIZE}, 3), got {o.shape}")
        return np.einsum("nij,ni->nj", self.data_rotations, o)

    def trainingBatches(self, gt_normals, device=None, aligned=False, batch_size=None):
        """The batches NetworkController.NetworkTrainer takes: a list of (inputs [b, 64, 20] float32, gt [b, 3]
        float32) device tensors, batch_size patches each (default self.batch_size; a short last batch is dropped, as
        the reference's loaders drop it).  gt_normals [n, 3] are the ground-truth normals of the patches' faces in
        the mesh's frame -- each is taken into its patch's aligned frame with R n, the inverse of unalign -- or, with
        aligned=True, already in the aligned frame.  Rows and normals are uploaded once; every batch is a view of
        that one device copy, so an epoch over the list moves nothing between host and device."""
        dev = _nat.device() if device is None else torch.device(device)
        gt = np.asarray(gt_normals, dtype=np.float64)
        if gt.shape != (self.SIZE, 3):
            raise ValueError(f"PatchDataset: gt_normals must have shape ({self.SIZE}, 3), got {gt.shape}")
        if not aligned:
            gt = np.einsum("nij,nj->ni", self.data_rotations, gt)
        bs = int(self.batch_size if batch_size is None else batch_size)
        if bs < 1:
            raise ValueError(f"PatchDataset: batch_size must be at least 1, got {bs}")
        x = torch.as_tensor(self.data_patch).to(dev, torch.float32)
        g = torch.as_tensor(gt).to(dev, torch.float32)
        return [(x[s:s + bs], g[s:s + bs]) for s in range(0, self.SIZE - bs + 1, bs)]


class PatchCollector:
    CHUNK = 16384     # faces per device pass of collectNetworkInput (160 MB of float64 rows)

    def __init__(self, mesh, k=4):
        if not isinstance(mesh, Mesh) or not isinstance(k, int):
            raise ValueError("mesh should be a Mesh and k should be an int")
        self.k = k
        self.mesh = mesh

    def _batch(self, state, fis_d, adjacency, dtype, channels_first):
        _, r, off, rows = self.mesh._patches(fis_d, self.k, state=state)
        vd, fd, vfd, nid, tt = state[:5]
        inputs, rot, ci, _ = _nat.patch_inputs(vd, fd, tt, vfd, nid, fis_d, off, rows, adjacency, dtype, channels_first)
        return PatchBatch(fis_d, inputs, rot, ci, off[1:] - off[:-1], r)

    def iterNetworkInput(self, batch_faces, faces=None, neighbours="reference", dtype=np.float64,
                         channels_first=False):
        """Yield the network input of `faces` (None: every face, in order) in chunks of batch_faces faces as
        PatchBatch tuples of device tensors: inputs [b, 64, 20], or [b, 20, 64] with channels_first (the layout the
        model takes).  Every chunk is bitwise the corresponding rows of one full run."""
        if not isinstance(batch_faces, (int, np.integer)) or batch_faces < 1:
            raise ValueError(f"batch_faces should be an integer bigger than zero. Currently it is {batch_faces}")
        if neighbours not in _NEIGHBOURS:
            raise ValueError(f"PatchCollector: unknown neighbours mode {neighbours!r} {_NEIGHBOURS}")
        dt = _torch_dtype(dtype)
        fis_d = self.mesh._faces_arg(faces)
        state = self.mesh._patch_state()                # (the mesh as it is now: one check for all chunks)
        for s in range(0, fis_d.size(0), int(batch_faces)):
            yield self._batch(state, fis_d[s:s + int(batch_faces)].contiguous(), neighbours == "adjacency", dt,
                              bool(channels_first))

    def predictNormals(self, model, batch_faces=4096, faces=None, neighbours="reference"):
        """The network's normal of `faces` (None: every face) in the mesh's frame, ready for
        Mesh.denoise(guided_normals=...): (normals float64 [n, 3] on the device, number of fallbacks).

        Chunks of batch_faces patches go from iterNetworkInput (float32, channels first) through `model` (a
        Network.GCNModel.DGCNN or BetterDGCNN in eval(), on the device) with one workspace for all of them, sized by
        the model's own layer table (model.native().workspace); each output o is taken
        back with R^T o (PatchDataset.unalign's convention; the reference's NetworkController.py:257 computes R o) and
        normalised.  A face keeps its own normal -- and is counted -- where its patch is empty, does not hold the
        face (centre_index < 0), or the output is zero or not finite."""
        fn = self.mesh._geometry()[6].to(torch.float64)
        parts, fallbacks, ws, done = [], 0, None, 0
        # a bad index column is recorded on the device and read once, after the last chunk: no chunk waits for it
        first_bad = torch.full((1,), _nat.DGCNN_NO_BAD_PATCH, dtype=torch.int32, device=fn.device)
        for b in self.iterNetworkInput(batch_faces, faces, neighbours, np.float32, channels_first=True):
            if ws is None:                              # (the first chunk is the largest)
                ws = model.native().workspace(b.inputs.size(0))
            o = model(b.inputs, workspace=ws, first_bad=first_bad, patch_base=done).to(torch.float64)
            done += b.inputs.size(0)
            g = torch.einsum("nij,ni->nj", b.rotations.to(torch.float64), o)
            norm = torch.linalg.vector_norm(g, dim=1, keepdim=True)
            bad = (b.patch_size <= 0) | (b.centre_index < 0) | ~torch.isfinite(g).all(1) | ~(norm[:, 0] > 0)
            parts.append(torch.where(bad[:, None], fn[b.faces], g / norm))
            fallbacks += int(bad.sum())
        if not parts:
            return torch.zeros((0, 3), dtype=torch.float64, device=fn.device), 0
        bad_patch = int(first_bad)
        if bad_patch != _nat.DGCNN_NO_BAD_PATCH:
            raise ValueError(f"PatchCollector: patch {bad_patch} of the request has an index column outside [0, 63]")
        return torch.cat(parts), fallbacks

    def collectNetworkInput(self, max_batch_size, faces=None, neighbours="reference", dtype=np.float64):
        """PatchCollector.collectNetworkInput (PatchCollector.py:161-166) for `faces` (None: all): a PatchDataset of
        host arrays.  neighbours: "reference" reproduces the index columns the reference's networks were trained on,
        "adjacency" gives the local edge-neighbours."""
        ndt = np.float32 if _torch_dtype(dtype) == torch.float32 else np.float64
        parts = [[np.zeros((0, ROWS, COLS), ndt)], [np.zeros((0, 3, 3))], [np.zeros(0, np.int64)],
                 [np.zeros(0, np.int64)], [np.zeros(0)]]
        for b in self.iterNetworkInput(self.CHUNK, faces, neighbours, dtype):
            for dst, t in zip(parts, b[1:]):
                dst.append(t.cpu().numpy())
        data, rot, ci, size, r = (np.concatenate(p) for p in parts)
        status = {"degenerate_faces": self.mesh._patch_state()[7] if len(self.mesh.f) else 0,
                  "centre_outside_window": int((ci >= ROWS).sum()), "centre_missing": int((ci < 0).sum())}
        return PatchDataset(data, rot, max_batch_size, centre_index=ci, patch_size=size, radius=r, status=status)
