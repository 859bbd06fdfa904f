"""The GCN-Denoiser network's forward pass on the device (drop-in for DGCNN of PatchGeneration/Modules/Network/
GCNModel.py, inference only).

`DGCNN(k, init_dims, emb_dims, dropout, output_channels)` holds the same parameters and buffers under the same
state-dict keys as the reference's module, so a checkpoint it wrote loads with `load_state_dict` (strict).  `forward`
runs the hand-written HIP kernels of csrc/dgcnn.hip through pcd_native.Dgcnn: there is no eager fallback.

Layer table (all kernel size 1, no convolution bias, batch norm + LeakyReLU(0.2) after each but the last linear):
  conv1-3   edge convolutions over the input's three index columns        2x17 -> 64, 2x64 -> 64, 2x64 -> 128
  conv4-6   edge convolutions over the k nearest rows in feature space    2x128 -> 256, 2x256 -> 256, 2x256 -> 256
  conv7     over the concatenation of the six outputs                     1024 -> emb_dims, then max and mean over nodes
  linear1-4                                                               2 emb -> 512 -> 256 -> 64 -> output_channels
Only eval() is supported: batch norms use their running statistics, dropout is the identity.  Training, backward,
BetterDGCNN and the reference's file-system half (saveModel, data loaders) are not part of this package.
"""
from __future__ import annotations

import torch
import torch.nn as nn

import pcd_native as _nat

_EDGE = ((17, 64), (64, 64), (64, 128), (128, 256), (256, 256), (256, 256))   # (in, out) of conv1-6
_HEAD = (512, 256, 64)


class DGCNN(nn.Module):
    def __init__(self, k, init_dims, emb_dims, dropout, output_channels=3):
        super().__init__()
        if int(init_dims) != 17:
            raise ValueError(f"DGCNN: init_dims must be 17 (forward takes rows 0:17 of its input), got {init_dims}")
        if not 1 <= int(k) <= 64:
            raise ValueError(f"DGCNN: k must be in [1, 64], got {k}")
        self.k = int(k)
        self.init_dims, self.emb_dims, self.output_channels = int(init_dims), int(emb_dims), int(output_channels)
        act = lambda: nn.LeakyReLU(negative_slope=0.2)
        # bnN is registered on its own AND as convN.1: both names are in the state dict, one tensor behind them
        for i, (cin, cout) in enumerate(_EDGE, start=1):
            bn = nn.BatchNorm2d(cout)
            setattr(self, f"bn{i}", bn)
            setattr(self, f"conv{i}", nn.Sequential(nn.Conv2d(2 * cin, cout, kernel_size=1, bias=False), bn, act()))
        self.bn7 = nn.BatchNorm1d(self.emb_dims)
        self.conv7 = nn.Sequential(nn.Conv1d(1024, self.emb_dims, kernel_size=1, bias=False), self.bn7, act())
        width = 2 * self.emb_dims
        for i, out in enumerate(_HEAD, start=1):
            setattr(self, f"linear{i}", nn.Linear(width, out, bias=i > 1))
            setattr(self, f"bn{7 + i}", nn.BatchNorm1d(out))
            if i < 3:
                setattr(self, f"dp{i}", nn.Dropout(p=dropout))
            width = out
        self.linear4 = nn.Linear(width, self.output_channels)
        self._packed = None          # (key, pcd_native.Dgcnn)
        self._workspace = None

    # ------------------------------------------------------------------------------------- packed device weights
    def _tensors(self):
        conv = [getattr(self, f"conv{i}")[0].weight for i in range(1, 8)]
        bns = [getattr(self, f"bn{i}") for i in range(1, 11)]
        lin = [getattr(self, f"linear{i}") for i in range(1, 5)]
        return conv, bns, lin

    def _native(self):
        """The packed weights, rebuilt when a parameter or buffer was replaced, moved or written in place."""
        conv, bns, lin = self._tensors()
        flat = list(conv)
        for bn in bns:
            flat += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        for l in lin:
            flat += [l.weight] + ([l.bias] if l.bias is not None else [])
        key = tuple((t.data_ptr(), t._version, str(t.device), t.dtype) for t in flat) + \
            tuple(float(bn.eps) for bn in bns)
        if self._packed is None or self._packed[0] != key:
            native = _nat.Dgcnn(conv, [(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps) for bn in bns],
                                [(l.weight, l.bias) for l in lin], self.k, self.init_dims, self.emb_dims,
                                self.output_channels)
            self._packed = (key, native)
        return self._packed[1]

    def forward(self, inputs, workspace=None, debug=False, first_bad=None, patch_base=0):
        """inputs [b, 20, 64] on the device (float64 is cast to float32) -> [b, output_channels] float32.
        workspace: an optional uint8 device tensor of at least native().workspace_bytes(b) bytes to reuse between
        calls; debug=True also returns the intermediate tensors; first_bad / patch_base: record a bad index column in
        a device flag instead of waiting for the device and raising (pcd_native.Dgcnn.forward)."""
        if self.training:
            raise NotImplementedError("DGCNN: only inference is implemented on the device -- call eval() first")
        if not isinstance(inputs, torch.Tensor) or not inputs.is_cuda:
            raise ValueError("DGCNN: inputs must be a tensor on the HIP device (there is no CPU path)")
        if inputs.dim() != 3 or inputs.size(1) != 20 or inputs.size(2) != 64:
            raise ValueError(f"DGCNN: inputs must be [b, 20, 64], got {tuple(inputs.shape)}")
        with torch.no_grad():
            return self._native().forward(inputs.to(torch.float32), workspace, debug, first_bad, patch_base)

    def native(self):
        """The pcd_native.Dgcnn behind forward (workspace_bytes, the stage entries)."""
        return self._native()
