"""The GCN-Denoiser network on the device (drop-in for DGCNN of PatchGeneration/Modules/Network/GCNModel.py):
inference, and -- for a model built with `trainable=True` -- the training step.

`DGCNN(k, init_dims, emb_dims, dropout, output_channels)` holds the same parameters and buffers under the same
state-dict keys as the reference's module, so a checkpoint it wrote loads with `load_state_dict` (strict).  `forward`
runs the hand-written HIP kernels of csrc/dgcnn.hip through pcd_native.Dgcnn: there is no eager fallback.

Layer table (all kernel size 1, no convolution bias, batch norm + LeakyReLU(0.2) after each but the last linear):
  conv1-3   edge convolutions over the input's three index columns        2x17 -> 64, 2x64 -> 64, 2x64 -> 128
  conv4-6   edge convolutions over the k nearest rows in feature space    2x128 -> 256, 2x256 -> 256, 2x256 -> 256
  conv7     over the concatenation of the six outputs                     1024 -> emb_dims, then max and mean over nodes
  linear1-4                                                               2 emb -> 512 -> 256 -> 64 -> output_channels
In eval() batch norms use their running statistics and dropout is the identity.  A default model supports eval()
only.  `DGCNN(..., trainable=True)` also runs in train(): conv1-7 and the pooling are one autograd Function on the
HIP kernels of csrc/dgcnn_train.hip (batch statistics, the arg-max bytes, the backward of the seven convolutions and
the weight-gradient GEMM), the head (linear1-4, bn8-10, dp1-2: under 1 % of the multiply-adds) runs through its torch
submodules.  Gradients reach every parameter; there is none with respect to the inputs, and the neighbour lists are
constants of the backward.  BetterDGCNN and the reference's data loaders are not part of this package; saveModel /
loadModel and the training loop are in PatchGeneration/Modules/NetworkController.py.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

import pcd_native as _nat

_EDGE = tuple(zip(_nat.DGCNN_CIN, _nat.DGCNN_COUT))   # (in, out) of conv1-6
_HEAD = (512, 256, 64)


class _Trunk(torch.autograd.Function):
    """inputs -> pooled [b, 2 emb] in train(): conv1-7 with batch statistics, max / mean pooling.  The parameters are
    the Function's inputs so that autograd hands their gradients on; the workspace carries the forward's state."""

    @staticmethod
    def forward(ctx, model, inputs, want_lists, *params):
        conv, gamma, beta = params[:7], params[7:14], params[14:21]
        bns = [getattr(model, f"bn{i}") for i in range(1, 8)]
        bn = [(g.detach(), b.detach(), m.running_mean, m.running_var, m.num_batches_tracked, m.eps, m.momentum)
              for g, b, m in zip(gamma, beta, bns)]
        conv = [c.detach() for c in conv]
        ws = torch.empty(_nat.dgcnn_train_workspace_bytes(model.k, model.emb_dims, inputs.size(0)), dtype=torch.uint8,
                         device=inputs.device)
        got = _nat.dgcnn_train_forward(conv, bn, model.k, model.emb_dims, inputs, ws, want_lists)
        pooled, lists = got if want_lists else (got, None)
        for m in bns:                                  # the kernels wrote the buffers: eval()'s packed-weight key sees it
            for buf in (m.running_mean, m.running_var, m.num_batches_tracked):
                torch.autograd.graph.increment_version(buf)
        ctx.save_for_backward(inputs, *params[:7])     # (autograd refuses a backward after an in-place change)
        ctx.ws, ctx.k, ctx.emb = ws, model.k, model.emb_dims
        ctx.set_materialize_grads(True)
        if want_lists:
            ctx.mark_non_differentiable(lists)
            return pooled, lists
        return pooled

    @staticmethod
    def backward(ctx, d_pooled, *unused):
        if ctx.ws is None:
            raise RuntimeError("DGCNN: the training workspace was consumed by an earlier backward of this forward")
        inputs, *conv = ctx.saved_tensors
        dw, dg, db = _nat.dgcnn_train_backward(conv, ctx.k, ctx.emb, inputs, d_pooled.contiguous(), ctx.ws)
        ctx.ws = None
        return (None, None, None, *dw, *dg, *db)


class DGCNN(nn.Module):
    def __init__(self, k, init_dims, emb_dims, dropout, output_channels=3, *, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
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

    @staticmethod
    def _check_inputs(inputs):
        if not isinstance(inputs, torch.Tensor) or not inputs.is_cuda:
            raise ValueError("DGCNN: inputs must be a tensor on the HIP device (there is no CPU path)")
        if inputs.dim() != 3 or inputs.size(1) != 20 or inputs.size(2) != 64:
            raise ValueError(f"DGCNN: inputs must be [b, 20, 64], got {tuple(inputs.shape)}")

    def forward(self, inputs, workspace=None, debug=False, first_bad=None, patch_base=0):
        """inputs [b, 20, 64] on the device (float64 is cast to float32) -> [b, output_channels] float32.
        workspace: an optional uint8 device tensor of at least native().workspace_bytes(b) bytes to reuse between
        calls; debug=True also returns the intermediate tensors; first_bad / patch_base: record a bad index column in
        a device flag instead of waiting for the device and raising (pcd_native.Dgcnn.forward).
        In train() (trainable=True only) the output carries a grad_fn, the batch norms use and update batch
        statistics, and only `debug` is accepted: it returns {"lists", "pooled"} (_train_forward)."""
        if self.training:
            if not self.trainable:
                raise NotImplementedError("DGCNN: only inference is implemented on the device -- call eval() first "
                                          "(or build the model with trainable=True)")
            if workspace is not None or first_bad is not None or patch_base != 0:
                raise ValueError("DGCNN: workspace / first_bad / patch_base belong to eval(); train() owns its workspace")
            return self._train_forward(inputs, debug)
        self._check_inputs(inputs)
        with torch.no_grad():
            return self._native().forward(inputs.to(torch.float32), workspace, debug, first_bad, patch_base)

    def native(self):
        """The pcd_native.Dgcnn behind forward (workspace_bytes, the stage entries)."""
        return self._native()

    # ------------------------------------------------------------------------------------------------ training
    def _train_forward(self, inputs, debug):
        """train() of a trainable model: [b, 20, 64] float32 -> [b, output_channels] with a grad_fn.  debug=True also
        returns {"lists" int32 [3, b, 64, k], "pooled" [b, 2 emb]}."""
        self._check_inputs(inputs)
        if inputs.requires_grad:
            raise ValueError("DGCNN: there is no gradient with respect to the inputs (inputs.requires_grad is set)")
        if inputs.size(0) < 1:
            raise ValueError("DGCNN: train() needs at least one patch (batch statistics)")
        conv, bns, _ = self._tensors()
        for i, bn in enumerate(bns[:7], start=1):
            if bn.momentum is None:
                raise ValueError(f"DGCNN: bn{i}.momentum=None (a cumulative average) is not supported in train()")
            if not bn.track_running_stats or bn.running_mean is None or not bn.affine:
                raise ValueError(f"DGCNN: bn{i} must be affine and track its running statistics")
        params = list(conv) + [bn.weight for bn in bns[:7]] + [bn.bias for bn in bns[:7]]
        for t in params + [b_ for bn in bns[:7] for b_ in (bn.running_mean, bn.running_var)]:
            if not t.is_cuda or t.device != inputs.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("DGCNN: train() needs float32 contiguous parameters and buffers on the inputs' device")
        x = inputs.to(torch.float32).contiguous()
        got = _Trunk.apply(self, x, bool(debug), *params)
        pooled, lists = got if debug else (got, None)
        h = pooled
        for i in (1, 2, 3):
            h = F.leaky_relu(getattr(self, f"bn{7 + i}")(getattr(self, f"linear{i}")(h)), negative_slope=0.2)
            if i < 3:
                h = getattr(self, f"dp{i}")(h)
        out = self.linear4(h)
        return (out, {"lists": lists, "pooled": pooled}) if debug else out
