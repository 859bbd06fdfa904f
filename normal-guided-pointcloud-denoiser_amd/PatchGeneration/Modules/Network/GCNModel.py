"""The GCN-Denoiser networks on the device (drop-ins for DGCNN and BetterDGCNN of
PatchGeneration/Modules/Network/GCNModel.py): inference, and -- for a model built with `trainable=True` -- the
training step.

`DGCNN(k, init_dims, emb_dims, dropout, output_channels)` and `BetterDGCNN(l_e, l_d, l_l, channel_sizes, k, init_dims,
dropout, output_channels)` hold the same parameters and buffers under the same state-dict keys as the reference's
modules, so a checkpoint it wrote loads with `load_state_dict` (strict), and the other way round.  `forward` runs the
hand-written HIP kernels of csrc/dgcnn.hip through pcd_native.Dgcnn / BetterDgcnn: there is no eager fallback.

Both are one layer table (pcd_native.DgcnnTable; all kernel size 1, no convolution bias, batch norm + LeakyReLU after
each layer but the last linear):
  conv 1 .. l_e             edge convolutions over the input's three index columns   2 C_{i-1} -> C_i,  C_0 = 17
  conv l_e+1 .. l_e+l_d     edge convolutions over the k nearest rows in feature space (with l_e = 0 the first search
                            runs on rows 0:17 of the input, and the index columns are never read)
  conv l_e+l_d+1            over the concatenation of those outputs                  Ccat -> C, then max and mean over nodes
  linear 1 .. l_l                                                                    2 C -> ... -> output_channels
DGCNN is the table 3, 3, 4, [64, 64, 128, 256, 256, 256, emb_dims, 512, 256, 64].  The convolutions' LeakyReLU slope
is 0.2 in both; the head's is 0.2 in DGCNN and 0.01 in BetterDGCNN, whose forward calls F.leaky_relu without a slope
(GCNModel.py:291 of the reference).
In eval() batch norms use their running statistics and dropout is the identity.  A default model supports eval()
only.  `trainable=True` also runs in train(): the convolutions and the pooling are one autograd Function on the HIP
kernels of csrc/dgcnn_train.hip (batch statistics, the arg-max bytes, the backward of the convolutions and the
weight-gradient GEMM), the head (the linears, their batch norms and dropouts: under 1 % of DGCNN's multiply-adds) runs
through its torch submodules -- in BetterDGCNN the batch norms on float64 views of their tensors (_batch_norm_wide).
Gradients reach every parameter; there is none with respect to the inputs, and the neighbour lists are constants of the
backward.  The reference's data loaders are not part of this package; saveModel /
loadModel and the training loop are in PatchGeneration/Modules/NetworkController.py.

`operands="bf16"` (constructor keyword, or `model.set_operands("bf16")`; the default is "fp32") is an opt-in inference
mode: the convolutions' GEMMs -- every edge layer with at least 32 input channels and the pooled convolution -- take
their operands rounded to bf16 and accumulate in float32 (include/pcd.h, "bf16 operands").  Faster and less precise;
a patch's output still depends on that patch alone, bit for bit.  The setting is no part of the state dict, survives
load_state_dict / .to / in-place writes, and train() ignores it.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

import pcd_native as _nat


class _Trunk(torch.autograd.Function):
    """inputs -> pooled [b, 2 C] in train(): the convolutions with batch statistics, max / mean pooling.  The
    parameters are the Function's inputs so that autograd hands their gradients on; the workspace carries the
    forward's state."""

    @staticmethod
    def forward(ctx, model, inputs, want_lists, *params):
        n = model.table.n_edge + 1
        conv, gamma, beta = params[:n], params[n:2 * n], params[2 * n:3 * n]
        bns = [getattr(model, f"bn{i}") for i in range(1, n + 1)]
        bn = [(g.detach(), b.detach(), m.running_mean, m.running_var, m.num_batches_tracked, m.eps, m.momentum)
              for g, b, m in zip(gamma, beta, bns)]
        conv = [c.detach() for c in conv]
        ws = torch.empty(model._train_workspace_bytes(inputs.size(0)), dtype=torch.uint8, device=inputs.device)
        got = model._train_trunk_forward(conv, bn, inputs, ws, want_lists)
        pooled, lists = got if want_lists else (got, None)
        for m in bns:                                  # the kernels wrote the buffers: eval()'s packed-weight key sees it
            for buf in (m.running_mean, m.running_var, m.num_batches_tracked):
                torch.autograd.graph.increment_version(buf)
        ctx.save_for_backward(inputs, *params[:n])     # (autograd refuses a backward after an in-place change)
        ctx.ws, ctx.model = ws, model
        ctx.set_materialize_grads(True)
        if want_lists:
            ctx.mark_non_differentiable(lists)
            return pooled, lists
        return pooled

    @staticmethod
    def backward(ctx, d_pooled, *unused):
        if ctx.ws is None:
            raise RuntimeError(f"{type(ctx.model).__name__}: the training workspace was consumed by an earlier backward "
                               "of this forward")
        inputs, *conv = ctx.saved_tensors
        dw, dg, db = ctx.model._train_trunk_backward(conv, inputs, d_pooled.contiguous(), ctx.ws)
        ctx.ws = None
        return (None, None, None, *dw, *dg, *db)


def _batch_norm_wide(bn, y):
    """bn(y) in train(): the module's own forward, run on float64 views of its parameters, buffers and input, the
    result back in y's dtype.  As the trunk's kernels form their batch statistics in double: a batch norm over a few
    samples multiplies rounding by up to 1 / sigma^3 in its backward (sigma^2 >= eps = 1e-5), which float32
    accumulators hand on to every gradient below it -- at b = 2 the gradient of a hidden linear's bias, zero in exact
    arithmetic, came out as 1.9e-6 in float32 (the reference's CPU run, whose batch norm accumulates in double, leaves
    6.8e-8) and comes out as exactly 0 this way.  Costs 0.15 ms a step in small launches.  Semantics (momentum, the
    unbiased running variance, num_batches_tracked, the error at b = 1) stay the module's."""
    wide = {key: v.double() if v.is_floating_point() else v
            for key, v in list(bn.named_parameters()) + list(bn.named_buffers())}
    z = torch.func.functional_call(bn, wide, (y.double(),))
    with torch.no_grad():
        for key, buf in bn.named_buffers():
            if buf.is_floating_point():                # (num_batches_tracked was counted in place)
                buf.copy_(wide[key])
    return z.to(y.dtype)


class _TableNet(nn.Module):
    """What DGCNN and BetterDGCNN share: the submodules of a layer table under the reference's names, the packed
    device weights, forward in eval() and train()."""
    _HEAD_SLOPE = 0.2
    _HEAD_BN_WIDE = False            # train(): the head's batch norms on float64 views (_batch_norm_wide)

    def _build(self, table, dropout, trainable, operands="fp32"):
        _nat.operands_code(operands, type(self).__name__)
        self.operands = operands
        self.trainable = bool(trainable)
        self.table = table
        self.k, self.init_dims, self.output_channels = table.k, table.init_dims, table.output_channels
        act = lambda: nn.LeakyReLU(negative_slope=0.2)
        E = table.n_edge
        # bnN is registered on its own AND as convN.1: both names are in the state dict, one tensor behind them
        for i, (cin, cout) in enumerate(zip(table.cin, table.cout), start=1):
            bn = nn.BatchNorm2d(cout)
            setattr(self, f"bn{i}", bn)
            setattr(self, f"conv{i}", nn.Sequential(nn.Conv2d(2 * cin, cout, kernel_size=1, bias=False), bn, act()))
        bn = nn.BatchNorm1d(table.emb)
        setattr(self, f"bn{E + 1}", bn)
        setattr(self, f"conv{E + 1}", nn.Sequential(nn.Conv1d(table.ccat, table.emb, kernel_size=1, bias=False), bn, act()))
        width = 2 * table.emb
        for i, out in enumerate(table.head, start=1):
            setattr(self, f"linear{i}", nn.Linear(width, out, bias=i > 1))
            setattr(self, f"bn{E + 1 + i}", nn.BatchNorm1d(out))
            if i < len(table.head):
                setattr(self, f"dp{i}", nn.Dropout(p=dropout))
            width = out
        setattr(self, f"linear{table.l_l}", nn.Linear(width, self.output_channels))
        self._packed = None          # (key, pcd_native.Dgcnn)
        self._workspace = None

    # ------------------------------------------------------------------------------------- packed device weights
    def _tensors(self):
        t = self.table
        conv = [getattr(self, f"conv{i}")[0].weight for i in range(1, t.n_edge + 2)]
        bns = [getattr(self, f"bn{i}") for i in range(1, t.n_edge + t.l_l + 1)]
        lin = [getattr(self, f"linear{i}") for i in range(1, t.l_l + 1)]
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
            native = self._pack(conv, [(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps) for bn in bns],
                                [(l.weight, l.bias) for l in lin])
            if self.operands != "fp32":
                native.set_operands(self.operands)
            self._packed = (key, native)
        return self._packed[1]

    def set_operands(self, operands):
        """"bf16": eval() runs the convolutions' GEMMs on bf16 operands with float32 accumulation; "fp32": the default.
        Anything else is a ValueError.  train() is float32 whatever this says."""
        _nat.operands_code(operands, type(self).__name__)
        self.operands = operands
        if self._packed is not None:
            self._packed[1].set_operands(operands)
        return self

    def _check_inputs(self, inputs):
        name = type(self).__name__
        if not isinstance(inputs, torch.Tensor) or not inputs.is_cuda:
            raise ValueError(f"{name}: inputs must be a tensor on the HIP device (there is no CPU path)")
        if inputs.dim() != 3 or inputs.size(1) != 20 or inputs.size(2) != 64:
            raise ValueError(f"{name}: inputs must be [b, 20, 64], got {tuple(inputs.shape)}")

    def forward(self, inputs, workspace=None, debug=False, first_bad=None, patch_base=0):
        """inputs [b, 20, 64] on the device (float64 is cast to float32) -> [b, output_channels] float32.
        workspace: an optional uint8 device tensor of at least native().workspace_bytes(b) bytes to reuse between
        calls; debug=True also returns the intermediate tensors; first_bad / patch_base: record a bad index column in
        a device flag instead of waiting for the device and raising (pcd_native.Dgcnn.forward).
        In train() (trainable=True only) the output carries a grad_fn, the batch norms use and update batch
        statistics, and only `debug` is accepted: it returns {"lists", "pooled"} (_train_forward)."""
        name = type(self).__name__
        if self.training:
            if not self.trainable:
                raise NotImplementedError(f"{name}: only inference is implemented on the device -- call eval() first "
                                          "(or build the model with trainable=True)")
            if workspace is not None or first_bad is not None or patch_base != 0:
                raise ValueError(f"{name}: workspace / first_bad / patch_base belong to eval(); train() owns its workspace")
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
        returns {"lists" int32 [l_d, b, 64, k], "pooled" [b, 2 C]}."""
        name = type(self).__name__
        self._check_inputs(inputs)
        if inputs.requires_grad:
            raise ValueError(f"{name}: there is no gradient with respect to the inputs (inputs.requires_grad is set)")
        if inputs.size(0) < 1:
            raise ValueError(f"{name}: train() needs at least one patch (batch statistics)")
        n = self.table.n_edge + 1                      # the convolutions: the trunk
        conv, bns, _ = self._tensors()
        for i, bn in enumerate(bns[:n], start=1):
            if bn.momentum is None:
                raise ValueError(f"{name}: bn{i}.momentum=None (a cumulative average) is not supported in train()")
            if not bn.track_running_stats or bn.running_mean is None or not bn.affine:
                raise ValueError(f"{name}: bn{i} must be affine and track its running statistics")
        params = list(conv) + [bn.weight for bn in bns[:n]] + [bn.bias for bn in bns[:n]]
        for t in params + [b_ for bn in bns[:n] for b_ in (bn.running_mean, bn.running_var)]:
            if not t.is_cuda or t.device != inputs.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{name}: train() needs float32 contiguous parameters and buffers on the inputs' device")
        x = inputs.to(torch.float32).contiguous()
        got = _Trunk.apply(self, x, bool(debug), *params)
        pooled, lists = got if debug else (got, None)
        h = pooled
        hidden = len(self.table.head)
        for i in range(1, hidden + 1):
            bn, y = getattr(self, f"bn{n + i}"), getattr(self, f"linear{i}")(h)
            h = F.leaky_relu(_batch_norm_wide(bn, y) if self._HEAD_BN_WIDE else bn(y), negative_slope=self._HEAD_SLOPE)
            if i < hidden:
                h = getattr(self, f"dp{i}")(h)
        out = getattr(self, f"linear{hidden + 1}")(h)
        return (out, {"lists": lists, "pooled": pooled}) if debug else out


class DGCNN(_TableNet):
    def __init__(self, k, init_dims, emb_dims, dropout, output_channels=3, *, trainable=False, operands="fp32"):
        super().__init__()
        if int(init_dims) != 17:
            raise ValueError(f"DGCNN: init_dims must be 17 (forward takes rows 0:17 of its input), got {init_dims}")
        if not 1 <= int(k) <= 64:
            raise ValueError(f"DGCNN: k must be in [1, 64], got {k}")
        self.emb_dims = int(emb_dims)
        self._build(_nat.DgcnnTable.fixed(k, emb_dims, output_channels), dropout, trainable, operands)

    def _pack(self, conv, bn, lin):
        return _nat.Dgcnn(conv, bn, lin, self.k, self.init_dims, self.emb_dims, self.output_channels)

    def _train_workspace_bytes(self, b):
        return _nat.dgcnn_train_workspace_bytes(self.k, self.emb_dims, b)

    def _train_trunk_forward(self, conv, bn, inputs, ws, want_lists):
        return _nat.dgcnn_train_forward(conv, bn, self.k, self.emb_dims, inputs, ws, want_lists)

    def _train_trunk_backward(self, conv, inputs, d_pooled, ws):
        return _nat.dgcnn_train_backward(conv, self.k, self.emb_dims, inputs, d_pooled, ws)


class BetterDGCNN(_TableNet):
    """BetterDGCNN of the reference (GCNModel.py:217-297).  channel_sizes: a 1-D integer tensor (the reference needs
    one) or a sequence of ints, l_e + l_d + l_l of them.  Keeps the reference's attributes l_e, l_d, l_l,
    channel_sizes and cum_sizes."""
    _HEAD_SLOPE = 0.01               # F.leaky_relu's default: GCNModel.py:291 passes no slope
    _HEAD_BN_WIDE = True             # (DGCNN keeps its float32 head: its train() bits are the earlier ones)

    def __init__(self, l_e, l_d, l_l, channel_sizes, k, init_dims, dropout, output_channels=3, *, trainable=False,
                 operands="fp32"):
        super().__init__()
        table = _nat.DgcnnTable(l_e, l_d, l_l, channel_sizes, k, init_dims, output_channels)
        self.l_e, self.l_d, self.l_l = table.l_e, table.l_d, table.l_l
        self.channel_sizes = channel_sizes if isinstance(channel_sizes, torch.Tensor) else \
            torch.tensor(table.sizes, dtype=torch.int64)
        self.cum_sizes = F.pad(torch.cumsum(self.channel_sizes, 0), (1, 0), "constant", value=0)
        self.emb_dims = table.emb
        self._build(table, dropout, trainable, operands)

    def _pack(self, conv, bn, lin):
        return _nat.BetterDgcnn(self.table, conv, bn, lin)

    def _train_workspace_bytes(self, b):
        return _nat.bdgcnn_train_workspace_bytes(self.table, b)

    def _train_trunk_forward(self, conv, bn, inputs, ws, want_lists):
        return _nat.bdgcnn_train_forward(self.table, conv, bn, inputs, ws, want_lists)

    def _train_trunk_backward(self, conv, inputs, d_pooled, ws):
        return _nat.bdgcnn_train_backward(self.table, conv, inputs, d_pooled, ws)
