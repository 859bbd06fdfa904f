"""The bf16-operand entries of include/pcd.h refuse bad arguments with PCD_ERR_ARG before they touch a device, and the
modules refuse an unknown `operands` where it is given.  Runs without a GPU.
"""
import ctypes

import pytest
import torch

import pcd_native as nat
from PatchGeneration.Modules.Network.GCNModel import DGCNN, BetterDGCNN


def _refused(rc, text):
    assert rc == nat.PCD_ERR_ARG
    assert text.encode() in nat.lib().pcd_last_error(), nat.lib().pcd_last_error()


def test_operands_entries_refuse_bad_arguments():
    L = nat.lib()
    v = ctypes.c_int(-7)
    _refused(L.pcd_dgcnn_set_operands(None, 1), "model is null")
    _refused(L.pcd_dgcnn_set_operands(None, 0), "model is null")
    for bad in (2, -1, 16):                                                     # an unknown value, whatever the handle
        _refused(L.pcd_dgcnn_set_operands(None, bad), "operands must be")
    _refused(L.pcd_dgcnn_operands(None, ctypes.byref(v)), "model is null")
    assert v.value == -7
    assert nat.OPERANDS == {"fp32": 0, "bf16": 1}
    for bad in ("fp16", "BF16", None, 1, b"bf16"):
        with pytest.raises(ValueError, match="operands"):
            nat.operands_code(bad)


def test_stage_entries_refuse_bad_arguments():
    L = nat.lib()
    fake = ctypes.c_void_p(256)                                                 # never dereferenced: a check fails first
    gemm = L.pcd_dgcnn_gemm_bf16
    _refused(gemm(None, None, 4, 4, 1, 0, None, None, None, None), "is null")
    _refused(gemm(fake, fake, 4, 4, 1, 0, None, None, None, None), "is null")   # y
    _refused(gemm(fake, None, 4, 4, 1, 0, None, None, fake, None), "is null")   # x
    _refused(gemm(fake, fake, 0, 4, 1, 0, None, None, fake, None), "M and K")
    _refused(gemm(fake, fake, 4, 0, 1, 0, None, None, fake, None), "M and K")
    _refused(gemm(fake, fake, 4, 4, -1, 0, None, None, fake, None), "b must be")
    _refused(gemm(fake, fake, 4, 4, 1, 4, None, None, fake, None), "epilogue")  # no EPI_ADD on the bf16 kernel
    _refused(gemm(fake, fake, 4, 4, 1, -1, None, None, fake, None), "epilogue")
    for epi in (1, 2, 3):
        _refused(gemm(fake, fake, 4, 4, 1, epi, None, fake, fake, None), "s / t")
    edge = L.pcd_bdgcnn_edgeconv_bf16
    ok = dict(c_in=17, c_out=16, b=1, n=3, fused=nat.FUSED_AUTO)

    def call(w=fake, s=fake, t=fake, x=fake, lists=fake, out=fake, **kw):
        a = dict(ok, **kw)
        return edge(w, s, t, a["c_in"], a["c_out"], x, a["b"], lists, a["n"], a["fused"], out, None, 0, None)

    for name in ("w", "s", "t", "x", "lists", "out"):
        _refused(call(**{name: None}), "a pointer is null")
    _refused(call(fused=3), "fused must be")
    _refused(call(fused=nat.FUSED_ON, c_out=65), "2 c_out <= 128")
    _refused(call(c_in=0), "c_in and c_out")
    _refused(call(c_out=4097), "c_in and c_out")
    _refused(call(b=-1), "b must be")
    _refused(call(n=0), "list_len")
    _refused(call(n=65), "list_len")


def test_modules_refuse_unknown_operands():
    for bad in ("fp16", "float32", None, 16):
        with pytest.raises(ValueError, match="operands"):
            DGCNN(8, 17, 128, 0.5, operands=bad)
        with pytest.raises(ValueError, match="operands"):
            BetterDGCNN(1, 1, 2, (32, 48, 96, 40), 4, 17, 0.5, operands=bad)
    m = DGCNN(8, 17, 128, 0.5, operands="bf16")
    assert m.operands == "bf16" and DGCNN(8, 17, 128, 0.5).operands == "fp32"
    assert BetterDGCNN(1, 1, 2, (32, 48, 96, 40), 4, 17, 0.5, operands="bf16").operands == "bf16"
    with pytest.raises(ValueError, match="operands"):
        m.set_operands("fp16")
    assert m.operands == "bf16"                                                 # a refused value changes nothing
    assert m.set_operands("fp32") is m and m.operands == "fp32"
    # the setting is no part of the state dict
    a, b = DGCNN(8, 17, 128, 0.5, operands="bf16").state_dict(), DGCNN(8, 17, 128, 0.5).state_dict()
    assert list(a) == list(b) and not any("operands" in key for key in a)
    m.set_operands("bf16")
    m.load_state_dict(b, strict=True)
    assert m.operands == "bf16" and all(torch.equal(m.state_dict()[key], b[key]) for key in b)
