"""ctypes binding of ``libpcd.so`` -- the C-ABI declared in ``include/pcd.h``.

This is the only module that talks to the native library.  Every compute call of the drop-in classes under
``Pointcloud/Modules`` and ``PatchGeneration/Modules`` goes through here and runs a hand-written HIP kernel on the
current HIP device.  There is NO CPU fallback: if the library or a HIP device is missing, the call raises.
PyTorch is used for device memory, dtype/shape plumbing and the current stream only.
"""
from __future__ import annotations

import ctypes
import math
import os
from ctypes import POINTER, c_double, c_float, c_int, c_int64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCD_LIB", os.path.join(os.path.dirname(_HERE), "libpcd.so"))

PCD_OK, PCD_ERR_ARG, PCD_ERR_OOM, PCD_ERR_HIP, PCD_ERR_STATE, PCD_ERR_RCCL = 0, -1, -2, -3, -4, -5
DT_F32, DT_F64, DT_I32 = 0, 1, 2
OP_SUM, OP_MAX = 0, 1
COMM_HOST, COMM_RCCL = 0, 1
FIELD_POS, FIELD_NRM, FIELD_FN, FIELD_EDGE = 0, 1, 2, 3
(STAGE_KNN_NVT1, STAGE_NVT2, STAGE_PHASE_SUM, STAGE_PHASE_CENTRE, STAGE_PHASE_MAXDIST, STAGE_PHASE_APPLY,
 STAGE_FINISH) = range(7)
STEP_FLAT, STEP_EDGE, STEP_FEATURE, STEP_CORNER, STEP_NEW, STEP_DUMMY = range(6)


class PcdError(RuntimeError):
    """A native call failed (HIP error, OOM, bad state)."""


class _GridInfo(ctypes.Structure):
    _fields_ = [("n", c_int64), ("cells", c_int64), ("table_slots", c_int64), ("cell", c_float),
                ("origin", c_float * 3), ("dims", ctypes.c_int32 * 3)]


class CpsdParams(ctypes.Structure):
    """Mirror of ``pcd_cpsd_params`` (include/pcd.h)."""
    _fields_ = [("r", c_float), ("rho", c_float), ("tau", c_float), ("damp", c_float), ("d", c_float),
                ("step_clamp", c_float), ("alpha", c_float * 3), ("k_update", c_int)]


class DenoiseParams(ctypes.Structure):
    """Mirror of ``pcd_denoise_params`` (include/pcd.h)."""
    _fields_ = [("k", c_int), ("k_update", c_int), ("rho", c_float), ("tau", c_float), ("damp", c_float),
                ("class_scale", c_float), ("d", c_float), ("nphases", c_int), ("phase_class", c_int * 3),
                ("phase_kind", c_int * 3), ("phase_alpha", c_float * 3), ("jacobi", c_int), ("clamp_global", c_float)]


class DgcnnWeights(ctypes.Structure):
    """Mirror of ``pcd_dgcnn_weights`` (include/pcd.h)."""
    _fields_ = [("conv_w", c_void_p * 7), ("conv_rows", ctypes.c_int32 * 7), ("conv_cols", ctypes.c_int32 * 7),
                ("bn_weight", c_void_p * 10), ("bn_bias", c_void_p * 10), ("bn_mean", c_void_p * 10),
                ("bn_var", c_void_p * 10), ("bn_eps", c_double * 10), ("bn_len", ctypes.c_int32 * 10),
                ("lin_w", c_void_p * 4), ("lin_b", c_void_p * 4), ("lin_rows", ctypes.c_int32 * 4),
                ("lin_cols", ctypes.c_int32 * 4)]


class DgcnnDebug(ctypes.Structure):
    """Mirror of ``pcd_dgcnn_debug`` (include/pcd.h)."""
    _fields_ = [("cat", c_void_p), ("lists", c_void_p), ("pooled", c_void_p), ("h1", c_void_p), ("h2", c_void_p),
                ("h3", c_void_p)]


class DgcnnTrainParams(ctypes.Structure):
    """Mirror of ``pcd_dgcnn_train_params`` (include/pcd.h)."""
    _fields_ = [("conv_w", c_void_p * 7), ("bn_weight", c_void_p * 7), ("bn_bias", c_void_p * 7),
                ("bn_mean", c_void_p * 7), ("bn_var", c_void_p * 7), ("bn_tracked", c_void_p * 7),
                ("bn_eps", c_double * 7), ("bn_momentum", c_double * 7)]


class DgcnnTrainGrads(ctypes.Structure):
    """Mirror of ``pcd_dgcnn_train_grads`` (include/pcd.h)."""
    _fields_ = [("conv_w", c_void_p * 7), ("bn_weight", c_void_p * 7), ("bn_bias", c_void_p * 7)]


_I32P, _VPP, _F64P = POINTER(ctypes.c_int32), POINTER(c_void_p), POINTER(c_double)


class DgcnnTableStruct(ctypes.Structure):
    """Mirror of ``pcd_dgcnn_table`` (include/pcd.h)."""
    _fields_ = [("l_e", ctypes.c_int32), ("l_d", ctypes.c_int32), ("l_l", ctypes.c_int32), ("channel_sizes", _I32P),
                ("k", ctypes.c_int32), ("init_dims", ctypes.c_int32), ("output_channels", ctypes.c_int32)]


class BdgcnnWeights(ctypes.Structure):
    """Mirror of ``pcd_bdgcnn_weights`` (include/pcd.h)."""
    _fields_ = [("conv_w", _VPP), ("conv_rows", _I32P), ("conv_cols", _I32P), ("bn_weight", _VPP), ("bn_bias", _VPP),
                ("bn_mean", _VPP), ("bn_var", _VPP), ("bn_eps", _F64P), ("bn_len", _I32P), ("lin_w", _VPP),
                ("lin_b", _VPP), ("lin_rows", _I32P), ("lin_cols", _I32P)]


class BdgcnnDebug(ctypes.Structure):
    """Mirror of ``pcd_bdgcnn_debug`` (include/pcd.h)."""
    _fields_ = [("cat", c_void_p), ("lists", c_void_p), ("pooled", c_void_p), ("h", _VPP)]


class BdgcnnTrainParams(ctypes.Structure):
    """Mirror of ``pcd_bdgcnn_train_params`` (include/pcd.h)."""
    _fields_ = [("conv_w", _VPP), ("bn_weight", _VPP), ("bn_bias", _VPP), ("bn_mean", _VPP), ("bn_var", _VPP),
                ("bn_tracked", _VPP), ("bn_eps", _F64P), ("bn_momentum", _F64P)]


class BdgcnnTrainGrads(ctypes.Structure):
    """Mirror of ``pcd_bdgcnn_train_grads`` (include/pcd.h)."""
    _fields_ = [("conv_w", _VPP), ("bn_weight", _VPP), ("bn_bias", _VPP)]


# name -> (restype, argtypes); the exact export list of include/pcd.h
_SIGS = {
    "pcd_last_error": (ctypes.c_char_p, []),
    "pcd_version": (c_int, []),
    "pcd_build_id": (ctypes.c_char_p, []),
    "pcd_max_k": (c_int, []),
    "pcd_denoise_params_size": (c_int, []),
    "pcd_grid_build": (c_int, [c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p, POINTER(c_void_p)]),
    "pcd_grid_params": (c_int, [c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "pcd_grid_rebuild": (c_int, [c_void_p, c_int, c_float, c_void_p, POINTER(c_void_p)]),
    "pcd_grid_destroy": (c_int, [c_void_p]),
    "pcd_grid_get_info": (c_int, [c_void_p, POINTER(_GridInfo)]),
    "pcd_grid_perm": (c_int, [c_void_p, c_void_p, c_void_p]),
    "pcd_knn": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "pcd_knn_stats": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "pcd_radius_count": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "pcd_radius_fill": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_nvt_normal_csr": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_void_p,
                                   c_void_p, c_void_p]),
    "pcd_pvt_normal_csr": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_float,
                                   c_void_p, c_void_p, c_void_p]),
    "pcd_nvt_csr": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_void_p,
                            c_void_p, c_void_p]),
    "pcd_vu_smooth": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p, c_void_p]),
    "pcd_classify": (c_int, [c_void_p, c_int64, c_float, c_void_p, c_void_p, c_void_p]),
    "pcd_pca_dense": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "pcd_eigh3_batch": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "pcd_step_csr": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                             c_float, c_float, c_void_p, c_void_p]),
    "pcd_edge_length_sum": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_nn_dist": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "pcd_mesh_update": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p]),
    "pcd_mesh_update_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int,
                                    c_void_p]),
    "pcd_mesh_vta": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_int, c_void_p]),
    "pcd_mesh_face_geometry": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pcd_mesh_face_scale": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_mesh_nbr_count": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, ctypes.c_double,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "pcd_mesh_nbr_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_mesh_filter": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, ctypes.c_double,
                                ctypes.c_double, c_void_p, c_void_p, c_void_p]),
    "pcd_mesh_filter_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                    c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "pcd_mesh_denoise": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int, c_int, ctypes.c_double, ctypes.c_double, c_void_p, c_void_p]),
    "pcd_mesh_denoise_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int64, c_void_p, c_int, c_int, c_float, c_float, c_void_p, c_void_p]),
    "pcd_mesh_tta": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_int, c_void_p]),
    "pcd_patch_radius": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, ctypes.c_double,
                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    "pcd_patch_select_count": (c_int, [c_void_p, ctypes.c_double, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_patch_select_fill": (c_int, [c_void_p, ctypes.c_double, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_host_patch_radius": (c_int, [c_void_p, c_int64, ctypes.c_double, c_void_p]),
    "pcd_patch_inputs": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                 c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    "pcd_denoiser_create": (c_int, [c_void_p, c_int, POINTER(c_void_p)]),
    "pcd_denoiser_destroy": (c_int, [c_void_p]),
    "pcd_denoiser_load": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "pcd_denoiser_iterate": (c_int, [c_void_p, POINTER(DenoiseParams), c_int, c_void_p]),
    "pcd_denoiser_store": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pcd_denoiser_set_timing": (c_int, [c_void_p, c_int]),
    "pcd_denoiser_reset_seed": (c_int, [c_void_p]),
    "pcd_denoiser_set_seeding": (c_int, [c_void_p, c_int]),
    "pcd_denoiser_set_anchoring": (c_int, [c_void_p, c_int]),
    "pcd_denoiser_set_windows": (c_int, [c_void_p, c_int]),
    "pcd_denoiser_anchor_stats": (c_int, [c_void_p, c_void_p, c_void_p]),
    "pcd_denoiser_tile_stats": (c_int, [c_void_p, c_void_p, c_void_p]),
    "pcd_denoiser_check": (c_int, [c_void_p, c_void_p]),
    "pcd_denoiser_status": (c_int, [c_void_p, POINTER(c_int), c_void_p]),
    "pcd_denoiser_coverage_excess": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), c_void_p]),
    "pcd_denoiser_lists": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "pcd_denoiser_set_probe": (c_int, [c_void_p, c_int]),
    "pcd_denoiser_probe_store": (c_int, [c_void_p, c_void_p, c_void_p]),
    "pcd_denoiser_set_exact_nvt2": (c_int, [c_void_p, c_int]),
    "pcd_denoiser_decompose": (c_int, [c_void_p, POINTER(DenoiseParams), c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "pcd_denoiser_set_rows": (c_int, [c_void_p, c_void_p, c_int64]),
    "pcd_denoiser_set_coverage": (c_int, [c_void_p, c_void_p, c_void_p]),
    "pcd_denoiser_set_coverage_spheres": (c_int, [c_void_p, c_void_p, c_void_p]),
    "pcd_denoiser_stage": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "pcd_denoiser_pack": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_denoiser_unpack": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_denoiser_get_timing": (c_int, [c_void_p, POINTER(c_float), c_int, POINTER(c_int)]),
    "pcd_cpsd_iterate": (c_int, [c_void_p, POINTER(CpsdParams), c_int, c_void_p]),
    "pcd_comm_id_bytes": (c_int, []),
    "pcd_comm_id": (c_int, [c_void_p]),
    "pcd_comm_create": (c_int, [c_void_p, c_int, c_int, POINTER(c_void_p)]),
    "pcd_comm_create_host": (c_int, [c_void_p, c_int, c_int, POINTER(c_void_p)]),
    "pcd_comm_destroy": (c_int, [c_void_p]),
    "pcd_comm_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "pcd_comm_sendrecv": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "pcd_allreduce_scalars": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "pcd_denoiser_set_routes": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p]),
    "pcd_halo_exchange": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "pcd_denoiser_set_readset": (c_int, [c_void_p, c_int]),
    "pcd_denoiser_readset_stats": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "pcd_slab_iterate": (c_int, [c_void_p, c_void_p, POINTER(DenoiseParams), c_int, c_void_p]),
    "pcd_dgcnn_create": (c_int, [POINTER(DgcnnWeights), c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "pcd_dgcnn_destroy": (c_int, [c_void_p]),
    "pcd_dgcnn_workspace_bytes": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "pcd_dgcnn_forward": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, POINTER(DgcnnDebug),
                                  c_void_p]),
    "pcd_dgcnn_forward_deferred": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                           POINTER(DgcnnDebug), c_void_p, c_int64, c_void_p]),
    "pcd_dgcnn_knn": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "pcd_dgcnn_edgeconv": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "pcd_dgcnn_gemm": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "pcd_dgcnn_train_workspace_bytes": (c_int, [c_int, c_int, c_int64, POINTER(c_int64)]),
    "pcd_dgcnn_train_forward": (c_int, [POINTER(DgcnnTrainParams), c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p,
                                        c_int64, c_void_p, c_void_p]),
    "pcd_dgcnn_train_backward": (c_int, [c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                         POINTER(DgcnnTrainGrads), c_void_p]),
    "pcd_dgcnn_wgrad": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p]),
    "pcd_dgcnn_wgrad_split": (c_int, [c_int64, POINTER(c_int64)]),
    "pcd_dgcnn_edgeconv_train": (c_int, [c_void_p, c_void_p, c_void_p, c_double, c_double, c_void_p, c_void_p, c_void_p,
                                         c_int, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    "pcd_dgcnn_edgeconv_train_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_double, c_int, c_void_p, c_int64,
                                                  c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_void_p]),
    "pcd_bdgcnn_create": (c_int, [POINTER(DgcnnTableStruct), POINTER(BdgcnnWeights), POINTER(c_void_p)]),
    "pcd_bdgcnn_destroy": (c_int, [c_void_p]),
    "pcd_bdgcnn_workspace_bytes": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "pcd_bdgcnn_forward": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, POINTER(BdgcnnDebug),
                                   c_void_p]),
    "pcd_bdgcnn_forward_deferred": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                            POINTER(BdgcnnDebug), c_void_p, c_int64, c_void_p]),
    "pcd_bdgcnn_edgeconv": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int64, c_void_p, c_int,
                                    c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "pcd_bdgcnn_edgeconv_scratch_bytes": (c_int, [c_int, c_int, c_int64, POINTER(c_int64)]),
    "pcd_dgcnn_set_operands": (c_int, [c_void_p, c_int]),
    "pcd_dgcnn_operands": (c_int, [c_void_p, POINTER(c_int)]),
    "pcd_dgcnn_gemm_bf16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "pcd_bdgcnn_edgeconv_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int64, c_void_p, c_int,
                                         c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "pcd_bdgcnn_train_workspace_bytes": (c_int, [POINTER(DgcnnTableStruct), c_int64, POINTER(c_int64)]),
    "pcd_bdgcnn_train_forward": (c_int, [POINTER(DgcnnTableStruct), POINTER(BdgcnnTrainParams), c_void_p, c_int64,
                                         c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_bdgcnn_train_backward": (c_int, [POINTER(DgcnnTableStruct), c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                          c_int64, POINTER(BdgcnnTrainGrads), c_void_p]),
    "pcd_orient_normals_mst": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64]),
    "pcd_orient_normals_mst_gpu": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "pcd_host_eigh3": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_host_vu_smooth": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p]),
    "pcd_host_solve3": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_host_inv3": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "pcd_host_step_csr": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float,
                                  c_float, c_float, c_void_p]),
    "pcd_host_nvt_tensor": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_void_p]),
}

_lib = None


def lib():
    """Load libpcd.so once (raises ImportError with the build hint if it is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"pcd: native library not found at {LIB_PATH}; run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C normal-guided-pointcloud-denoiser_amd/csrc`")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name, None)
            if f is None:
                if "PCD_LIB" in os.environ:     # an older experiment build (A/B): its missing entry points stay unbound
                    continue
                raise ImportError(f"pcd: {LIB_PATH} does not export {name}: rebuild it")
            f.restype = res
            f.argtypes = args
        # the params mirror must match the library's struct (a shorter one would be read past its end)
        if ctypes.sizeof(DenoiseParams) != L.pcd_denoise_params_size():
            raise ImportError(f"pcd: DenoiseParams mirror is {ctypes.sizeof(DenoiseParams)} B, the library's "
                              f"pcd_denoise_params is {L.pcd_denoise_params_size()} B -- rebuild or update the mirror")
        _lib = L
    return _lib


def build_id() -> str:
    """The loaded library's build id (pcd_build_id: a hash of its sources and extra flags)."""
    return lib().pcd_build_id().decode()


def exported_symbols():
    return list(_SIGS.keys())


def check(status: int, what: str = ""):
    if status == PCD_OK:
        return
    msg = lib().pcd_last_error().decode(errors="replace")
    if status == PCD_ERR_ARG:
        raise ValueError(f"pcd: {what}: {msg}")
    raise PcdError(f"pcd: {what} failed ({status}): {msg}")


# ----------------------------------------------------------------------------------------------- device plumbing
def device() -> torch.device:
    """The HIP device every kernel runs on.  Raises if there is none (no CPU fallback)."""
    if not torch.cuda.is_available():
        raise RuntimeError("pcd: no HIP (ROCm) device available -- the denoiser runs its kernels on MI355X only")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: torch.Tensor | None):
    return None if t is None else c_void_p(t.data_ptr())


def on_device(t: torch.Tensor, dtype=None) -> torch.Tensor:
    """Contiguous copy/view of `t` on the HIP device with the requested dtype."""
    dev = device()
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if t.device != dev:
        t = t.to(dev, non_blocking=False)
    return t.contiguous()


def f32(t):
    return on_device(t, torch.float32)


def i64(t):
    return on_device(t, torch.int64)


# ----------------------------------------------------------------------------------------------- objects
class Grid:
    """Frozen snapshot + kNN index (pcd_grid).  Mirrors the KDTree made in Selector.__init__."""

    def __init__(self, xyz: torch.Tensor, k_hint: int = 16, cell: float = 0.0, origin=None):
        """origin: optional (3,) lattice origin (needs cell > 0), see pcd_grid_build."""
        L = lib()
        x = f32(xyz)
        assert x.dim() == 2 and x.size(1) == 3
        self._keep = x
        h = c_void_p()
        org = None
        if origin is not None:
            org = (ctypes.c_float * 3)(*[float(v) for v in origin])
        check(L.pcd_grid_build(ptr(x), x.size(0), int(k_hint), float(cell), org, c_void_p(stream_ptr()),
                               ctypes.byref(h)), "pcd_grid_build")
        self.handle = h
        self.n = x.size(0)
        self.k_hint = int(k_hint) if cell <= 0 else 0
        self._keep = None

    def rebuild(self, k_hint: int) -> "Grid":
        """A grid over this grid's own frozen snapshot with cells of ~k_hint/2 points (pcd_grid_rebuild)."""
        h = c_void_p()
        check(lib().pcd_grid_rebuild(self.handle, int(k_hint), 0.0, c_void_p(stream_ptr()), ctypes.byref(h)),
              "pcd_grid_rebuild")
        g = Grid.__new__(Grid)
        g.handle, g.n, g.k_hint, g._keep = h, self.n, int(k_hint), None
        return g

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value and _lib is not None:
            _lib.pcd_grid_destroy(h)
            self.handle = None

    def info(self) -> dict:
        gi = _GridInfo()
        check(lib().pcd_grid_get_info(self.handle, ctypes.byref(gi)), "pcd_grid_get_info")
        return {"n": gi.n, "cells": gi.cells, "table_slots": gi.table_slots, "cell": gi.cell,
                "origin": list(gi.origin), "dims": list(gi.dims)}

    def perm(self) -> torch.Tensor:
        out = torch.empty(self.n, dtype=torch.int32, device=device())
        check(lib().pcd_grid_perm(self.handle, ptr(out), c_void_p(stream_ptr())), "pcd_grid_perm")
        return out

    def knn(self, q: torch.Tensor, k: int, exclude_self: bool = False, with_d2: bool = False, idx_bits: int = 64,
            sorted_ids: bool = False):
        q = f32(q)
        nq = q.size(0)
        idx = torch.empty((nq, k), dtype=torch.int64 if idx_bits == 64 else torch.int32, device=q.device)
        d2 = torch.empty((nq, k), dtype=torch.float32, device=q.device) if with_d2 else None
        check(lib().pcd_knn(self.handle, ptr(q), nq, int(k), ptr(idx), idx_bits, int(sorted_ids), int(exclude_self),
                            ptr(d2), c_void_p(stream_ptr())), "pcd_knn")
        return (idx, d2) if with_d2 else idx

    def knn_stats(self, q: torch.Tensor, k: int, batched: bool = False) -> dict:
        """Per-query averages of the kNN search work (diagnostic build of the search; batched or insertion)."""
        q = f32(q)
        out = torch.zeros(6, dtype=torch.int64, device=q.device)
        check(lib().pcd_knn_stats(self.handle, ptr(q), q.size(0), int(k), int(bool(batched)), ptr(out),
                                  c_void_p(stream_ptr())),
              "pcd_knn_stats")
        v = out.cpu().double() / max(q.size(0), 1)
        names = ["cells_considered", "cells_probed", "cells_found", "candidates", "inserts", "extra_rings"]
        return {nm: round(float(x), 2) for nm, x in zip(names, v)}

    def radius_counts(self, q: torch.Tensor, radii: torch.Tensor) -> torch.Tensor:
        """Member counts of the balls of radii[i] around q[i] (pcd_radius_count), int64 [nq]."""
        q = f32(q)
        r = f32(radii)
        counts = torch.empty(q.size(0), dtype=torch.int64, device=q.device)
        check(lib().pcd_radius_count(self.handle, ptr(q), q.size(0), ptr(r), ptr(counts), c_void_p(stream_ptr())),
              "pcd_radius_count")
        return counts

    def radius(self, q: torch.Tensor, radii: torch.Tensor):
        """Members of the ball of radii[i] around q[i] (original snapshot ids, ascending): (slices int64 [nq+1],
        j int64 [total]) -- scipy query_ball_point semantics (pcd_radius_count / pcd_radius_fill)."""
        q = f32(q)
        r = f32(radii)
        nq = q.size(0)
        counts = torch.empty(nq, dtype=torch.int64, device=q.device)
        check(lib().pcd_radius_count(self.handle, ptr(q), nq, ptr(r), ptr(counts), c_void_p(stream_ptr())),
              "pcd_radius_count")
        slices = torch.zeros(nq + 1, dtype=torch.int64, device=q.device)
        torch.cumsum(counts, 0, out=slices[1:])
        total = int(slices[-1])
        j = torch.empty(total, dtype=torch.int64, device=q.device)
        check(lib().pcd_radius_fill(self.handle, ptr(q), nq, ptr(r), ptr(slices), total, ptr(j),
                                    c_void_p(stream_ptr())), "pcd_radius_fill")
        return slices, j

    def nn(self, q: torch.Tensor):
        q = f32(q)
        d2 = torch.empty(q.size(0), dtype=torch.float32, device=q.device)
        idx = torch.empty(q.size(0), dtype=torch.int64, device=q.device)
        check(lib().pcd_nn_dist(self.handle, ptr(q), q.size(0), ptr(d2), ptr(idx), c_void_p(stream_ptr())),
              "pcd_nn_dist")
        return d2, idx


class FusedDenoiser:
    """Persistent buffers of the fused loop (pcd_denoiser) bound to one Grid."""

    def __init__(self, grid: Grid, k_max: int):
        self.grid = grid
        h = c_void_p()
        check(lib().pcd_denoiser_create(grid.handle, int(k_max), ctypes.byref(h)), "pcd_denoiser_create")
        self.handle = h
        self.k_max = k_max

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value and _lib is not None:
            _lib.pcd_denoiser_destroy(h)
            self.handle = None

    def load(self, pos: torch.Tensor, n: torch.Tensor):
        pos, n = f32(pos), f32(n)
        check(lib().pcd_denoiser_load(self.handle, ptr(pos), ptr(n), c_void_p(stream_ptr())), "pcd_denoiser_load")

    def iterate(self, params: DenoiseParams, iterations: int):
        check(lib().pcd_denoiser_iterate(self.handle, ctypes.byref(params), int(iterations), c_void_p(stream_ptr())),
              "pcd_denoiser_iterate")

    def store(self, pos=None, n=None, classes=None, edge_vectors=None):
        check(lib().pcd_denoiser_store(self.handle, ptr(pos), ptr(n), ptr(classes), ptr(edge_vectors),
                                       c_void_p(stream_ptr())), "pcd_denoiser_store")

    def lists(self, cols: int) -> torch.Tensor:
        """The kNN lists of the last iteration (original indices, caller order): int64 [N, cols]."""
        out = torch.empty((self.grid.n, int(cols)), dtype=torch.int64, device=device())
        check(lib().pcd_denoiser_lists(self.handle, ptr(out), int(cols), c_void_p(stream_ptr())), "pcd_denoiser_lists")
        return out

    def set_probe(self, enable=True):
        """NVT2 parity probe on / off (pcd_denoiser_set_probe)."""
        check(lib().pcd_denoiser_set_probe(self.handle, int(bool(enable))), "pcd_denoiser_set_probe")

    def probe(self) -> torch.Tensor:
        """(λ0, λ1, λ2, Σw) of the last NVT2 stage per point, caller order: float32 [N, 4]."""
        out = torch.empty((self.grid.n, 4), dtype=torch.float32, device=device())
        check(lib().pcd_denoiser_probe_store(self.handle, ptr(out), c_void_p(stream_ptr())), "pcd_denoiser_probe_store")
        return out

    def set_exact_nvt2(self, enable=True):
        """NVT2 as the reference computes it (T / Σw, LAPACK's eigh: edge vectors with LAPACK's sign) on / off
        (pcd_denoiser_set_exact_nvt2; off by default)."""
        check(lib().pcd_denoiser_set_exact_nvt2(self.handle, int(bool(enable))), "pcd_denoiser_set_exact_nvt2")

    def decompose(self, params: DenoiseParams, want_classes: bool = False):
        """getMyFeatureDecomposition of the loaded state from the fused stages (pcd_denoiser_decompose):
        (eigval [N, 3], eigvec [N, 3, 3], f_n [N, 3][, classes int64 [N]]), caller order.  Moves nothing."""
        N, dev = self.grid.n, device()
        eigval = torch.empty((N, 3), dtype=torch.float32, device=dev)
        eigvec = torch.empty((N, 3, 3), dtype=torch.float32, device=dev)
        f_n = torch.empty((N, 3), dtype=torch.float32, device=dev)
        cls = torch.empty(N, dtype=torch.int64, device=dev) if want_classes else None
        check(lib().pcd_denoiser_decompose(self.handle, ctypes.byref(params), ptr(eigval), ptr(eigvec), ptr(f_n),
                                           ptr(cls), c_void_p(stream_ptr())), "pcd_denoiser_decompose")
        return (eigval, eigvec, f_n, cls) if want_classes else (eigval, eigvec, f_n)

    def set_seeding(self, enable=True):
        check(lib().pcd_denoiser_set_seeding(self.handle, int(bool(enable))), "pcd_denoiser_set_seeding")

    def set_anchoring(self, enable=True):
        check(lib().pcd_denoiser_set_anchoring(self.handle, int(bool(enable))), "pcd_denoiser_set_anchoring")

    def set_windows(self, enable=True):
        check(lib().pcd_denoiser_set_windows(self.handle, int(bool(enable))), "pcd_denoiser_set_windows")

    def redo_rows(self) -> int:
        """Rows re-anchored by the last anchored kNN stage (-1: none ran)."""
        v = ctypes.c_int64(0)
        check(lib().pcd_denoiser_anchor_stats(self.handle, ctypes.byref(v), c_void_p(stream_ptr())),
              "pcd_denoiser_anchor_stats")
        return v.value

    def tile_stats(self) -> dict:
        """Counters of the last anchored kNN stage (pcd_denoiser_tile_stats)."""
        v = (ctypes.c_int64 * 4)()
        check(lib().pcd_denoiser_tile_stats(self.handle, v, c_void_p(stream_ptr())), "pcd_denoiser_tile_stats")
        return {"rows": v[0], "spilled": v[1], "spilled_big_box": v[2], "spilled_ambiguous": v[3]}

    def reset_seed(self):
        check(lib().pcd_denoiser_reset_seed(self.handle), "pcd_denoiser_reset_seed")

    def set_timing(self, on):
        """False / True: off / every stage (TIMING_SLOTS); 2: the K1 stage only (one slot, K1's ms)."""
        check(lib().pcd_denoiser_set_timing(self.handle, int(on)), "pcd_denoiser_set_timing")

    def check(self):
        check(lib().pcd_denoiser_check(self.handle, c_void_p(stream_ptr())), "pcd_denoiser_check")

    def status(self) -> int:
        """Device error word (bit 0: invalid list entry, bit 1: a k-ball left the coverage box -- bit 2: a sphere-less
        row, bit 3: a coverage-sphere row), not raising."""
        v = c_int(0)
        check(lib().pcd_denoiser_status(self.handle, ctypes.byref(v), c_void_p(stream_ptr())), "pcd_denoiser_status")
        return v.value

    def coverage_excess(self) -> tuple:
        """(band_excess, sphere_ratio) of the failed coverage checks (pcd_denoiser_coverage_excess): how far the
        farthest sphere-less k-ball reached past the coverage box, the largest (|q - c| + d_k) / R of a sphere row
        (0: no such failure)."""
        b, s = c_float(0.0), c_float(0.0)
        check(lib().pcd_denoiser_coverage_excess(self.handle, ctypes.byref(b), ctypes.byref(s), c_void_p(stream_ptr())),
              "pcd_denoiser_coverage_excess")
        return float(b.value), float(s.value)

    # ---- spatial slabs: active rows, coverage, staged iteration, halo pack/unpack (include/pcd.h)
    @staticmethod
    def _rows_i32(rows: torch.Tensor) -> torch.Tensor:
        """Row lists go to the C-ABI as int32_t*: any integer tensor is converted on the HIP device (the converted
        tensor must be kept alive by the caller until the launch has consumed it)."""
        assert not rows.is_floating_point() and not rows.is_complex(), "row indices must be an integer tensor"
        return on_device(rows.reshape(-1), torch.int32)

    def set_rows(self, rows):
        """rows: integer tensor of spatial-order rows (converted to int32 on the device and kept alive here), or
        None for all rows."""
        self._rows = None if rows is None else self._rows_i32(rows)
        n = 0 if rows is None else self._rows.numel()
        check(lib().pcd_denoiser_set_rows(self.handle, ptr(self._rows), n), "pcd_denoiser_set_rows")

    def set_coverage(self, lo=None, hi=None):
        if lo is None:
            check(lib().pcd_denoiser_set_coverage(self.handle, None, None), "pcd_denoiser_set_coverage")
            return
        lo3 = (c_float * 3)(*[float(v) for v in lo])
        hi3 = (c_float * 3)(*[float(v) for v in hi])
        check(lib().pcd_denoiser_set_coverage(self.handle, lo3, hi3), "pcd_denoiser_set_coverage")

    def set_coverage_spheres(self, radii=None):
        """Per-point coverage spheres (float32 [n], caller order, 0 = none; None clears): pcd_denoiser_set_coverage_spheres."""
        r = None if radii is None else f32(radii)
        if r is not None:
            assert r.dim() == 1 and r.numel() == self.grid.n
        check(lib().pcd_denoiser_set_coverage_spheres(self.handle, ptr(r), c_void_p(stream_ptr())),
              "pcd_denoiser_set_coverage_spheres")
        if r is not None:
            torch.cuda.current_stream().synchronize()

    def stage(self, params: DenoiseParams, stage: int, phase: int = 0, red: torch.Tensor = None):
        check(lib().pcd_denoiser_stage(self.handle, ctypes.byref(params), int(stage), int(phase), ptr(red),
                                       c_void_p(stream_ptr())), "pcd_denoiser_stage")

    def pack(self, field: int, rows: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        rows = self._rows_i32(rows)
        n = rows.numel()
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=rows.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (n, 4) and out.device == rows.device
        check(lib().pcd_denoiser_pack(self.handle, int(field), ptr(rows), n, ptr(out), c_void_p(stream_ptr())),
              "pcd_denoiser_pack")
        return out

    def unpack(self, field: int, rows: torch.Tensor, data: torch.Tensor):
        rows = self._rows_i32(rows)
        data = data.contiguous()
        assert data.dtype == torch.float32 and data.shape == (rows.numel(), 4) and data.device == rows.device
        check(lib().pcd_denoiser_unpack(self.handle, int(field), ptr(rows), rows.numel(), ptr(data),
                                        c_void_p(stream_ptr())), "pcd_denoiser_unpack")

    # ---- spatial slabs in one call per iteration (pcd_denoiser_set_routes / pcd_slab_iterate, include/pcd.h)
    def set_routes(self, peers, send_rows, recv_rows, own_lo=None, own_hi=None):
        """peers: list of peer ranks; send_rows / recv_rows: per peer an integer tensor of spatial-order rows.  The
        library copies them.  own_lo / own_hi: the owned slab's box (enables the exchange / compute overlap)."""
        npeers = len(peers)
        pa = (c_int * max(npeers, 1))(*[int(q) for q in peers])
        ns = (c_int64 * max(npeers, 1))(*[int(r.numel()) for r in send_rows])
        nr = (c_int64 * max(npeers, 1))(*[int(r.numel()) for r in recv_rows])
        dev = device()
        cat = lambda rs: (torch.cat([self._rows_i32(r) for r in rs]) if rs and sum(r.numel() for r in rs)
                          else torch.zeros(1, dtype=torch.int32, device=dev))
        sr, rr = cat(send_rows), cat(recv_rows)
        lo3 = None if own_lo is None else (c_float * 3)(*[float(v) for v in own_lo])
        hi3 = None if own_hi is None else (c_float * 3)(*[float(v) for v in own_hi])
        check(lib().pcd_denoiser_set_routes(self.handle, npeers, pa, ns, ptr(sr), nr, ptr(rr), lo3, hi3,
                                            c_void_p(stream_ptr())), "pcd_denoiser_set_routes")

    def cpsd_iterate(self, params: "CpsdParams", iterations: int):
        """The CPSD driver's iterations on the loaded state (pcd_cpsd_iterate)."""
        check(lib().pcd_cpsd_iterate(self.handle, ctypes.byref(params), int(iterations), c_void_p(stream_ptr())),
              "pcd_cpsd_iterate")

    def slab_iterate(self, comm: "Comm", params: DenoiseParams, iterations: int = 1):
        check(lib().pcd_slab_iterate(self.handle, comm.handle, ctypes.byref(params), int(iterations),
                                     c_void_p(stream_ptr())), "pcd_slab_iterate")

    def halo_exchange(self, comm: "Comm", field: int):
        check(lib().pcd_halo_exchange(self.handle, comm.handle, int(field), c_void_p(stream_ptr())),
              "pcd_halo_exchange")

    def set_readset(self, on: bool):
        """slab_iterate moves only the halo rows the lists read (pcd_denoiser_set_readset; default on)."""
        check(lib().pcd_denoiser_set_readset(self.handle, int(bool(on))), "pcd_denoiser_set_readset")

    def readset_stats(self) -> tuple:
        """(iterations, send rows, receive rows) of the read-set exchange since set_routes, summed."""
        it, s, r = c_int64(0), c_int64(0), c_int64(0)
        check(lib().pcd_denoiser_readset_stats(self.handle, ctypes.byref(it), ctypes.byref(s), ctypes.byref(r)),
              "pcd_denoiser_readset_stats")
        return it.value, s.value, r.value

    TIMING_SLOTS = ("anchor_test", "requery", "spill_search", "nvt1", "nvt2", "flat_phase", "edge_phase",
                    "corner_phase", "finish")

    def timing(self):
        """Per-stage ms averaged over the iterations timed since set_timing / the last call (TIMING_SLOTS order)."""
        buf = (c_float * 16)()
        nw = c_int(0)
        check(lib().pcd_denoiser_get_timing(self.handle, buf, 16, ctypes.byref(nw)), "pcd_denoiser_get_timing")
        return [buf[i] for i in range(nw.value)]


# ----------------------------------------------------------------------------------------------- slab transport
_EXCHANGE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_int, POINTER(c_int), POINTER(c_float), POINTER(c_int64),
                                POINTER(c_float), POINTER(c_int64))
_ALLREDUCE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_int, c_int, c_int)


class _HostTransport(ctypes.Structure):
    _fields_ = [("user", c_void_p), ("exchange", _EXCHANGE_FN), ("allreduce", _ALLREDUCE_FN)]


class Comm:
    """The slab transport of libpcd (pcd_comm): RCCL, or host callbacks over a torch.distributed CPU group (gloo)."""

    def __init__(self, handle, keep=None):
        self.handle = handle
        self._keep = keep

    @staticmethod
    def rccl(world: int, rank: int, broadcast) -> "Comm":
        """Collective: rank 0 makes an RCCL unique id, `broadcast(uint8 tensor)` (in place, from rank 0) hands it to
        every rank, and every rank joins the communicator on its current HIP device."""
        L = lib()
        nb = L.pcd_comm_id_bytes()
        buf = (ctypes.c_ubyte * nb)()
        if rank == 0:
            check(L.pcd_comm_id(buf), "pcd_comm_id")
        t = torch.tensor(bytearray(buf), dtype=torch.uint8)
        t = broadcast(t)
        ctypes.memmove(buf, bytes(t.cpu().numpy().tobytes()), nb)
        h = c_void_p()
        check(L.pcd_comm_create(buf, int(world), int(rank), ctypes.byref(h)), "pcd_comm_create")
        return Comm(h)

    @staticmethod
    def host(world: int, rank: int, exchange, allreduce) -> "Comm":
        """exchange(peers, send [ns, 4] f32 array, send_off, recv [nr, 4] array to fill, recv_off) and
        allreduce(buf array, op) over numpy views of the library's host staging buffers (no copies)."""
        import numpy as np

        def _ex(user, npeers, peers, send, soff, recv, roff):
            try:
                P = [peers[q] for q in range(npeers)]
                so = [soff[q] for q in range(npeers + 1)]
                ro = [roff[q] for q in range(npeers + 1)]
                sa = np.ctypeslib.as_array(send, shape=(max(so[-1], 1) * 4,)).reshape(-1, 4)
                ra = np.ctypeslib.as_array(recv, shape=(max(ro[-1], 1) * 4,)).reshape(-1, 4)
                exchange(P, sa, so, ra, ro)
                return 0
            except Exception as e:                              # noqa: BLE001  (reported as a status code)
                import traceback
                traceback.print_exc()
                return 1

        def _ar(user, buf, count, dtype, op):
            try:
                dt = {DT_F32: np.float32, DT_F64: np.float64, DT_I32: np.int32}[dtype]
                arr = np.frombuffer((ctypes.c_char * (count * np.dtype(dt).itemsize)).from_address(buf), dtype=dt)
                allreduce(arr, op)
                return 0
            except Exception:                                   # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        cbs = _HostTransport(None, _EXCHANGE_FN(_ex), _ALLREDUCE_FN(_ar))
        h = c_void_p()
        check(lib().pcd_comm_create_host(ctypes.byref(cbs), int(world), int(rank), ctypes.byref(h)),
              "pcd_comm_create_host")
        return Comm(h, keep=(cbs, _ex, _ar))

    def info(self) -> dict:
        """world / rank / transport ("rccl" or "host") as the library's communicator sees them (pcd_comm_info)."""
        w, r, tr = c_int(0), c_int(0), c_int(0)
        check(lib().pcd_comm_info(self.handle, ctypes.byref(w), ctypes.byref(r), ctypes.byref(tr)), "pcd_comm_info")
        return {"world": w.value, "rank": r.value, "transport": "rccl" if tr.value == COMM_RCCL else "host"}

    def sendrecv(self, send_peer: int = -1, send: torch.Tensor = None, recv_peer: int = -1,
                 recv: torch.Tensor = None):
        """Point-to-point copy of contiguous device tensors (pcd_comm_sendrecv): `send` to rank send_peer, `recv`
        filled from rank recv_peer, in place; either side may be absent (peer -1)."""
        for t in (send, recv):
            assert t is None or (t.is_cuda and t.is_contiguous() and (t.numel() * t.element_size()) % 4 == 0)
        sb = 0 if send is None else send.numel() * send.element_size()
        rb = 0 if recv is None else recv.numel() * recv.element_size()
        check(lib().pcd_comm_sendrecv(self.handle, int(send_peer if send is not None else -1), ptr(send), sb,
                                      int(recv_peer if recv is not None else -1), ptr(recv), rb,
                                      c_void_p(stream_ptr())), "pcd_comm_sendrecv")
        return recv

    def allreduce_(self, t: torch.Tensor, op: int = OP_SUM) -> torch.Tensor:
        """In-place all-reduce of a small device tensor (float32 / float64 / int32)."""
        dt = {torch.float32: DT_F32, torch.float64: DT_F64, torch.int32: DT_I32}[t.dtype]
        assert t.is_contiguous() and t.is_cuda
        check(lib().pcd_allreduce_scalars(self.handle, ptr(t), t.numel(), dt, int(op), c_void_p(stream_ptr())),
              "pcd_allreduce_scalars")
        return t

    def destroy(self):
        """pcd_comm_destroy now (every rank at the same point of its program: the RCCL communicator's teardown)."""
        h = getattr(self, "handle", None)
        if h is not None and h.value and _lib is not None:
            _lib.pcd_comm_destroy(h)
        self.handle = None

    def __del__(self):
        self.destroy()


def make_cpsd_params(r, d, rho=0.9, tau=0.3, damp=3.0, step_clamp=None, alphas=(0.1, 1.0, 1.0), k_update=8):
    p = CpsdParams()
    p.r, p.rho, p.tau, p.damp, p.d = float(r), float(rho), float(tau), float(damp), float(d)
    p.step_clamp = float(d * 20000.0 if step_clamp is None else step_clamp)
    for a in range(3):
        p.alpha[a] = float(alphas[a])
    p.k_update = int(k_update)
    return p


def make_params(k=16, k_update=8, rho=None, tau=0.3, damp=3.0, class_scale=0.2, d=1.0,
                phases=((0, STEP_FLAT, 1.0), (1, STEP_EDGE, 0.2), (2, STEP_FEATURE, 1.0)), jacobi=False,
                clamp_global=0.0) -> DenoiseParams:
    import math
    p = DenoiseParams()
    p.k, p.k_update = int(k), int(k_update)
    p.rho = float(math.pi * 5 / 12 if rho is None else rho)
    p.tau, p.damp, p.class_scale, p.d = float(tau), float(damp), float(class_scale), float(d)
    p.nphases = len(phases)
    for t, (c, kind, a) in enumerate(phases):
        p.phase_class[t], p.phase_kind[t], p.phase_alpha[t] = int(c), int(kind), float(a)
    p.jacobi = int(bool(jacobi))
    p.clamp_global = float(clamp_global)
    return p


# ----------------------------------------------------------------------------------------------- op wrappers
def nvt_csr(pos, n, ci, off, nbr, rho):
    m = ci.size(0)
    ev = torch.empty((m, 3), dtype=torch.float32, device=pos.device)
    evec = torch.empty((m, 3, 3), dtype=torch.float32, device=pos.device)
    check(lib().pcd_nvt_csr(ptr(pos), ptr(n), pos.size(0), ptr(ci), ptr(off), ptr(nbr), m, float(rho), ptr(ev),
                            ptr(evec), c_void_p(stream_ptr())), "pcd_nvt_csr")
    return ev, evec


def nvt_normal_csr(n, ci, off, nbr, rho):
    m = ci.size(0)
    ev = torch.empty((m, 3), dtype=torch.float32, device=n.device)
    evec = torch.empty((m, 3, 3), dtype=torch.float32, device=n.device)
    check(lib().pcd_nvt_normal_csr(ptr(n), n.size(0), ptr(ci), ptr(off), ptr(nbr), m, float(rho), ptr(ev),
                                   ptr(evec), c_void_p(stream_ptr())), "pcd_nvt_normal_csr")
    return ev, evec


def pvt_normal_csr(pos, n, ci, off, nbr, rho):
    m = ci.size(0)
    ev = torch.empty((m, 3), dtype=torch.float32, device=pos.device)
    evec = torch.empty((m, 3, 3), dtype=torch.float32, device=pos.device)
    check(lib().pcd_pvt_normal_csr(ptr(pos), ptr(n), pos.size(0), ptr(ci), ptr(off), ptr(nbr), m, float(rho),
                                   ptr(ev), ptr(evec), c_void_p(stream_ptr())), "pcd_pvt_normal_csr")
    return ev, evec


def vu_smooth(eigval, eigvec, n, tau, damp):
    out = torch.empty_like(n)
    check(lib().pcd_vu_smooth(ptr(eigval), ptr(eigvec), ptr(n), n.size(0), float(tau), float(damp), ptr(out),
                              c_void_p(stream_ptr())), "pcd_vu_smooth")
    return out


def classify(eigval, scale, want_features=False):
    m = eigval.size(0)
    cls = torch.empty(m, dtype=torch.int64, device=eigval.device)
    feat = torch.empty((m, 3), dtype=torch.float32, device=eigval.device) if want_features else None
    check(lib().pcd_classify(ptr(eigval), m, float(scale), ptr(feat), ptr(cls), c_void_p(stream_ptr())),
          "pcd_classify")
    return cls, feat


def pca_dense(pos, nbr, k):
    n = pos.size(0)
    ev = torch.empty((n, 3), dtype=torch.float32, device=pos.device)
    evec = torch.empty((n, 3, 3), dtype=torch.float32, device=pos.device)
    check(lib().pcd_pca_dense(ptr(pos), n, ptr(nbr), int(k), ptr(ev), ptr(evec), c_void_p(stream_ptr())),
          "pcd_pca_dense")
    return ev, evec


def eigh3_batch(t6, solver=0):
    """Device eigen-solvers of the kernels on t6 (m, 6): solver 0 (LAPACK restatement) -> (w (m,3), V (m,3,3));
    solver 1 (NVT2's Jacobi) -> (w (m,3), y (m,3))."""
    t = f32(t6)
    assert t.dim() == 2 and t.size(1) == 6
    m = t.size(0)
    w = torch.empty((m, 3), dtype=torch.float32, device=t.device)
    vec = torch.empty((m, 3, 3) if solver == 0 else (m, 3), dtype=torch.float32, device=t.device)
    check(lib().pcd_eigh3_batch(ptr(t), m, int(solver), ptr(w), ptr(vec), c_void_p(stream_ptr())), "pcd_eigh3_batch")
    return w, vec


def step_csr(kind, pos, n, edge_vectors, ci, off, nbr, d, alpha):
    m = ci.size(0)
    out = torch.empty((m, 3), dtype=torch.float32, device=pos.device)
    check(lib().pcd_step_csr(int(kind), ptr(pos), ptr(n), ptr(edge_vectors), pos.size(0), ptr(ci), ptr(off),
                             ptr(nbr), m, float(d), float(alpha), ptr(out), c_void_p(stream_ptr())), "pcd_step_csr")
    return out


def edge_length_sum(pos, a, b):
    s = torch.empty(1, dtype=torch.float64, device=pos.device)
    check(lib().pcd_edge_length_sum(ptr(pos), ptr(a), ptr(b), a.size(0), ptr(s), c_void_p(stream_ptr())),
          "pcd_edge_length_sum")
    return s


def mesh_update(v, f, fn, vf, ni, k):
    check(lib().pcd_mesh_update(ptr(v), v.size(0), ptr(f), ptr(fn), f.size(0), ptr(vf), ptr(ni), int(k),
                                c_void_p(stream_ptr())), "pcd_mesh_update")


def mesh_update_f32(v, f, fn, vf, ni, k):
    """fp32 sweeps: v float32 [nv,3] (in place), f int32 [nf,3], fn float32 [nf,3], vf / ni int32 (device)."""
    assert v.dtype == torch.float32 and fn.dtype == torch.float32
    assert f.dtype == torch.int32 and vf.dtype == torch.int32 and ni.dtype == torch.int32
    check(lib().pcd_mesh_update_f32(ptr(v), v.size(0), ptr(f), ptr(fn), f.size(0), ptr(vf), ptr(ni), int(k),
                                    c_void_p(stream_ptr())), "pcd_mesh_update_f32")


def mesh_vta(f: torch.Tensor, nv: int, out_dtype=torch.int64):
    """igl.vertex_triangle_adjacency on the device: (vf [3 nf], ni [nv + 1]) in out_dtype (int32 / int64)."""
    f = on_device(f)
    assert f.dtype in (torch.int32, torch.int64) and f.dim() == 2 and f.size(1) == 3
    nf = f.size(0)
    vf = torch.empty(3 * nf, dtype=out_dtype, device=f.device)
    ni = torch.empty(nv + 1, dtype=out_dtype, device=f.device)
    check(lib().pcd_mesh_vta(ptr(f), 32 if f.dtype == torch.int32 else 64, nf, int(nv), ptr(vf), ptr(ni),
                             32 if out_dtype == torch.int32 else 64, c_void_p(stream_ptr())), "pcd_mesh_vta")
    return vf, ni


# guided bilateral normal filtering (MeshNormalFiltering.cpp:170-244); every tensor on the device, contiguous
def _is(t, dtype, *shape):
    return t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape


def mesh_face_geometry(v, f):
    """(centroid [nf,3], area [nf], normal [nf,3]) of the faces f int64 [nf,3] over v float64 [nv,3]."""
    nf = f.size(0)
    assert _is(v, torch.float64, v.size(0), 3) and _is(f, torch.int64, nf, 3)
    c = torch.empty((nf, 3), dtype=torch.float64, device=v.device)
    a = torch.empty(nf, dtype=torch.float64, device=v.device)
    n = torch.empty((nf, 3), dtype=torch.float64, device=v.device)
    check(lib().pcd_mesh_face_geometry(ptr(v), v.size(0), ptr(f), nf, ptr(c), ptr(a), ptr(n), c_void_p(stream_ptr())),
          "pcd_mesh_face_geometry")
    return c, a, n


def mesh_face_scale(c, f, vf, ni):
    """Device float64 [2]: the mean centroid distance of edge-adjacent faces, and the number of (ordered) pairs."""
    nf, nv = f.size(0), ni.size(0) - 1
    assert _is(c, torch.float64, nf, 3) and _is(f, torch.int64, nf, 3)
    assert _is(vf, torch.int64, 3 * nf) and _is(ni, torch.int64, nv + 1)
    out = torch.empty(2, dtype=torch.float64, device=c.device)
    check(lib().pcd_mesh_face_scale(ptr(c), ptr(f), nf, ptr(vf), ptr(ni), nv, ptr(out), c_void_p(stream_ptr())),
          "pcd_mesh_face_scale")
    return out


def mesh_neighbourhoods(c, f, vf, ni, mode, radius, cap):
    """Face neighbourhoods as a CSR (offsets int64 [nf+1], faces int64, rows ascending): mode 0 radius-based, 1
    vertex-based; cap int64 [nf] bounds every row's length from above (pcd_mesh_nbr_count / pcd_mesh_nbr_fill)."""
    nf, nv = f.size(0), ni.size(0) - 1
    assert _is(c, torch.float64, nf, 3) and _is(f, torch.int64, nf, 3) and _is(cap, torch.int64, nf)
    assert _is(vf, torch.int64, 3 * nf) and _is(ni, torch.int64, nv + 1)
    cap_off = torch.zeros(nf + 1, dtype=torch.int64, device=c.device)
    torch.cumsum(cap, 0, out=cap_off[1:])
    rows = torch.empty(int(cap_off[-1]) if nf else 0, dtype=torch.int64, device=c.device)
    counts = torch.empty(nf, dtype=torch.int64, device=c.device)
    check(lib().pcd_mesh_nbr_count(ptr(c), ptr(f), nf, ptr(vf), ptr(ni), nv, int(mode), float(radius), ptr(cap_off),
                                   ptr(rows), ptr(counts), c_void_p(stream_ptr())), "pcd_mesh_nbr_count")
    off = torch.zeros(nf + 1, dtype=torch.int64, device=c.device)
    torch.cumsum(counts, 0, out=off[1:])
    nbr = torch.empty(int(off[-1]) if nf else 0, dtype=torch.int64, device=c.device)
    check(lib().pcd_mesh_nbr_fill(ptr(rows), ptr(cap_off), ptr(off), nf, ptr(nbr), c_void_p(stream_ptr())),
          "pcd_mesh_nbr_fill")
    return off, nbr


def mesh_filter(c, area, guided, src, off, nbr, sigma_r, multiple_sigma_s, scale):
    """One filter pass; the precision follows c (float64 rows with an int64 CSR, or float32 rows with an int32 one)."""
    nf = c.size(0)
    fp32 = c.dtype == torch.float32
    dt, it = (torch.float32, torch.int32) if fp32 else (torch.float64, torch.int64)
    assert _is(c, dt, nf, 3) and _is(area, dt, nf) and _is(guided, dt, nf, 3) and _is(src, dt, nf, 3)
    assert _is(off, it, nf + 1) and nbr.dtype == it and nbr.is_contiguous() and _is(scale, torch.float64, 2)
    out = torch.empty_like(src)
    if fp32:
        check(lib().pcd_mesh_filter_f32(ptr(c), ptr(area), ptr(guided), ptr(src), nf, ptr(off), ptr(nbr), nbr.numel(),
                                        float(sigma_r), float(multiple_sigma_s), ptr(scale), ptr(out),
                                        c_void_p(stream_ptr())), "pcd_mesh_filter_f32")
    else:
        check(lib().pcd_mesh_filter(ptr(c), ptr(area), ptr(guided), ptr(src), nf, ptr(off), ptr(nbr), float(sigma_r),
                                    float(multiple_sigma_s), ptr(scale), ptr(out), c_void_p(stream_ptr())),
              "pcd_mesh_filter")
    return out


def mesh_denoise(v, f, vf, ni, off, nbr, guided, normal_iterations, vertex_iterations, sigma_r, multiple_sigma_s):
    """The whole loop in place on v (float64 + int64 topology, or float32 + int32); returns the last filtered normals.
    guided None: the input mesh's own face normals."""
    nf, nv = f.size(0), v.size(0)
    fp32 = v.dtype == torch.float32
    dt, it = (torch.float32, torch.int32) if fp32 else (torch.float64, torch.int64)
    assert _is(v, dt, nv, 3) and _is(f, it, nf, 3) and _is(vf, it, 3 * nf) and _is(ni, it, nv + 1)
    assert _is(off, it, nf + 1) and nbr.dtype == it and nbr.is_contiguous()
    assert guided is None or _is(guided, dt, nf, 3)
    out = torch.zeros((nf, 3), dtype=dt, device=v.device)
    if fp32:
        check(lib().pcd_mesh_denoise_f32(ptr(v), nv, ptr(f), nf, ptr(vf), ptr(ni), ptr(off), ptr(nbr), nbr.numel(),
                                         ptr(guided), int(normal_iterations), int(vertex_iterations), float(sigma_r),
                                         float(multiple_sigma_s), ptr(out), c_void_p(stream_ptr())),
              "pcd_mesh_denoise_f32")
    else:
        check(lib().pcd_mesh_denoise(ptr(v), nv, ptr(f), nf, ptr(vf), ptr(ni), ptr(off), ptr(nbr), ptr(guided),
                                     int(normal_iterations), int(vertex_iterations), float(sigma_r),
                                     float(multiple_sigma_s), ptr(out), c_void_p(stream_ptr())), "pcd_mesh_denoise")
    return out


# the GCN network input (PatchCollector.collectNetworkInput); every tensor on the device, contiguous
def mesh_tta(f: torch.Tensor, nv: int, out_dtype=torch.int64):
    """igl.triangle_triangle_adjacency(f)[0] on the device: [nf, 3] in out_dtype (int32 / int64), -1 = no neighbour."""
    f = on_device(f)
    assert f.dtype in (torch.int32, torch.int64) and f.dim() == 2 and f.size(1) == 3
    nf = f.size(0)
    tt = torch.empty((nf, 3), dtype=out_dtype, device=f.device)
    check(lib().pcd_mesh_tta(ptr(f), 32 if f.dtype == torch.int32 else 64, nf, int(nv), ptr(tt),
                             32 if out_dtype == torch.int32 else 64, c_void_p(stream_ptr())), "pcd_mesh_tta")
    return tt


def patch_radius(v, f, tt, faces, k, libm_pow=True):
    """(centre float64 [n,3], radius float64 [n]) of the patches of `faces` int64 [n] (pcd_patch_radius).
    libm_pow: the reference writes r = k * mean ** 0.5 on a numpy scalar, which is libm's pow(mean, 0.5) and differs
    from the correctly rounded root in the last bit now and then (2 of 640 faces of the shells fixture); to give the
    reference's r bit for bit the device's mean areas (8 bytes per face) make a round trip through the same libm call.
    False keeps the device's k * sqrt(mean) and the stage free of host work."""
    nv, nf, n = v.size(0), f.size(0), faces.size(0)
    assert _is(v, torch.float64, nv, 3) and _is(f, torch.int64, nf, 3) and _is(tt, torch.int64, nf, 3)
    assert _is(faces, torch.int64, n)
    centre = torch.empty((n, 3), dtype=torch.float64, device=v.device)
    r = torch.empty(n, dtype=torch.float64, device=v.device)
    mean = torch.empty(n, dtype=torch.float64, device=v.device) if libm_pow else None
    check(lib().pcd_patch_radius(ptr(v), nv, ptr(f), nf, ptr(tt), ptr(faces), n, float(k), ptr(centre), ptr(r),
                                 ptr(mean), c_void_p(stream_ptr())), "pcd_patch_radius")
    if libm_pow and n:
        host = mean.cpu()
        rh = torch.empty_like(host)
        check(lib().pcd_host_patch_radius(ptr(host), n, float(k), ptr(rh)), "pcd_host_patch_radius")
        r = rh.to(v.device)
    return centre, r


def patch_select(grid, widen, v, f, vf, ni, centre, r, out=None):
    """The patches as a CSR (offsets int64 [n+1], faces int64, rows ascending): every face with a vertex strictly
    inside the ball (centre[i], r[i]).  grid: a Grid over v rounded to float32, widen: a bound on that rounding (added
    to every radius when the cells to visit are chosen; membership is the exact float64 test).
    out: the buffer to fill (its length is the capacity; ValueError, nothing written, when the patches do not fit);
    None allocates the exact size (pcd_patch_select_count / pcd_patch_select_fill)."""
    nv, nf, n = v.size(0), f.size(0), r.size(0)
    assert _is(v, torch.float64, nv, 3) and _is(f, torch.int64, nf, 3)
    assert _is(vf, torch.int64, 3 * nf) and _is(ni, torch.int64, nv + 1)
    assert _is(centre, torch.float64, n, 3) and _is(r, torch.float64, n)
    head = (grid.handle, float(widen), ptr(v), nv, ptr(f), nf, ptr(vf), ptr(ni), ptr(centre), ptr(r), n)
    counts = torch.empty(n, dtype=torch.int64, device=v.device)
    check(lib().pcd_patch_select_count(*head, ptr(counts), c_void_p(stream_ptr())), "pcd_patch_select_count")
    off = torch.zeros(n + 1, dtype=torch.int64, device=v.device)
    torch.cumsum(counts, 0, out=off[1:])
    if out is None:
        out = torch.empty(int(off[-1]) if n else 0, dtype=torch.int64, device=v.device)
    assert out.dtype == torch.int64 and out.is_contiguous() and out.dim() == 1
    check(lib().pcd_patch_select_fill(*head, ptr(off), out.numel(), ptr(out), c_void_p(stream_ptr())),
          "pcd_patch_select_fill")
    return off, out


def patch_inputs(v, f, tt, vf, ni, faces, off, patch_faces, adjacency=False, dtype=torch.float64,
                 channels_first=False):
    """(inputs [n,64,20] (or [n,20,64]) in dtype, rotations float64 [n,3,3], centre_index int64 [n], eigenvalues
    float64 [n,3]) of the patches (off, patch_faces) of `faces` (pcd_patch_inputs)."""
    nv, nf, n = v.size(0), f.size(0), faces.size(0)
    assert dtype in (torch.float64, torch.float32)
    assert _is(v, torch.float64, nv, 3) and _is(f, torch.int64, nf, 3) and _is(tt, torch.int64, nf, 3)
    assert _is(vf, torch.int64, 3 * nf) and _is(ni, torch.int64, nv + 1)
    assert _is(faces, torch.int64, n) and _is(off, torch.int64, n + 1)
    assert patch_faces.dtype == torch.int64 and patch_faces.is_contiguous() and patch_faces.dim() == 1
    out = torch.empty((n, 20, 64) if channels_first else (n, 64, 20), dtype=dtype, device=v.device)
    rot = torch.empty((n, 3, 3), dtype=torch.float64, device=v.device)
    ci = torch.empty(n, dtype=torch.int64, device=v.device)
    eig = torch.empty((n, 3), dtype=torch.float64, device=v.device)
    check(lib().pcd_patch_inputs(ptr(v), nv, ptr(f), nf, ptr(tt), ptr(vf), ptr(ni), ptr(faces), n, ptr(off),
                                 ptr(patch_faces), patch_faces.numel(), int(bool(adjacency)),
                                 32 if dtype == torch.float32 else 64, int(bool(channels_first)), ptr(out), ptr(rot),
                                 ptr(ci), ptr(eig), c_void_p(stream_ptr())), "pcd_patch_inputs")
    return out, rot, ci, eig


def list_cap(k: int) -> int:
    """Columns of the fused loop's stored lists for k = max(k, k_update) (denoise.hip list_cap)."""
    return 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64


def fused_k_hint(k_max: int) -> int:
    """Cell size of the fused loop's snapshot index: about one list cap of points per occupied cell (k_hint = 2 x
    the cap) for the anchored searches (cap <= 32).  Measured at 10M points, k = 32 (cap 32), iterations 6-25: 8 points
    a cell 8.16 ms per iteration, 16 a cell 5.77 ms, 32 a cell 5.44 ms, 48 a cell 5.46 ms, 64 a cell 5.57 ms."""
    cap = list_cap(k_max)
    return 2 * cap if cap <= 32 else 0


def grid_params(xyz: torch.Tensor, k_hint: int = 16, cell: float = 0.0):
    """(origin (3,), cell edge) of the lattice pcd_grid_build would use for xyz."""
    x = f32(xyz)
    org = (ctypes.c_float * 3)()
    h = ctypes.c_float()
    check(lib().pcd_grid_params(ptr(x), x.size(0), int(k_hint), float(cell), org, ctypes.byref(h),
                                c_void_p(stream_ptr())), "pcd_grid_params")
    return [org[0], org[1], org[2]], h.value


def host_eigh3(t6):
    """CPU build of the kernels' eigen-decomposition: t6 (m, 6) float32 -> (w (m,3), v (m,3,3))."""
    import numpy as np
    t6 = np.ascontiguousarray(t6, dtype=np.float32)
    m = t6.shape[0]
    w = np.empty((m, 3), np.float32)
    v = np.empty((m, 3, 3), np.float32)
    check(lib().pcd_host_eigh3(t6.ctypes.data, m, w.ctypes.data, v.ctypes.data), "pcd_host_eigh3")
    return w, v


def host_vu_smooth(w, v, n, tau=0.3, damp=3.0):
    import numpy as np
    w = np.ascontiguousarray(w, np.float32); v = np.ascontiguousarray(v, np.float32)
    n = np.ascontiguousarray(n, np.float32)
    out = np.empty_like(n)
    check(lib().pcd_host_vu_smooth(w.ctypes.data, v.ctypes.data, n.ctypes.data, n.shape[0], float(tau), float(damp),
                                   out.ctypes.data), "pcd_host_vu_smooth")
    return out


def host_nvt_tensor(pos, n, ci, off, nbr, rho):
    """The fused kernels' NVT vote + tensor sums on the host (numpy in, (m, 6) float32 out)."""
    import numpy as np
    pos = np.ascontiguousarray(pos, np.float32); n = np.ascontiguousarray(n, np.float32)
    ci = np.ascontiguousarray(ci, np.int64); off = np.ascontiguousarray(off, np.int64)
    nbr = np.ascontiguousarray(nbr, np.int64)
    out = np.empty((len(ci), 6), np.float32)
    check(lib().pcd_host_nvt_tensor(pos.ctypes.data, n.ctypes.data, ci.ctypes.data, off.ctypes.data, nbr.ctypes.data,
                                    len(ci), float(rho), out.ctypes.data), "pcd_host_nvt_tensor")
    return out


def host_solve3(a, b):
    import numpy as np
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    x = np.zeros_like(b)
    ok = np.zeros(b.shape[0], np.int32)
    check(lib().pcd_host_solve3(a.ctypes.data, b.ctypes.data, b.shape[0], x.ctypes.data, ok.ctypes.data),
          "pcd_host_solve3")
    return x, ok.astype(bool)


def host_inv3(a):
    """torch.linalg.inv_ex's arithmetic for 3x3 as the position steps restate it (host build): (inverse, ok)."""
    import numpy as np
    a = np.ascontiguousarray(a, np.float32)
    x = np.zeros_like(a)
    ok = np.zeros(a.shape[0], np.int32)
    check(lib().pcd_host_inv3(a.ctypes.data, a.shape[0], x.ctypes.data, ok.ctypes.data), "pcd_host_inv3")
    return x, ok.astype(bool)


def host_step_csr(kind, pos, n, edge_vectors, ci, nbr, d, alpha, delta=0.0):
    """The kernels' Denoiser.*_step on the host (dense neighbour rows nbr [m, k]): out [m, 3]."""
    import numpy as np
    pos = np.ascontiguousarray(pos, np.float32); n = np.ascontiguousarray(n, np.float32)
    ev = None if edge_vectors is None else np.ascontiguousarray(edge_vectors, np.float32)
    ci = np.ascontiguousarray(ci, np.int64); nbr = np.ascontiguousarray(nbr, np.int64)
    m, k = nbr.shape
    off = np.arange(m + 1, dtype=np.int64) * k
    out = np.empty((m, 3), np.float32)
    check(lib().pcd_host_step_csr(int(kind), pos.ctypes.data, n.ctypes.data, None if ev is None else ev.ctypes.data,
                                  ci.ctypes.data, off.ctypes.data, nbr.ctypes.data, m, float(delta), float(d),
                                  float(alpha), out.ctypes.data), "pcd_host_step_csr")
    return out


def orient_normals_mst(pos_host, n_host, a_host, b_host):
    """Host (CPU) MST orientation; tensors must be contiguous CPU f32 / int64.  Modifies n_host in place."""
    assert not pos_host.is_cuda and not n_host.is_cuda
    check(lib().pcd_orient_normals_mst(ptr(pos_host), ptr(n_host), pos_host.size(0), ptr(a_host), ptr(b_host),
                                       a_host.size(0)), "pcd_orient_normals_mst")


def orient_normals_mst_gpu(pos, n, a, b) -> torch.Tensor:
    """Device MST orientation (Borůvka + Euler tour + sign pointer jumping), bit-identical to the host version.
    Returns the oriented normals as a new device f32 tensor; the inputs are not modified."""
    p = f32(pos)
    out = f32(n).clone()
    a = i64(a).reshape(-1)
    b = i64(b).reshape(-1)
    assert p.dim() == 2 and p.size(1) == 3 and out.shape == p.shape and a.numel() == b.numel()
    check(lib().pcd_orient_normals_mst_gpu(ptr(p), ptr(out), p.size(0), ptr(a), ptr(b), a.numel(),
                                           c_void_p(stream_ptr())), "pcd_orient_normals_mst_gpu")
    return out


# ----------------------------------------------------------------------------------------------- DGCNN forward
DGCNN_CIN = (17, 64, 64, 128, 256, 256)
DGCNN_COUT = (64, 64, 128, 256, 256, 256)
EPI_PLAIN, EPI_AFFINE_LRELU, EPI_POOL, EPI_AFFINE, EPI_ADD = range(5)
host_packs = 0                       # how often Dgcnn() packed a model's weights through the host (pcd_dgcnn_create)
DGCNN_NO_BAD_PATCH = 0x7f7f7f7f      # PCD_DGCNN_NO_BAD_PATCH
OPERANDS = {"fp32": 0, "bf16": 1}    # PCD_OPERANDS_*


def operands_code(operands, what="pcd") -> int:
    """"fp32" / "bf16" -> PCD_OPERANDS_*; ValueError for anything else."""
    if not isinstance(operands, str) or operands not in OPERANDS:
        raise ValueError(f'{what}: operands must be "fp32" or "bf16", got {operands!r}')
    return OPERANDS[operands]


class DgcnnTable:
    """The layer table of a network (pcd_dgcnn_table): l_e static edge convolutions, l_d dynamic ones, l_l linears,
    the l_e + l_d + l_l channel sizes, k, init_dims, output_channels -- BetterDGCNN's constructor arguments
    (GCNModel.py:217-256).  Refuses, naming the argument, what the reference cannot build or the kernels do not index
    (the bounds of include/pcd.h).  `fixed(k, emb_dims, output_channels)` is DGCNN's table."""
    MAX_EDGE_LAYERS, MAX_LINEARS, MAX_EDGE_WIDTH, MAX_WIDTH = 16, 16, 4096, 65536

    def __init__(self, l_e, l_d, l_l, channel_sizes, k, init_dims=17, output_channels=3, what="BetterDGCNN"):
        if isinstance(channel_sizes, torch.Tensor):
            if channel_sizes.dim() != 1 or channel_sizes.dtype.is_floating_point or channel_sizes.dtype == torch.bool:
                raise ValueError(f"{what}: channel_sizes must be a 1-D integer tensor or a sequence of ints")
            sizes = [int(v) for v in channel_sizes.tolist()]
        else:
            sizes = list(channel_sizes)
            if any(int(v) != v for v in sizes):
                raise ValueError(f"{what}: channel_sizes must hold integers, got {sizes}")
            sizes = [int(v) for v in sizes]
        for name, v in (("l_e", l_e), ("l_d", l_d), ("l_l", l_l), ("k", k), ("init_dims", init_dims),
                        ("output_channels", output_channels)):
            if int(v) != v:
                raise ValueError(f"{what}: {name} must be an integer, got {v!r}")
        l_e, l_d, l_l = int(l_e), int(l_d), int(l_l)
        if l_e < 0 or l_d < 0 or not 1 <= l_e + l_d <= self.MAX_EDGE_LAYERS:
            raise ValueError(f"{what}: l_e + l_d must be in [1, {self.MAX_EDGE_LAYERS}] (without an edge layer there is "
                             f"nothing to concatenate), got l_e = {l_e}, l_d = {l_d}")
        if not 2 <= l_l <= self.MAX_LINEARS:
            raise ValueError(f"{what}: l_l must be in [2, {self.MAX_LINEARS}] (the last linear reads channel_sizes[-1], "
                             f"a hidden width), got {l_l}")
        if len(sizes) != l_e + l_d + l_l:
            raise ValueError(f"{what}: channel_sizes must have l_e + l_d + l_l = {l_e + l_d + l_l} entries, got {len(sizes)}")
        for i, v in enumerate(sizes):
            lim = self.MAX_EDGE_WIDTH if i < l_e + l_d else self.MAX_WIDTH
            if not 1 <= v <= lim:
                raise ValueError(f"{what}: channel_sizes[{i}] must be in [1, {lim}], got {v}")
        if not 1 <= int(k) <= 64:
            raise ValueError(f"{what}: k must be in [1, 64], got {k}")
        if int(init_dims) != 17:
            raise ValueError(f"{what}: init_dims must be 17 (forward takes rows 0:17 of its input), got {init_dims}")
        if not 1 <= int(output_channels) <= 4096:
            raise ValueError(f"{what}: output_channels must be in [1, 4096], got {output_channels}")
        self.l_e, self.l_d, self.l_l, self.sizes = l_e, l_d, l_l, tuple(sizes)
        self.k, self.init_dims, self.output_channels = int(k), int(init_dims), int(output_channels)
        E = self.n_edge = l_e + l_d
        self.cin = (17,) + self.sizes[:E - 1]          # (in, out) of the edge convolutions
        self.cout = self.sizes[:E]
        self.cat_off = tuple(sum(self.cout[:i]) for i in range(E + 1))
        self.ccat = self.cat_off[-1]
        self.emb = self.sizes[E]                        # the pooled convolution's width
        self.head = self.sizes[E + 1:]                  # the l_l - 1 hidden widths
        self._sizes_c = (ctypes.c_int32 * len(sizes))(*sizes)
        self.struct = DgcnnTableStruct(l_e, l_d, l_l, ctypes.cast(self._sizes_c, _I32P), self.k, self.init_dims,
                                       self.output_channels)

    @classmethod
    def fixed(cls, k, emb_dims, output_channels=3):
        if int(emb_dims) != emb_dims or not 1 <= int(emb_dims) <= cls.MAX_WIDTH:
            raise ValueError(f"DGCNN: emb_dims must be an integer in [1, {cls.MAX_WIDTH}], got {emb_dims!r}")
        return cls(3, 3, 4, DGCNN_COUT + (int(emb_dims), 512, 256, 64), k, 17, output_channels, what="DGCNN")

    def conv_shapes(self):
        """[rows, cols] of the l_e + l_d + 1 convolution weights."""
        return [(co, 2 * ci) for ci, co in zip(self.cin, self.cout)] + [(self.emb, self.ccat)]

    def list_len(self, layer):
        """The neighbour list length of edge layer `layer` (0-based)."""
        return 3 if layer < self.l_e else self.k

    def byref(self):
        return ctypes.byref(self.struct)


def _voidp_array(values):
    return (c_void_p * len(values))(*values)


class Dgcnn:
    """Packed device weights of one DGCNN (pcd_dgcnn) and its forward.

    conv: 7 weights [out, 2 in] (conv7 [emb, 1024]); bn: 10 tuples (weight, bias, running_mean, running_var, eps);
    lin: 4 tuples (weight [out, in], bias or None).  The tensors may live on the host or the device (float32); they
    are copied."""
    _NAME = "DGCNN"

    def __init__(self, conv, bn, lin, k, init_dims, emb_dims, output_channels=3):
        if len(conv) != 7 or len(bn) != 10 or len(lin) != 4:
            raise ValueError("pcd: Dgcnn takes 7 convolution weights, 10 batch norms and 4 linears")
        w = DgcnnWeights()
        keep = self._fill(w, conv, bn, lin)
        global host_packs
        host_packs += 1
        h = c_void_p()
        device()
        check(lib().pcd_dgcnn_create(ctypes.byref(w), int(k), int(init_dims), int(emb_dims), int(output_channels),
                                     ctypes.byref(h)), "pcd_dgcnn_create")
        del keep
        self.handle = h
        self.k, self.emb_dims, self.output_channels = int(k), int(emb_dims), int(output_channels)
        self.table = DgcnnTable.fixed(k, emb_dims, output_channels)

    @staticmethod
    def _fill(w, conv, bn, lin):
        """Writes the pointers and shapes of the weights into the (array or pointer) fields of `w`; returns what must
        stay alive until the library has copied them."""
        keep = []

        def p32(t):
            t = t.detach()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        for i, cw in enumerate(conv):
            cw2 = cw.reshape(cw.shape[0], -1)
            w.conv_w[i], w.conv_rows[i], w.conv_cols[i] = p32(cw2), cw2.shape[0], cw2.shape[1]
        for i, (g, be, mu, var, eps) in enumerate(bn):
            if not (g.numel() == be.numel() == mu.numel() == var.numel()):
                raise ValueError(f"pcd: bn{i + 1}: weight, bias, running_mean and running_var differ in length")
            w.bn_weight[i], w.bn_bias[i], w.bn_mean[i], w.bn_var[i] = p32(g), p32(be), p32(mu), p32(var)
            w.bn_eps[i], w.bn_len[i] = float(eps), g.numel()
        for i, (lw, lb) in enumerate(lin):
            if lw.dim() != 2 or (lb is not None and lb.numel() != lw.shape[0]):
                raise ValueError(f"pcd: linear{i + 1}: weight must be [out, in] and the bias [out]")
            w.lin_w[i], w.lin_rows[i], w.lin_cols[i] = p32(lw), lw.shape[0], lw.shape[1]
            w.lin_b[i] = None if lb is None else p32(lb)
        return keep

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value and _lib is not None:
            _lib.pcd_dgcnn_destroy(h)
            self.handle = None

    def set_operands(self, operands: str):
        """"bf16": the trunk's GEMMs (edge layers with Cin >= 32, the pooled convolution) take bf16 operands and
        accumulate in float32; "fp32": the default (pcd_dgcnn_set_operands).  The first switch to bf16 rounds the
        packed weights, synchronously."""
        check(lib().pcd_dgcnn_set_operands(self.handle, operands_code(operands, f"pcd: {self._NAME}")),
              "pcd_dgcnn_set_operands")

    @property
    def operands(self) -> str:
        v = c_int(0)
        check(lib().pcd_dgcnn_operands(self.handle, ctypes.byref(v)), "pcd_dgcnn_operands")
        return {c: n for n, c in OPERANDS.items()}[v.value]

    def workspace_bytes(self, b: int) -> int:
        v = c_int64(0)
        check(lib().pcd_dgcnn_workspace_bytes(self.handle, int(b), ctypes.byref(v)), "pcd_dgcnn_workspace_bytes")
        return v.value

    def workspace(self, b: int) -> torch.Tensor:
        return torch.empty(max(self.workspace_bytes(b), 1), dtype=torch.uint8, device=device())

    def _debug_tensors(self, b, dev):
        t = self.table
        d = {"cat": torch.empty((b, t.ccat, 64), dtype=torch.float32, device=dev),
             "lists": torch.empty((t.l_d, b, 64, t.k), dtype=torch.int32, device=dev),
             "pooled": torch.empty((b, 2 * t.emb), dtype=torch.float32, device=dev)}
        for j, width in enumerate(t.head, start=1):
            d[f"h{j}"] = torch.empty((width, b), dtype=torch.float32, device=dev)
        return d

    def _debug(self, b, dev):
        """(the tensors the debug struct fills, the struct, what the struct points to)"""
        d = self._debug_tensors(b, dev)
        return d, DgcnnDebug(*[d[n].data_ptr() for n in ("cat", "lists", "pooled", "h1", "h2", "h3")]), None

    def _forward_entries(self):
        return (lib().pcd_dgcnn_forward, "pcd_dgcnn_forward", lib().pcd_dgcnn_forward_deferred,
                "pcd_dgcnn_forward_deferred")

    def forward(self, inputs: torch.Tensor, workspace: torch.Tensor = None, debug: bool = False,
                first_bad: torch.Tensor = None, patch_base: int = 0):
        """inputs [b, 20, 64] float32 on the device -> out [b, output_channels]; with debug also a dict of the
        intermediate tensors (pcd_dgcnn_debug).  workspace: a contiguous device tensor of workspace_bytes(b) bytes or
        more, on the inputs' device.  first_bad: None -- a bad index column raises ValueError (one stream synchronise
        per call); or an int32 [1] device tensor holding DGCNN_NO_BAD_PATCH -- nothing waits for the device, and the
        tensor takes the lowest patch_base + patch with a bad index column (pcd_dgcnn_forward_deferred)."""
        x = f32(inputs)
        if x.dim() != 3 or x.size(1) != 20 or x.size(2) != 64:
            raise ValueError(f"pcd: {self._NAME} inputs must be [b, 20, 64], got {tuple(inputs.shape)}")
        b, dev = x.size(0), x.device
        ws = self.workspace(b) if workspace is None else workspace
        if not isinstance(ws, torch.Tensor) or ws.device != dev or not ws.is_contiguous():
            raise ValueError(f"pcd: {self._NAME} workspace must be a contiguous tensor on {dev}, got "
                             f"{getattr(ws, 'device', type(ws).__name__)}")
        if first_bad is not None and (not isinstance(first_bad, torch.Tensor) or first_bad.device != dev
                                      or first_bad.dtype != torch.int32 or first_bad.numel() != 1):
            raise ValueError(f"pcd: {self._NAME} first_bad must be an int32 tensor of one element on {dev}")
        out = torch.empty((b, self.output_channels), dtype=torch.float32, device=dev)
        dbg, d, held = None, None, None
        if debug:
            d, dbg, held = self._debug(b, dev)
        dbg_ref = None if dbg is None else ctypes.byref(dbg)
        fwd, fwd_name, deferred, deferred_name = self._forward_entries()
        if first_bad is None:
            check(fwd(self.handle, ptr(x), b, ptr(out), ptr(ws), ws.numel() * ws.element_size(), dbg_ref,
                      c_void_p(stream_ptr())), fwd_name)
        else:
            check(deferred(self.handle, ptr(x), b, ptr(out), ptr(ws), ws.numel() * ws.element_size(), dbg_ref,
                           ptr(first_bad), int(patch_base), c_void_p(stream_ptr())), deferred_name)
        del held
        return (out, d) if debug else out

    def edgeconv(self, layer: int, x: torch.Tensor, lists: torch.Tensor) -> torch.Tensor:
        """Edge layer `layer` (1-based) on x [b, Cin, 64] with neighbour lists int32 [b, 64, n] -> [b, Cout, 64]
        (pcd_dgcnn_edgeconv)."""
        t = self.table
        if not 1 <= int(layer) <= t.n_edge:
            raise ValueError(f"pcd: {self._NAME} edge layers are 1-{t.n_edge}")
        x, lists = f32(x), on_device(lists, torch.int32)
        b = x.size(0)
        if tuple(x.shape) != (b, t.cin[layer - 1], 64) or lists.dim() != 3 or tuple(lists.shape[:2]) != (b, 64):
            raise ValueError(f"pcd: edgeconv layer {layer}: x {tuple(x.shape)} / lists {tuple(lists.shape)} do not fit")
        out = torch.empty((b, t.cout[layer - 1], 64), dtype=torch.float32, device=x.device)
        check(lib().pcd_dgcnn_edgeconv(self.handle, int(layer), ptr(x), b, ptr(lists), lists.size(2), ptr(out),
                                       c_void_p(stream_ptr())), "pcd_dgcnn_edgeconv")
        return out


class BetterDgcnn(Dgcnn):
    """Packed device weights of one BetterDGCNN (pcd_bdgcnn_create) and its forward: Dgcnn with the layer table from
    the caller.  table: a DgcnnTable; conv: l_e + l_d + 1 weights; bn: l_e + l_d + l_l tuples; lin: l_l tuples."""
    _NAME = "BetterDGCNN"

    def __init__(self, table: DgcnnTable, conv, bn, lin):
        if len(conv) != table.n_edge + 1 or len(bn) != table.n_edge + table.l_l or len(lin) != table.l_l:
            raise ValueError(f"pcd: BetterDgcnn takes {table.n_edge + 1} convolution weights, "
                             f"{table.n_edge + table.l_l} batch norms and {table.l_l} linears")
        w, arrays = BdgcnnWeights(), []
        for name, typ in BdgcnnWeights._fields_:        # the pointer fields' arrays, of the table's lengths
            n = len(conv) if name.startswith("conv") else len(bn) if name.startswith("bn") else len(lin)
            arrays.append((typ._type_ * n)())
            setattr(w, name, ctypes.cast(arrays[-1], typ))
        keep = self._fill(w, conv, bn, lin) + arrays
        global host_packs
        host_packs += 1
        h = c_void_p()
        device()
        check(lib().pcd_bdgcnn_create(table.byref(), ctypes.byref(w), ctypes.byref(h)), "pcd_bdgcnn_create")
        del keep
        self.handle = h
        self.table = table
        self.k, self.emb_dims, self.output_channels = table.k, table.emb, table.output_channels

    def _debug(self, b, dev):
        d = self._debug_tensors(b, dev)
        hs = _voidp_array([d[f"h{j}"].data_ptr() for j in range(1, len(self.table.head) + 1)])
        return d, BdgcnnDebug(d["cat"].data_ptr(), d["lists"].data_ptr(), d["pooled"].data_ptr(),
                              ctypes.cast(hs, _VPP)), hs

    def _forward_entries(self):
        return (lib().pcd_bdgcnn_forward, "pcd_bdgcnn_forward", lib().pcd_bdgcnn_forward_deferred,
                "pcd_bdgcnn_forward_deferred")


FUSED_OFF, FUSED_ON, FUSED_AUTO = range(3)       # PCD_FUSED_*


def bdgcnn_edgeconv_scratch_bytes(c_in: int, c_out: int, b: int) -> int:
    v = c_int64(0)
    check(lib().pcd_bdgcnn_edgeconv_scratch_bytes(int(c_in), int(c_out), int(b), ctypes.byref(v)),
          "pcd_bdgcnn_edgeconv_scratch_bytes")
    return v.value


def bdgcnn_edgeconv(w, s, t, x, lists, fused: int = FUSED_AUTO, scratch=None, out=None, operands: str = "fp32"):
    """One edge layer in eval() by its shapes (pcd_bdgcnn_edgeconv): w [Cout, 2 Cin], the folded batch norm s, t
    [Cout], x [b, Cin, 64], lists int32 [b, 64, n] -> [b, Cout, 64].  fused: FUSED_OFF (GEMM, then the max over the
    lists), FUSED_ON (one kernel, 2 Cout <= 128 only) or FUSED_AUTO (the library's choice); the bits are the same.
    scratch: None, or a contiguous device tensor of bdgcnn_edgeconv_scratch_bytes(Cin, Cout, b) bytes -- then nothing
    is allocated and nothing waits for the device; out: None or the float32 [b, Cout, 64] tensor to write.
    operands = "bf16": the product on the bf16 kernel, whatever Cin is (pcd_bdgcnn_edgeconv_bf16)."""
    bf16 = operands_code(operands, "pcd: bdgcnn_edgeconv") == OPERANDS["bf16"]
    w, s, t, x, lists = f32(w), f32(s), f32(t), f32(x), on_device(lists, torch.int32)
    w = w.reshape(w.shape[0], -1)
    b, cout = x.size(0), w.size(0)
    if x.dim() != 3 or x.size(2) != 64 or w.size(1) != 2 * x.size(1) or s.numel() != cout or t.numel() != cout \
            or lists.dim() != 3 or tuple(lists.shape[:2]) != (b, 64):
        raise ValueError(f"pcd: bdgcnn_edgeconv: w {tuple(w.shape)} / x {tuple(x.shape)} / lists {tuple(lists.shape)} "
                         "do not fit")
    if scratch is not None and (not isinstance(scratch, torch.Tensor) or scratch.device != x.device
                                or not scratch.is_contiguous()):
        raise ValueError(f"pcd: bdgcnn_edgeconv: scratch must be a contiguous tensor on {x.device}")
    if out is None:
        out = torch.empty((b, cout, 64), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (b, cout, 64) or out.device != x.device \
            or not out.is_contiguous():
        raise ValueError(f"pcd: bdgcnn_edgeconv: out must be float32 [{b}, {cout}, 64] contiguous on {x.device}")
    nbytes = 0 if scratch is None else scratch.numel() * scratch.element_size()
    entry, name = ((lib().pcd_bdgcnn_edgeconv_bf16, "pcd_bdgcnn_edgeconv_bf16") if bf16 else
                   (lib().pcd_bdgcnn_edgeconv, "pcd_bdgcnn_edgeconv"))
    check(entry(ptr(w), ptr(s), ptr(t), x.size(1), cout, ptr(x), b, ptr(lists), lists.size(2), int(fused), ptr(out),
                ptr(scratch), nbytes, c_void_p(stream_ptr())), name)
    return out


def dgcnn_knn(x: torch.Tensor, k: int) -> torch.Tensor:
    """x [b, C, 64] -> int32 [b, 64, k]: each row's k nearest rows in feature space (pcd_dgcnn_knn)."""
    x = f32(x)
    if x.dim() != 3 or x.size(2) != 64:
        raise ValueError(f"pcd: dgcnn_knn takes [b, C, 64], got {tuple(x.shape)}")
    lists = torch.empty((x.size(0), 64, int(k)), dtype=torch.int32, device=x.device)
    check(lib().pcd_dgcnn_knn(ptr(x), x.size(0), x.size(1), int(k), ptr(lists), c_void_p(stream_ptr())),
          "pcd_dgcnn_knn")
    return lists


def dgcnn_gemm(w: torch.Tensor, x: torch.Tensor, epilogue: int = EPI_PLAIN, s=None, t=None, y=None) -> torch.Tensor:
    """w [M, K] . x on the network's MFMA GEMM (pcd_dgcnn_gemm): x [b, K, 64] -> [b, M, 64] ([b, 2 M] with the
    pooling epilogue), or x [K, b] -> [M, b].  EPI_ADD adds the product into y (float32, contiguous, on the device)
    and returns it."""
    w, x = f32(w), f32(x)
    M, K = w.shape
    if x.dim() == 3:
        b, nodes = x.size(0), 64
        if tuple(x.shape) != (b, K, 64):
            raise ValueError(f"pcd: dgcnn_gemm: x {tuple(x.shape)} does not fit w {tuple(w.shape)}")
        shape = (b, 2 * M) if epilogue == EPI_POOL else (b, M, 64)
    else:
        b, nodes = x.size(1), 1
        if x.dim() != 2 or x.size(0) != K:
            raise ValueError(f"pcd: dgcnn_gemm: x {tuple(x.shape)} does not fit w {tuple(w.shape)}")
        shape = (M, b)
    s = None if s is None else f32(s)
    t = None if t is None else f32(t)
    if epilogue == EPI_ADD:
        if not isinstance(y, torch.Tensor) or y.dtype != torch.float32 or y.device != x.device \
                or tuple(y.shape) != shape or not y.is_contiguous():
            raise ValueError(f"pcd: dgcnn_gemm: EPI_ADD needs y float32 {shape} contiguous on {x.device}")
    elif y is not None:
        raise ValueError("pcd: dgcnn_gemm: y is taken by EPI_ADD only")
    else:
        y = torch.empty(shape, dtype=torch.float32, device=x.device)
    check(lib().pcd_dgcnn_gemm(ptr(w), ptr(x), M, K, b, nodes, int(epilogue), ptr(s), ptr(t), ptr(y),
                               c_void_p(stream_ptr())), "pcd_dgcnn_gemm")
    return y


def dgcnn_gemm_bf16(w: torch.Tensor, x: torch.Tensor, epilogue: int = EPI_PLAIN, s=None, t=None) -> torch.Tensor:
    """dgcnn_gemm for x [b, K, 64] on the bf16 kernel (pcd_dgcnn_gemm_bf16): float32 w and x are rounded to bf16 as the
    forward in bf16 mode rounds them, the products accumulated in float32.  Epilogues 0-3."""
    w, x = f32(w), f32(x)
    M, K = w.shape
    b = x.size(0)
    if x.dim() != 3 or tuple(x.shape) != (b, K, 64):
        raise ValueError(f"pcd: dgcnn_gemm_bf16: x {tuple(x.shape)} does not fit w {tuple(w.shape)}")
    s = None if s is None else f32(s)
    t = None if t is None else f32(t)
    y = torch.empty((b, 2 * M) if epilogue == EPI_POOL else (b, M, 64), dtype=torch.float32, device=x.device)
    check(lib().pcd_dgcnn_gemm_bf16(ptr(w), ptr(x), M, K, b, int(epilogue), ptr(s), ptr(t), ptr(y),
                                    c_void_p(stream_ptr())), "pcd_dgcnn_gemm_bf16")
    return y


# ----------------------------------------------------------------------------------------------- DGCNN training
def dgcnn_train_workspace_bytes(k: int, emb_dims: int, b: int) -> int:
    v = c_int64(0)
    check(lib().pcd_dgcnn_train_workspace_bytes(int(k), int(emb_dims), int(b), ctypes.byref(v)),
          "pcd_dgcnn_train_workspace_bytes")
    return v.value


def _train_tensor(t, what, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"pcd: DGCNN training: {what} must be a contiguous {dtype} tensor on the HIP device")
    return t.data_ptr()


def _train_workspace(ws, dev):
    if not isinstance(ws, torch.Tensor) or ws.device != dev or not ws.is_contiguous():
        raise ValueError(f"pcd: DGCNN training workspace must be a contiguous tensor on {dev}, got "
                         f"{getattr(ws, 'device', type(ws).__name__)}")
    return ws.numel() * ws.element_size()


def _train_params(table, conv, bn, inputs):
    """The checks of a train-mode forward; -> (b, device, the eight per-layer lists of pcd_*_train_params)."""
    n = table.n_edge + 1
    if len(conv) != n or len(bn) != n:
        raise ValueError(f"pcd: DGCNN training takes {n} convolution weights and {n} batch norms")
    x = inputs
    _train_tensor(x, "inputs")
    if x.dim() != 3 or x.size(1) != 20 or x.size(2) != 64:
        raise ValueError(f"pcd: DGCNN inputs must be [b, 20, 64], got {tuple(x.shape)}")
    cols = {key: [] for key in ("conv_w", "bn_weight", "bn_bias", "bn_mean", "bn_var", "bn_tracked", "bn_eps",
                                "bn_momentum")}
    shapes = table.conv_shapes()
    for i, cw in enumerate(conv):
        rows, width = shapes[i]
        if cw.numel() != rows * width or cw.shape[0] != rows:
            raise ValueError(f"pcd: conv{i + 1} weight must be [{rows}, {width}], got {tuple(cw.shape)}")
        cols["conv_w"].append(_train_tensor(cw, f"conv{i + 1} weight"))
    for i, (g, be, mu, var, nbt, eps, mom) in enumerate(bn):
        if mom is None:
            raise ValueError(f"pcd: bn{i + 1}: momentum=None (a cumulative average) is not supported in training")
        for t, what in ((g, "weight"), (be, "bias"), (mu, "running_mean"), (var, "running_var")):
            if t is not None and t.numel() != shapes[i][0]:
                raise ValueError(f"pcd: bn{i + 1}.{what} must have {shapes[i][0]} channels")
        cols["bn_weight"].append(_train_tensor(g, f"bn{i + 1}.weight"))
        cols["bn_bias"].append(_train_tensor(be, f"bn{i + 1}.bias"))
        cols["bn_mean"].append(None if mu is None else _train_tensor(mu, f"bn{i + 1}.running_mean"))
        cols["bn_var"].append(None if var is None else _train_tensor(var, f"bn{i + 1}.running_var"))
        cols["bn_tracked"].append(None if nbt is None else
                                  _train_tensor(nbt, f"bn{i + 1}.num_batches_tracked", torch.int64))
        cols["bn_eps"].append(float(eps))
        cols["bn_momentum"].append(float(mom))
    return x.size(0), x.device, cols


def _pointer_struct(struct, cols):
    """A struct of pointer fields over arrays made from `cols` {field: list}; -> (struct, the arrays to keep alive)."""
    keep = []
    for name, values in cols.items():
        typ = c_double if name in ("bn_eps", "bn_momentum") else c_void_p
        arr = (typ * len(values))(*values)
        keep.append(arr)
        setattr(struct, name, ctypes.cast(arr, POINTER(typ)))
    return struct, keep


def dgcnn_train_forward(conv, bn, k: int, emb_dims: int, inputs: torch.Tensor, workspace: torch.Tensor,
                        want_lists: bool = False):
    """conv1-7 and the pooling in train() (pcd_dgcnn_train_forward).  conv: 7 weights [out, 2 in(, 1, 1)]; bn: 7 tuples
    (weight, bias, running_mean, running_var, num_batches_tracked, eps, momentum) whose buffers (None: none) are
    updated in place -- all float32 (the counter int64), contiguous, on the device: nothing is copied.  inputs
    [b, 20, 64] float32 -> pooled [b, 2 emb]; with want_lists also the lists of layers 4-6, int32 [3, b, 64, k].  The
    workspace (dgcnn_train_workspace_bytes) carries the forward's state to dgcnn_train_backward."""
    if len(conv) != 7 or len(bn) != 7:
        raise ValueError("pcd: DGCNN training takes 7 convolution weights and 7 batch norms")
    b, dev, cols = _train_params(DgcnnTable.fixed(k, emb_dims), conv, bn, inputs)
    prm = DgcnnTrainParams()
    for name, values in cols.items():
        for i, v in enumerate(values):
            getattr(prm, name)[i] = v
    nbytes = _train_workspace(workspace, dev)
    pooled = torch.empty((b, 2 * int(emb_dims)), dtype=torch.float32, device=dev)
    lists = torch.empty((3, b, 64, int(k)), dtype=torch.int32, device=dev) if want_lists else None
    check(lib().pcd_dgcnn_train_forward(ctypes.byref(prm), int(k), int(emb_dims), ptr(inputs), b, ptr(pooled),
                                        ptr(workspace), nbytes, ptr(lists), c_void_p(stream_ptr())),
          "pcd_dgcnn_train_forward")
    return (pooled, lists) if want_lists else pooled


def _train_grads(conv, inputs, d_pooled, emb):
    x = inputs
    _train_tensor(x, "inputs")
    b, dev = x.size(0), x.device
    dp = f32(d_pooled)
    if tuple(dp.shape) != (b, 2 * int(emb)):
        raise ValueError(f"pcd: d_pooled must be [{b}, {2 * int(emb)}], got {tuple(dp.shape)}")
    dw = [torch.empty_like(cw, memory_format=torch.contiguous_format) for cw in conv]
    dg = [torch.empty(cw.shape[0], dtype=torch.float32, device=dev) for cw in conv]
    db = [torch.empty(cw.shape[0], dtype=torch.float32, device=dev) for cw in conv]
    return b, dev, dp, dw, dg, db


def dgcnn_train_backward(conv, k: int, emb_dims: int, inputs: torch.Tensor, d_pooled: torch.Tensor,
                         workspace: torch.Tensor):
    """d_pooled [b, 2 emb] -> (7 conv weight gradients shaped like conv, 7 bn weight gradients, 7 bn bias gradients)
    from the workspace dgcnn_train_forward left (pcd_dgcnn_train_backward).  One backward per forward."""
    b, dev, dp, dw, dg, db = _train_grads(conv, inputs, d_pooled, emb_dims)
    g = DgcnnTrainGrads()
    for i in range(7):
        g.conv_w[i], g.bn_weight[i], g.bn_bias[i] = dw[i].data_ptr(), dg[i].data_ptr(), db[i].data_ptr()
    check(lib().pcd_dgcnn_train_backward(int(k), int(emb_dims), ptr(inputs), b, ptr(dp),
                                         c_void_p(_train_tensor(conv[6], "conv7 weight")),
                                         ptr(workspace), _train_workspace(workspace, dev), ctypes.byref(g),
                                         c_void_p(stream_ptr())), "pcd_dgcnn_train_backward")
    return dw, dg, db


def bdgcnn_train_workspace_bytes(table: DgcnnTable, b: int) -> int:
    v = c_int64(0)
    check(lib().pcd_bdgcnn_train_workspace_bytes(table.byref(), int(b), ctypes.byref(v)),
          "pcd_bdgcnn_train_workspace_bytes")
    return v.value


def bdgcnn_train_forward(table: DgcnnTable, conv, bn, inputs: torch.Tensor, workspace: torch.Tensor,
                         want_lists: bool = False):
    """dgcnn_train_forward for a table from the caller (pcd_bdgcnn_train_forward): conv and bn hold l_e + l_d + 1
    entries; -> pooled [b, 2 C]; with want_lists also the dynamic layers' lists, int32 [l_d, b, 64, k]."""
    b, dev, cols = _train_params(table, conv, bn, inputs)
    prm, keep = _pointer_struct(BdgcnnTrainParams(), cols)
    nbytes = _train_workspace(workspace, dev)
    pooled = torch.empty((b, 2 * table.emb), dtype=torch.float32, device=dev)
    lists = torch.empty((table.l_d, b, 64, table.k), dtype=torch.int32, device=dev) if want_lists else None
    check(lib().pcd_bdgcnn_train_forward(table.byref(), ctypes.byref(prm), ptr(inputs), b, ptr(pooled), ptr(workspace),
                                         nbytes, ptr(lists), c_void_p(stream_ptr())), "pcd_bdgcnn_train_forward")
    del keep
    return (pooled, lists) if want_lists else pooled


def bdgcnn_train_backward(table: DgcnnTable, conv, inputs: torch.Tensor, d_pooled: torch.Tensor,
                          workspace: torch.Tensor):
    """dgcnn_train_backward for a table from the caller (pcd_bdgcnn_train_backward)."""
    if len(conv) != table.n_edge + 1:
        raise ValueError(f"pcd: DGCNN training takes {table.n_edge + 1} convolution weights")
    b, dev, dp, dw, dg, db = _train_grads(conv, inputs, d_pooled, table.emb)
    g, keep = _pointer_struct(BdgcnnTrainGrads(), {"conv_w": [t.data_ptr() for t in dw],
                                                   "bn_weight": [t.data_ptr() for t in dg],
                                                   "bn_bias": [t.data_ptr() for t in db]})
    check(lib().pcd_bdgcnn_train_backward(table.byref(), ptr(inputs), b, ptr(dp),
                                          c_void_p(_train_tensor(conv[-1], "the pooled convolution's weight")),
                                          ptr(workspace), _train_workspace(workspace, dev), ctypes.byref(g),
                                          c_void_p(stream_ptr())), "pcd_bdgcnn_train_backward")
    del keep
    return dw, dg, db


def dgcnn_wgrad_split(b: int) -> int:
    """Patches per run of the weight gradient's split reduction (pcd_dgcnn_wgrad_split)."""
    v = c_int64(0)
    check(lib().pcd_dgcnn_wgrad_split(int(b), ctypes.byref(v)), "pcd_dgcnn_wgrad_split")
    return v.value


def dgcnn_wgrad(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """dy [b, M, 64], x [b, K, 64] -> dw [M, K] = sum over the b x 64 columns of dy x^T (pcd_dgcnn_wgrad)."""
    dy, x = f32(dy), f32(x)
    if dy.dim() != 3 or x.dim() != 3 or dy.size(0) != x.size(0) or dy.size(2) != 64 or x.size(2) != 64:
        raise ValueError(f"pcd: dgcnn_wgrad: dy {tuple(dy.shape)} / x {tuple(x.shape)} do not fit")
    dw = torch.empty((dy.size(1), x.size(1)), dtype=torch.float32, device=x.device)
    check(lib().pcd_dgcnn_wgrad(ptr(dy), ptr(x), dy.size(1), x.size(1), x.size(0), ptr(dw), c_void_p(stream_ptr())),
          "pcd_dgcnn_wgrad")
    return dw


def _edge_train_args(layer, w, x, lists):
    if not 1 <= int(layer) <= 6:
        raise ValueError("pcd: DGCNN edge layers are 1-6")
    cin, cout = DGCNN_CIN[layer - 1], DGCNN_COUT[layer - 1]
    w, x, lists = f32(w).reshape(w.shape[0], -1), f32(x), on_device(lists, torch.int32)
    b = x.size(0)
    if tuple(w.shape) != (cout, 2 * cin) or tuple(x.shape) != (b, cin, 64) or lists.dim() != 3 \
            or tuple(lists.shape[:2]) != (b, 64):
        raise ValueError(f"pcd: edgeconv_train layer {layer}: w {tuple(w.shape)} / x {tuple(x.shape)} / lists "
                         f"{tuple(lists.shape)} do not fit")
    return w, x, lists, b, cin, cout


def dgcnn_edgeconv_train(layer: int, w, gamma, beta, eps: float, x, lists, momentum: float = 0.1, running_mean=None,
                         running_var=None, tracked=None):
    """One edge layer in train() with injected lists (pcd_dgcnn_edgeconv_train): (out [b, Cout, 64], argmax uint8
    [b, Cout, 64], stats float64 [3, Cout] = mean, biased variance, 1 / sqrt(var + eps)).  The running buffers
    (float32 / int64, contiguous, on the device), when given, are updated in place."""
    w, x, lists, b, cin, cout = _edge_train_args(layer, w, x, lists)
    gamma, beta = f32(gamma), f32(beta)
    bufs = [None if t is None else _train_tensor(t, what, dt) for t, what, dt in
            ((running_mean, "running_mean", torch.float32), (running_var, "running_var", torch.float32),
             (tracked, "num_batches_tracked", torch.int64))]
    out = torch.empty((b, cout, 64), dtype=torch.float32, device=x.device)
    arg = torch.empty((b, cout, 64), dtype=torch.uint8, device=x.device)
    stats = torch.empty((3, cout), dtype=torch.float64, device=x.device)
    check(lib().pcd_dgcnn_edgeconv_train(ptr(w), ptr(gamma), ptr(beta), float(eps), float(momentum), bufs[0], bufs[1],
                                         bufs[2], int(layer), ptr(x), b, ptr(lists), lists.size(2), ptr(out), ptr(arg),
                                         ptr(stats), c_void_p(stream_ptr())), "pcd_dgcnn_edgeconv_train")
    return out, arg, stats


def dgcnn_edgeconv_train_backward(layer: int, w, gamma, beta, eps: float, x, lists, g, want_dx: bool = True):
    """The backward of dgcnn_edgeconv_train for g = dL/d out [b, Cout, 64] (pcd_dgcnn_edgeconv_train_backward):
    {"dab" [b, 2 Cout, 64], "dgamma", "dbeta" [Cout], "dw" [Cout, 2 Cin], "dx" [b, Cin, 64]}."""
    w, x, lists, b, cin, cout = _edge_train_args(layer, w, x, lists)
    gamma, beta, g = f32(gamma), f32(beta), f32(g)
    if tuple(g.shape) != (b, cout, 64):
        raise ValueError(f"pcd: edgeconv_train_backward: g must be [{b}, {cout}, 64], got {tuple(g.shape)}")
    dev = x.device
    r = {"dab": torch.empty((b, 2 * cout, 64), dtype=torch.float32, device=dev),
         "dgamma": torch.empty(cout, dtype=torch.float32, device=dev),
         "dbeta": torch.empty(cout, dtype=torch.float32, device=dev),
         "dw": torch.empty((cout, 2 * cin), dtype=torch.float32, device=dev),
         "dx": torch.empty((b, cin, 64), dtype=torch.float32, device=dev) if want_dx else None}
    check(lib().pcd_dgcnn_edgeconv_train_backward(ptr(w), ptr(gamma), ptr(beta), float(eps), int(layer), ptr(x), b,
                                                  ptr(lists), lists.size(2), ptr(g), ptr(r["dab"]), ptr(r["dgamma"]),
                                                  ptr(r["dbeta"]), ptr(r["dw"]), ptr(r["dx"]), c_void_p(stream_ptr())),
          "pcd_dgcnn_edgeconv_train_backward")
    return r
