"""ctypes binding of libvpc_hip.so (C ABI declared in include/vpc.h).

The product path has NO CPU fallback: if the HIP library is missing or a launch fails this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from functools import lru_cache

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VPC_LIB") or os.path.join(_HERE, "csrc", "libvpc_hip.so")  # VPC_LIB: diagnostic builds only

_ERR = {1: "bad argument (null / misaligned pointer or bad count)", 2: "unsupported shape (beyond the limits of this entry point, include/vpc.h)",
        3: "HIP runtime error", 4: "the phases of the one-launch step do not share one grid (nothing was launched)"}
ERR_PHASES = 4  # vpc_step_f32 only: the caller makes the three launches


class VpcError(RuntimeError):
    pass


P = C.c_void_p
PP = C.POINTER(C.c_void_p)
I = C.c_int
L_ = C.c_long
F = C.c_float
IP = C.POINTER(C.c_int)
ULL = C.c_ulonglong


class VpcLossCoef(C.Structure):
    """VpcLossCoef of include/vpc.h: the coefficients of the generic loss form as ONE 32-byte record, passed by address to
    every entry point that computes or finalises the loss and copied as it is into the head of a VpcMember row.  One pass:
    cA[1] = cE[1] = 0.  Built once per distinct set of hyperparameters and shared (models.loss_coefficients): read-only."""
    _fields_ = [("cA", F * 2), ("cE", F * 2), ("bq", F), ("bp", F), ("cr", F), ("wml", F)]

    def __init__(self, cA, cE, bq, bp=0.0, cr=0.0, wml=0.0):
        super().__init__((F * 2)(*cA), (F * 2)(*cE), bq, bp, cr, wml)
        self._as_parameter_ = P(C.addressof(self))  # what a c_void_p argument takes: no per-call conversion object

    ml_on = property(lambda self: self.wml != 0.0)  # the ml_reg term: the step consumes a third eps plane
    maskB_on = property(lambda self: self.cE[0] != 0.0)  # the E terms of pass 0: they take mask & ~mask_p (maskB = [mask_p, None])

# name -> argtypes, in the order of include/vpc.h
_PROTOS = {
    "vpc_layout_sizes": [I, I, I, IP, IP, IP, IP, IP, IP, IP, IP],
    "vpc_build_indices": [I, I, I, P, P, P],
    "vpc_layout_sizes_pointnet": [I, I, I, IP, IP, IP, IP, IP, IP, IP, IP, IP],
    "vpc_build_indices_pointnet": [I, I, I, P, P, P],
    "vpc_num_cus": [],
    "vpc_max_partial_blocks": [],
    "vpc_pack_weights": [P, P, P, I, P],
    "vpc_reduce_partials": [P, I, L_, P, P, I, F, P],
    "vpc_adam_step": [P, P, P, P, I, F, F, F, F, L_, P, P, P, P, P, P],
    "vpc_layout_sizes_bf16": [I, I, I, IP, IP],
    "vpc_build_indices_bf16": [I, I, I, P, P],
    "vpc_pack_weights_bf16": [P, P, P, I, P],
    "vpc_step_small_max_rows": [],
    "vpc_step_small_f32": [P, P, P, I, PP, PP, P, PP, P, F, F, P, P, P, IP, L_, I, I, P],
    "vpc_step_small_draw_f32": [P, P, P, I, PP, PP, P, PP, P, F, F, P, P, P, IP, L_, I, I, P, F, P, L_, ULL, ULL, ULL, P, L_, L_,
                                L_, L_, I, P],
    "vpc_step_small_aug_f32": [P, P, P, I, PP, PP, P, PP, P, F, F, P, P, P, IP, L_, I, I, I, P],
    "vpc_step_small_aug_draw_f32": [P, P, P, I, PP, PP, P, PP, P, F, F, P, P, P, IP, L_, I, I, I, P, F, P, L_, ULL, ULL, ULL, P, L_,
                                    L_, L_, L_, I, P],
    "vpc_step_small_eddi_f32": [P, P, P, I, PP, PP, P, PP, P, F, F, P, P, P, IP, L_, I, I, I, I, P, P, P, P],
    "vpc_step_small_eddi_draw_f32": [P, P, P, I, PP, PP, P, PP, P, F, F, P, P, P, IP, L_, I, I, I, I, P, P, P, P, F, P, L_, ULL, ULL,
                                     ULL, P, L_, L_, L_, L_, I, P],
    "vpc_reduce_step_adam_eddi": [P, I, L_, P, I, L_, P, P, I, P, I, P, L_, L_, I, P, P, P, P, P, F, F, F, F, L_, P, P, P, I, P, I,
                                  I, P],
    "vpc_step_small_multi_f32": [P, P, P, P, P, P, P, I, I, I, I, ULL, ULL, F, F, P, P, P, C.POINTER(L_), L_, I, I, I, P],
    "vpc_reduce_step_adam_multi": [P, P, P, I, L_, L_, C.POINTER(L_), P, P, I, P, L_, I, P, P, P, P, P, F, F, F, L_, P, P, P],
    "vpc_step_small_multi_aug_f32": [P, P, P, P, P, P, P, I, I, I, I, ULL, ULL, F, F, P, P, P, C.POINTER(L_), L_, I, I, I, I, P],
    "vpc_step_small_multi_eddi_f32": [P, P, P, P, P, P, P, I, I, I, I, ULL, ULL, F, F, P, P, P, C.POINTER(L_), L_, I, I, I, I, P, P,
                                      P, I, P],
    "vpc_reduce_step_adam_eddi_multi": [P, P, P, I, L_, L_, C.POINTER(L_), P, P, I, P, I, L_, I, P, P, P, P, P, F, F, F, L_, P, P, P,
                                        P, I, I, P],
    "vpc_eval_small_multi_f32": [P, P, P, P, P, P, I, P, L_, L_, L_, I, ULL, F, P, C.POINTER(L_), I, I, I, I, P],
    "vpc_eval_small_multi_aug_f32": [P, P, P, P, P, P, I, P, L_, L_, L_, I, ULL, F, P, C.POINTER(L_), I, I, I, I, P],
    "vpc_eval_small_multi_eddi_f32": [P, P, P, P, P, P, I, P, L_, L_, L_, I, ULL, F, P, C.POINTER(L_), I, I, I, I, P, I, P],
    "vpc_eval_reduce_multi": [P, P, L_, P, I, P, I, L_, L_, I, P, P],
    "vpc_impute_small_multi_f32": [P, P, P, P, P, P, I, P, L_, L_, L_, I, ULL, F, I, P, L_, C.POINTER(L_), I, I, I, I, P],
    "vpc_impute_small_multi_aug_f32": [P, P, P, P, P, P, I, P, L_, L_, L_, I, ULL, F, I, P, L_, C.POINTER(L_), I, I, I, I, P],
    "vpc_impute_small_multi_eddi_f32": [P, P, P, P, P, P, I, P, L_, L_, L_, I, ULL, F, I, P, L_, C.POINTER(L_), I, I, I, I, P, I,
                                        P],
    "vpc_target_mse_multi": [P, L_, L_, I, P, L_, P],
    "vpc_reward_scratch_multi_ex": [I, I, I, I, I, C.POINTER(L_), C.POINTER(L_), C.POINTER(L_)],
    "vpc_reward_matrix_multi_ex": [I, P, P, P, P, P, P, I, P, P, P, P, P, I, I, C.POINTER(L_), I, I, I, I, P],
    "vpc_eddi_fold_multi": [P, L_, P, L_, I, I, I, P],
    "vpc_reward_scratch_multi": [I, I, I, C.POINTER(L_), C.POINTER(L_), C.POINTER(L_)],
    "vpc_reward_matrix_multi": [P, P, P, P, P, P, P, P, P, P, I, I, C.POINTER(L_), I, I, I, I, P],
    "vpc_acquire_multi": [P, L_, P, L_, I, P, L_, I, P, L_, I, I, I, I, P],
    "vpc_step_fused_applicable": [L_, I, I, I],
    "vpc_step_layout_bf16": [I, I, IP, IP],
    "vpc_step_build_indices_bf16": [I, I, P, P],
    "vpc_step_pack_weights_bf16": [P, P, P, I, P],
    "vpc_step_workspace_floats": [L_],
    "vpc_step_fused_bf16": [P, P, I, PP, PP, P, PP, P, F, F, P, P, P, P, IP, L_, I, I, P],
    "vpc_encoder_fwd": [P, P, I, PP, PP, PP, PP, PP, PP, PP, I, I, I, L_, I, I, P],
    "vpc_encoder_bwd": [P, P, I, PP, PP, PP, PP, PP, I, I, I, P, IP, L_, I, I, P],
    "vpc_decoder_fwd": [P, P, P, L_, I, I, P],
    "vpc_decoder_bwd": [P, P, P, P, P, IP, L_, I, I, P],
    "vpc_loss_fwd_bwd": [P, I, PP, PP, PP, P, PP, PP, P, F, F, PP, PP, PP, P, I, IP, L_, I, I, P],
    "vpc_decoder_fused": [P, P, I, PP, PP, P, PP, PP, PP, P, F, F, PP, PP, I, I, P, P, IP, L_, I, I, P],
    "vpc_loss_finalize": [P, I, P, L_, L_, I, P, P, P],
    "vpc_build_inverse_maps": [P, I, I, L_, L_, P, P],
    "vpc_reduce_step": [P, I, L_, P, I, L_, P, P, P, I, I, P, I, P, L_, L_, I, P, P, P, C.c_longlong, P],
    "vpc_reduce_step_adam": [P, I, L_, P, I, L_, P, P, P, I, I, P, I, P, L_, L_, I, P, P, P, P, P, F, F, F, F, L_, P, P, P],
    "vpc_reduce_step_adam_bf16c": [P, I, L_, P, I, L_, P, P, P, I, I, P, I, P, L_, L_, I, P, P, P, P, P, F, F, F, F, L_, P, P, P],
    "vpc_draw_mask": [P, P, L_, F, ULL, ULL, L_, P],
    "vpc_draw_step": [P, P, L_, F, P, L_, ULL, ULL, ULL, P, L_, L_, L_, L_, I, P],
    "vpc_fill_normal": [P, L_, ULL, ULL, P, L_, L_, L_, I, P],
    "vpc_encoder_fwd_draw_f32": [P, P, P, P, PP, PP, PP, PP, L_, I, I, F, ULL, ULL, P, L_, P],
    "vpc_encoder_fwd_last_form": [],
    "vpc_decoder_fused_draw_f32": [P, P, I, PP, PP, P, PP, PP, PP, F, F, PP, PP, P, P, IP, L_, I, I, ULL, ULL, P, L_, L_, P],
    "vpc_step_f32": [P, P, P, P, P, PP, P, PP, PP, PP, PP, PP, PP, PP, F, F, P, P, P, IP, IP, L_, I, I, F, ULL, ULL, ULL, P, L_, L_,
                     L_, I, P],
    "vpc_rccl_unique_id": [P],
    "vpc_rccl_comm_init": [P, I, I, PP],
    "vpc_allreduce_flat": [P, P, L_, P],
    "vpc_rccl_comm_destroy": [P],
    "vpc_reward_scratch": [I, I, I, C.POINTER(L_), C.POINTER(L_), C.POINTER(L_)],
    "vpc_reward_matrix": [P, P, P, P, P, P, P, P, P, P, I, I, I, I, P],
    "vpc_reward_scratch_ex": [I, I, I, I, I, C.POINTER(L_), C.POINTER(L_), C.POINTER(L_)],
    "vpc_reward_matrix_ex": [I, P, P, P, P, P, P, I, P, P, P, P, P, I, I, I, I, P],
    # MNAR path (config 3)
    "vpc_linear_fwd": [P, L_, P, P, P, L_, L_, I, I, I, I, I, P],
    "vpc_linear_dgrad": [P, L_, P, L_, I, I, P, P, L_, I, P, L_, L_, I, I, I, P],
    "vpc_linear_wgrad_scratch": [L_, I, I],
    "vpc_linear_wgrad": [P, L_, P, L_, I, I, P, L_, P, P, P, L_, L_, I, I, I, I, P],
    "vpc_linear_wgrad_reduce": [I, PP, C.POINTER(L_), IP, IP, PP, PP, IP, P],
    # the same layer ops for few rows (csrc/vpc_rows.hip)
    "vpc_rows_max_rows": [],
    "vpc_rows_fwd": [P, L_, P, P, P, L_, L_, I, I, I, I, P],
    "vpc_rows_bwd": [P, L_, P, L_, I, I, P, P, L_, P, L_, I, P, L_, P, P, L_, I, I, I, P],
    "vpc_nm_sample": [P, L_, P, P, L_, L_, I, I, P],
    "vpc_nm_sample_bwd": [P, L_, P, P, L_, P, L_, P, L_, L_, I, I, P],
    "vpc_nm_mul": [P, P, P, L_, P],
    "vpc_nm_loss_blocks": [L_],
    "vpc_nm_loss_scratch": [L_, I],
    "vpc_nm_loss": [P, P, P, P, P, L_, P, P, L_, P, P, L_, P, P, P, P, P, L_, P, P, L_, P, P, L_, P, P, I, P, P, L_, P,
                    P, P, P, C.c_longlong, I, L_, L_, I, I, I, C.c_double, P],
    "vpc_nm_prep": [P, P, P, P, L_, I, F, P, L_, ULL, ULL, ULL, P, L_, L_, L_, L_, I, P],
    "vpc_nmdec_applicable": [L_, I, I, I],
    "vpc_nmdec_layout": [L_, I, I, I, IP, C.POINTER(C.c_long), IP],
    "vpc_nmdec_build_indices": [I, I, I, P, P, I],
    "vpc_nmenc_fwd": [P, P, P, P, P, L_, I, I, P],
    "vpc_nmenc_bwd": [P, P, P, P, P, P, L_, P, P, L_, I, I, P],
    "vpc_nmenc_build_indices": [I, I, I, P, C.POINTER(C.c_long), I],
    "vpc_nm_fused_bwd_step": [P, P, P, P, P, P, P, P, L_, P, P, P, P, P, L_, P, P, P, I, P, P, P, L_, L_, I, I, I, C.c_double,
                              P, P, P, F, F, F, F, L_, P, P],
    "vpc_nmdec_step": [P, P, P, P, P, L_, P, P, P, P, P, P, P, I, P, P, P, P, C.c_longlong, L_, L_, I, I, I, C.c_double, P],
    # MIWAE path (csrc/vpc_miw.hip)
    "vpc_miw_sample": [P, P, P, P, L_, I, I, P],
    "vpc_miw_sample_bwd": [P, P, P, P, P, L_, I, I, P],
    "vpc_miw_heads": [P, P, L_, I, P],
    "vpc_miw_heads_bwd": [P, P, P, L_, I, P],
    "vpc_miw_loss_scratch": [L_, I],
    "vpc_miw_loss": [P, P, P, P, P, L_, I, P, P, P, P, P, P, L_, P, P, P, P, L_, P, P, P, L_, I, I, I, C.c_double, I, P],
    # small-batch MIWAE step (csrc/vpc_miw_small.hip)
    "vpc_miw_small_workspace": [I, I],
    "vpc_miw_small_fwd": [P] * 11 + [L_, I, I, I, I, P],
    "vpc_miw_small_bwd": [P] * 13 + [L_, L_, I, I, I, I, P],
    "vpc_miw_small_tail": [P, L_, L_, I, I, I, P, P, P, P, F, F, F, F, L_, P],
    # the small-batch MIWAE step for G members (csrc/vpc_miw_small.hip, vpc_miw.hip, vpc_misc.hip)
    "vpc_miw_multi_workspace": [I, I, I, I],
    "vpc_miw_multi_prep": [P, L_, P, L_, P, P, P, P, I, I, L_, I, I, I, ULL, ULL, P],
    "vpc_miw_small_fwd_multi": [P, L_] + [P] * 10 + [I, L_, I, I, I, I, I, P],
    "vpc_miw_loss_multi": [P, L_, P, L_] + [P] * 7 + [L_, P, P, P, P, I, L_, I, I, I, I, P],
    "vpc_miw_small_bwd_multi": [P, L_] + [P] * 12 + [L_, I, I, L_, I, I, I, I, I, P],
    "vpc_miw_small_tail_multi": [P, L_, I, I, I, I, P, P, P, P, L_, P, F, F, F, L_, P],
    # streaming MIWAE imputation (csrc/vpc_miw_impute.hip)
    "vpc_miw_impute_scratch": [L_, I, I, I, I],
    "vpc_miw_impute": [P, P, P, P, ULL, ULL, L_, P, L_, P, P, L_, I, I, I, I, P],
    "vpc_miw_impute_draws": [P, L_, I, I, ULL, ULL, L_, P],
    # streaming MNAR imputation (csrc/vpc_nm_impute.hip)
    "vpc_nm_impute_scratch": [L_, I, I, I, I],
    "vpc_nm_impute": [P, P, P, P, ULL, ULL, L_, P, L_, P, P, L_, I, I, I, I, I, P],
    # flow path (csrc/vpc_flow.hip)
    "vpc_flow_prep": [P, P, P, P, P, P, L_, L_, I, F, ULL, ULL, ULL, P],
    "vpc_flow_fwd": [P, L_, P, P, P, L_, L_, P],
    "vpc_flow_bwd": [P, L_, P, P, P, P, P, L_, L_, L_, P],
    "vpc_flow_loss_scratch": [L_],
    "vpc_flow_loss": [P, P, P, P, P, L_, P, P, P, P, P, P, L_, P, P, P, P, P, L_, P, P, P, L_, I, I, F, F, F, I, P],
    # the few-row flow step with a member axis (csrc/vpc_rows.hip, vpc_flow.hip, vpc_misc.hip)
    "vpc_rows_fwd_multi": [P, L_, L_, P, P, L_, P, L_, L_, I, L_, I, I, I, I, I, P],
    "vpc_rows_bwd_multi": [P, L_, L_, P, L_, L_, I, I, P, P, L_, L_, P, L_, L_, I, P, L_, L_, P, P, L_, I, L_, I, I, I, I, P],
    "vpc_flow_multi_prep": [P, L_, P, L_, P, L_, P, L_, P, L_, P, I, I, L_, L_, I, ULL, ULL, P],
    "vpc_flow_fwd_multi": [P, L_, L_, P, P, P, L_, I, L_, L_, P],
    "vpc_flow_bwd_multi": [P, L_, L_, P, P, P, P, L_, P, L_, L_, I, L_, L_, P],
    "vpc_flow_loss_multi_scratch": [I, L_],
    "vpc_flow_loss_multi": [P, L_, P, L_, P, L_, P, P, L_, L_, P, P, P, P, P, P, L_, L_, P, P, P, P, L_, P, L_, P, P, P, P, I, L_,
                            I, I, F, I, P],
    "vpc_adam_step_multi": [P, P, P, P, L_, I, P, I, F, F, F, L_, P],
    # batched evaluation of a flow model (csrc/vpc_floweval.hip); every table as (host, device copy)
    "vpc_flow_fwd_tiles": [P, L_, P, P, P, L_, P, P, L_, P],
    "vpc_flow_eval_tiles_scratch": [L_, L_],
    "vpc_flow_eval_tiles": [P, P, P, L_, P, P, L_, I, P, P, L_, F, P, L_, P, P],
    "vpc_flow_eval_finalize": [P, L_, P, P, L_, P, P],
    # config 5 reward of the flow models (csrc/vpc_flowreward.hip)
    "vpc_flow_reward_scratch": [I, I, I, I, I, C.POINTER(L_)],
    "vpc_flow_reward_matrix": [P, P, P, P, P, P, P, P, P, P, ULL, P, L_, P, I, I, I, I, I, P],
    "vpc_flow_reward_draws": [P, I, I, I, ULL, P],
    # annealed importance sampling (csrc/vpc_ais.hip)
    "vpc_ais_applicable": [L_, I, I],
    "vpc_ais_state_floats": [L_],
    "vpc_ais_run": [P, P, P, I, I, I, I, P, P, P, P, ULL, F, I, F, F, F, L_, L_, I, I, P],
    "vpc_ais_draws": [P, P, P, L_, I, I, ULL, P],
    # the GEMM-backed AIS engine (csrc/vpc_aisg.hip)
    "vpc_aisg_workspace_floats": [L_, I, I, IP],
    "vpc_aisg_run": [P, P, PP, PP, IP, IP, IP, I, I, F, P, I, I, I, I, P, L_, P, P, P, ULL, F, I, F, F, L_, L_, I, I, P],
    # PNP / EDDI encoder front-end
    "vpc_eddi_fold": [P, P, P, P, P, I, I, P],
    "vpc_eddi_front_fwd": [P, P, P, P, P, L_, I, I, P],
    "vpc_eddi_front_scratch": [L_, I, I],
    "vpc_eddi_front_bwd": [P, P, P, P, P, P, P, P, P, L_, P, P, P, P, I, L_, I, I, P],
    # the same front-end at image width (vpc_eddiw_*, csrc/vpc_eddi.hip)
    "vpc_eddiw_fold": [P, P, P, P, P, I, I, P],
    "vpc_eddiw_front_fwd": [P, P, P, P, P, L_, I, I, P],
    "vpc_eddiw_front_scratch": [L_, I, I],
    "vpc_eddiw_front_bwd": [P, P, P, P, P, P, P, P, P, L_, P, P, P, P, I, L_, I, I, P],
}
_RESTYPE_LONG = {"vpc_step_small_max_rows", "vpc_step_workspace_floats", "vpc_linear_wgrad_scratch", "vpc_nm_loss_scratch", "vpc_eddi_front_scratch", "vpc_miw_loss_scratch", "vpc_miw_small_workspace", "vpc_miw_multi_workspace", "vpc_miw_impute_scratch", "vpc_nm_impute_scratch", "vpc_flow_loss_scratch", "vpc_flow_loss_multi_scratch", "vpc_flow_eval_tiles_scratch", "vpc_eddiw_front_scratch", "vpc_ais_state_floats", "vpc_aisg_workspace_floats"}

_lib = None


def lib():
    """Load the shared library (once).  Raises VpcError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VpcError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
        handle = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            fn = getattr(handle, name)  # AttributeError here = header / library mismatch
            fn.argtypes = argtypes
            fn.restype = L_ if name in _RESTYPE_LONG else I
        _lib = handle
    return _lib


def exported_symbols():
    return list(_PROTOS)


def check(code: int, what: str):
    if code != 0:
        raise VpcError(f"{what} failed: {_ERR.get(code, code)}")


def ptr(t):
    """Device / host pointer of a tensor (or None) as c_void_p."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def ptr_array(tensors):
    """HOST array of pointers for the per-pass arguments."""
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr():
    """torch's CURRENT stream on the current device as a hipStream_t (queried on every launch: graph capture and user
    streams change it; the raw C query is ~10x cheaper than building a torch.cuda.Stream object per launch)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise VpcError("this path runs only on the GPU (HIP kernels, no CPU fallback): got a CPU tensor; "
                           "move the model and its inputs to 'cuda'")


class Layout:
    """Sizes and index tables of the packed layouts for one (d, L).  pointnet_K > 0: the point-net kind (Reg_EDDI /
    vanilla_EDDI on the small-batch step) - the encoder is the trunk with an input of pointnet_K columns, n_params counts trunk
    and decoder, n_front the four front-end tensors behind them in the flat vector."""

    def __init__(self, d: int, L: int, mask_augm: bool = False, pointnet_K: int = 0):
        l = lib()
        self.mask_augm = int(bool(mask_augm))
        self.K, self.n_front = pointnet_K, 0
        vals = [C.c_int() for _ in range(8)]
        if pointnet_K:
            nf = C.c_int()
            refs = [C.byref(v) for v in vals]
            check(l.vpc_layout_sizes_pointnet(d, pointnet_K, L, *refs[:4], C.byref(nf), *refs[4:]), "vpc_layout_sizes_pointnet")
            self.n_front = nf.value
        else:
            check(l.vpc_layout_sizes(d, L, self.mask_augm, *[C.byref(v) for v in vals]), "vpc_layout_sizes")
        (self.enc_img, self.dec_img, self.n_enc, self.n_params, self.enc_part, self.dec_part, self.loss_terms,
         self.tile_rows) = [v.value for v in vals]
        self.d, self.L = d, L
        self.pack_idx = np.empty(self.n_params, np.int32)
        self.grad_idx = np.empty(self.n_params, np.int32)
        self.img_template = np.empty(self.enc_img + self.dec_img, np.float32)
        tables = (self.pack_idx.ctypes.data_as(P), self.grad_idx.ctypes.data_as(P), self.img_template.ctypes.data_as(P))
        if pointnet_K:
            check(l.vpc_build_indices_pointnet(d, pointnet_K, L, *tables), "vpc_build_indices_pointnet")
        else:
            check(l.vpc_build_indices(d, L, self.mask_augm, *tables), "vpc_build_indices")
        self._dev = {}

    def device_tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.pack_idx).to(device), torch.from_numpy(self.grad_idx).to(device))
        return self._dev[key]

    def bf16_tables(self, device):
        """(pack_idx_bf [n_params] int32 on `device`, img_template_bf numpy [enc + dec floats], enc_img floats) of the
        bf16 weight images (precision 1 / 2: csrc/vpc_bf16.h)."""
        key = ("bf16", str(device))
        if key not in self._dev:
            l = lib()
            e, dd = C.c_int(), C.c_int()
            check(l.vpc_layout_sizes_bf16(self.d, self.L, self.mask_augm, C.byref(e), C.byref(dd)), "vpc_layout_sizes_bf16")
            idx = np.empty(self.n_params, np.int32)
            tmpl = np.empty(e.value + dd.value, np.float32)
            check(l.vpc_build_indices_bf16(self.d, self.L, self.mask_augm, idx.ctypes.data_as(P), tmpl.ctypes.data_as(P)),
                  "vpc_build_indices_bf16")
            self._dev[key] = (torch.from_numpy(idx).to(device), tmpl, e.value)
        return self._dev[key]

    def step_tables(self, device):
        """(pack_idx_c [n_params] int32 on `device`, img_template_c numpy [floats]) of the compact bf16 image of the
        whole-step kernel (csrc/vpc_step.hip)."""
        key = ("step", str(device))
        if key not in self._dev:
            l = lib()
            n = C.c_int()
            check(l.vpc_step_layout_bf16(self.d, self.L, C.byref(n), None), "vpc_step_layout_bf16")
            idx = np.empty(self.n_params, np.int32)
            tmpl = np.empty(n.value, np.float32)
            check(l.vpc_step_build_indices_bf16(self.d, self.L, idx.ctypes.data_as(P), tmpl.ctypes.data_as(P)),
                  "vpc_step_build_indices_bf16")
            self._dev[key] = (torch.from_numpy(idx).to(device), tmpl)
        return self._dev[key]

    def inverse_maps(self, device):
        """Caller-owned inverse maps (partial-block position -> flat parameter, -1 = padding) for the layout-order
        gradient reduction of vpc_reduce_step: [enc_part | dec_part] int32 on `device`, built once per device by the
        explicit entry point vpc_build_inverse_maps (the library itself allocates nothing)."""
        key = ("inv", str(device))
        if key not in self._dev:
            _, gidx = self.device_tables(device)
            inv = torch.empty(self.enc_part + self.dec_part, dtype=torch.int32, device=device)
            check(lib().vpc_build_inverse_maps(ptr(gidx), self.n_enc, self.n_params, self.enc_part, self.dec_part,
                                               ptr(inv), stream_ptr()), "vpc_build_inverse_maps")
            self._dev[key] = inv
        return self._dev[key]

    def nblocks(self, B: int, ncu: int) -> int:
        return min((B + self.tile_rows - 1) // self.tile_rows, ncu)


@lru_cache(maxsize=None)
def layout(d: int, L: int, mask_augm: bool = False) -> Layout:
    return Layout(d, L, mask_augm)


@lru_cache(maxsize=None)
def pointnet_layout(d: int, K: int, L: int) -> Layout:
    return Layout(d, L, pointnet_K=K)


_NCU = None


def num_cus() -> int:
    global _NCU
    if _NCU is None:
        _NCU = int(lib().vpc_num_cus())
    return _NCU


def max_blocks() -> int:
    """Upper bound of the partial blocks any kernel writes (sizes the partial / loss-partial buffers)."""
    return int(lib().vpc_max_partial_blocks())


# Positions of the hidden units (index H = the constant-1 unit of the bias chain) inside the padded 112- / 64-wide
# workspaces and weight images (csrc/vpc_layout.h pos1 / pos2): the last, partly filled tile is laid out j-major so
# that the MFMA k-steps holding only padding can be skipped.  Only tests and debugging tools need this.
HIDDEN_POS1 = list(range(96)) + [96, 100, 104, 108, 97]
HIDDEN_POS2 = list(range(48)) + [48, 52, 56]
