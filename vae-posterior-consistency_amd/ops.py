"""Thin Python wrappers over the C ABI + the autograd Functions of the API-compatible path.

Every function here launches HIP kernels on torch's current stream; tensors must live on the GPU.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from ._lib import check, lib, ptr, ptr_array, require_cuda, stream_ptr
from .linear import _f32c  # noqa: F401  (also reached as ops._f32c)

H1P, H2P = 112, 64  # padded hidden widths of the h1 / h2 workspaces (csrc/vpc_layout.h)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def as_mask_u8(mask: torch.Tensor) -> torch.Tensor:
    """bool / float / uint8 mask -> contiguous uint8 holding 0 / 1 (non-zero = observed): the kernels convert mask bytes
    with v_cvt_f32_ubyte, so the ABI contract is 0 / 1 bytes (include/vpc.h).  uint8 input of unknown origin is clamped
    (one small launch); masks this package produced itself are passed through."""
    if mask.dtype == torch.uint8:
        m = mask if getattr(mask, "_vpc_mask01", False) else torch.clamp(mask, max=1)
    elif mask.dtype == torch.bool:
        m = mask.contiguous().view(torch.uint8)
    else:
        m = (mask != 0).view(torch.uint8)
    m = m.contiguous()
    try:
        m._vpc_mask01 = True  # plain attribute on the tensor object: survives as long as this object is passed around
    except Exception:
        pass
    return m


# ------------------------------------------------------------------------------------------------ raw ops
def pack_weights(flat_params, pack_idx, img):
    check(lib().vpc_pack_weights(ptr(flat_params), ptr(pack_idx), ptr(img), flat_params.numel(), stream_ptr()),
          "vpc_pack_weights")


def reduce_partials(partials, nblocks, stride, grad_idx, out, scale=1.0):
    check(lib().vpc_reduce_partials(ptr(partials), nblocks, stride, ptr(grad_idx), ptr(out), out.numel(),
                                    float(scale), stream_ptr()), "vpc_reduce_partials")


def adam_step(params, grads, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, pack_idx=None, img=None,
              step_dev=None, loss_in=None, accum=None):
    check(lib().vpc_adam_step(ptr(params), ptr(grads), ptr(m), ptr(v), params.numel(), lr, beta1, beta2, eps,
                              int(step), ptr(step_dev), ptr(pack_idx), ptr(img), ptr(loss_in), ptr(accum),
                              stream_ptr()), "vpc_adam_step")


PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16": 2}


def pack_weights_bf16(flat_params, pack_idx_bf, img_bf):
    check(lib().vpc_pack_weights_bf16(ptr(flat_params), ptr(pack_idx_bf), ptr(img_bf), flat_params.numel(),
                                      stream_ptr()), "vpc_pack_weights_bf16")


def encoder_fwd(x, enc_img, masks, eps, h1, h2, mean, logvar, z, d, Ld, lat_pitch=None, mask_augm=False, precision=0):
    n = len(masks)
    B = x.shape[0]
    check(lib().vpc_encoder_fwd(ptr(x), ptr(enc_img), n, ptr_array(masks),
                                ptr_array(eps) if eps is not None else None, ptr_array(h1), ptr_array(h2),
                                ptr_array(mean), ptr_array(logvar), ptr_array(z) if z is not None else None,
                                lat_pitch or Ld, int(mask_augm), int(precision), B, d, Ld, stream_ptr()),
          "vpc_encoder_fwd")


def encoder_bwd(x, enc_img, masks, h1, h2, dmean, dlogvar, partials, d, Ld, lat_pitch=None, mask_augm=False,
                precision=0):
    n = len(masks)
    nb = C.c_int(0)
    check(lib().vpc_encoder_bwd(ptr(x), ptr(enc_img), n, ptr_array(masks), ptr_array(h1), ptr_array(h2),
                                ptr_array(dmean), ptr_array(dlogvar), lat_pitch or Ld, int(mask_augm), int(precision),
                                ptr(partials), C.byref(nb),
                                x.shape[0], d, Ld, stream_ptr()), "vpc_encoder_bwd")
    return nb.value


def decoder_fwd(z, dec_img, xhat, d, Ld):
    check(lib().vpc_decoder_fwd(ptr(z), ptr(dec_img), ptr(xhat), z.shape[0], d, Ld, stream_ptr()), "vpc_decoder_fwd")


def decoder_bwd(z, dxhat, dec_img, dz, partials, d, Ld):
    nb = C.c_int(0)
    check(lib().vpc_decoder_bwd(ptr(z), ptr(dxhat), ptr(dec_img), ptr(dz), ptr(partials), C.byref(nb), z.shape[0], d,
                                Ld, stream_ptr()), "vpc_decoder_bwd")
    return nb.value


def loss_fwd_bwd(x, xhat, maskA, maskB, co, mean, logvar, eps_ml, inv_B, x_logvar, dxhat, dmean, dlogvar, loss_part, d, Ld):
    """co: the loss coefficients, a _lib.VpcLossCoef (here and in every wrapper below that takes `co`)."""
    n = len(xhat)
    nb = C.c_int(0)
    want = dxhat is not None
    check(lib().vpc_loss_fwd_bwd(ptr(x), n, ptr_array(xhat), ptr_array(maskA), ptr_array(maskB), co,
                                 ptr_array(mean), ptr_array(logvar), ptr(eps_ml), inv_B, x_logvar,
                                 ptr_array(dxhat) if want else None, ptr_array(dmean) if want else None,
                                 ptr_array(dlogvar) if want else None, ptr(loss_part), loss_part.shape[0],
                                 C.byref(nb), x.shape[0], d, Ld, stream_ptr()), "vpc_loss_fwd_bwd")
    return nb.value


def decoder_fused(x, dec_img, maskA, maskB, co, mean, logvar, eps, eps_ml, inv_B, x_logvar, dmean, dlogvar, partials,
                  loss_part, d, Ld, lat_pitch=None, precision=0):
    n = len(maskA)
    nb = C.c_int(0)
    check(lib().vpc_decoder_fused(ptr(x), ptr(dec_img), n, ptr_array(maskA), ptr_array(maskB), co,
                                  ptr_array(mean), ptr_array(logvar), ptr_array(eps), ptr(eps_ml), inv_B, x_logvar, ptr_array(dmean), ptr_array(dlogvar), lat_pitch or Ld, int(precision),
                                  ptr(partials), ptr(loss_part), C.byref(nb), x.shape[0], d, Ld, stream_ptr()),
          "vpc_decoder_fused")
    return nb.value


def encoder_fwd_draw_f32(x, enc_img, mask_in, mask_p_out, h1, h2, mean, logvar, d, Ld, keep_prob, seed, offset_mask, state=None,
                         elem_lo=0):
    """encoder_fwd (two passes, fp32, padded latent workspaces) that draws mask_p = mask_in & keep for the mask words it
    holds, with vpc_draw_step's counters, and stores it to mask_p_out."""
    check(lib().vpc_encoder_fwd_draw_f32(ptr(x), ptr(enc_img), ptr(mask_in), ptr(mask_p_out), ptr_array(h1), ptr_array(h2),
                                         ptr_array(mean), ptr_array(logvar), x.shape[0], d, Ld, float(keep_prob), int(seed),
                                         int(offset_mask), ptr(state), int(elem_lo), stream_ptr()), "vpc_encoder_fwd_draw_f32")


def decoder_fused_draw_f32(x, dec_img, maskA, maskB, co, mean, logvar, eps, inv_B, x_logvar, dmean, dlogvar, partials, loss_part,
                           d, Ld, seed, offset_eps, state=None, eps_shard=None):
    """decoder_fused (fp32, 8-wave kernel, no ml_reg sample) that draws the eps planes it consumes, with vpc_draw_step's
    counters, and stores them to eps (plane p = eps[p], [B][16])."""
    n = len(maskA)
    nb = C.c_int(0)
    rows_local, rows_global, row_lo, _ = (x.shape[0], x.shape[0], 0, 16) if eps_shard is None else _shard4(eps_shard)
    check(lib().vpc_decoder_fused_draw_f32(ptr(x), ptr(dec_img), n, ptr_array(maskA), ptr_array(maskB), co, ptr_array(mean),
                                           ptr_array(logvar), ptr_array(eps), inv_B, x_logvar, ptr_array(dmean),
                                           ptr_array(dlogvar), ptr(partials), ptr(loss_part), C.byref(nb), x.shape[0], d, Ld,
                                           int(seed), int(offset_eps), ptr(state), rows_global, row_lo, stream_ptr()),
          "vpc_decoder_fused_draw_f32")
    return nb.value


def step_f32(x, enc_img, dec_img, mask_in, mask_p_out, maskB, co, h1, h2, mean, logvar, eps, inv_B, x_logvar, dmean, dlogvar,
             partE, partD, loss_part, d, Ld, keep_prob, seed, offset_mask, offset_eps, state=None, elem_lo=0, eps_shard=None,
             force_shape=False):
    """encoder_fwd_draw_f32 + decoder_fused_draw_f32 + encoder_bwd (two passes, fp32, padded latent workspaces) as three phases
    of ONE launch, csrc/vpc_step_f32.hip: the same bytes everywhere.  Returns the (encoder, decoder) partial-block counts for
    reduce_step, or None - nothing launched - when the three kernels would not run one common grid (encoder_bwd takes the
    small-batch shape at this B and force_shape is off): the caller then makes the three launches."""
    nbE, nbD = C.c_int(0), C.c_int(0)
    rows_local, rows_global, row_lo, _ = (x.shape[0], x.shape[0], 0, 16) if eps_shard is None else _shard4(eps_shard)
    rc = lib().vpc_step_f32(ptr(x), ptr(enc_img), ptr(dec_img), ptr(mask_in), ptr(mask_p_out), ptr_array(maskB), co,
                            ptr_array(h1), ptr_array(h2), ptr_array(mean), ptr_array(logvar), ptr_array(eps), ptr_array(dmean),
                            ptr_array(dlogvar), inv_B, x_logvar, ptr(partE), ptr(partD), ptr(loss_part), C.byref(nbE),
                            C.byref(nbD), x.shape[0], d, Ld, float(keep_prob), int(seed), int(offset_mask), int(offset_eps),
                            ptr(state), int(elem_lo), rows_global, row_lo, int(bool(force_shape)), stream_ptr())
    if rc == L.ERR_PHASES:
        return None
    check(rc, "vpc_step_f32")
    return nbE.value, nbD.value


def step_small_max_rows():
    return int(lib().vpc_step_small_max_rows())


def step_small_f32(x, enc_img, dec_img, masks, maskB, co, eps, eps_ml, inv_B, x_logvar, partE, partD, loss_part, d, Ld):
    """Whole fp32 step of a small batch in one launch (16-row tiles, feature tiles split over the waves); returns the
    number of partial blocks."""
    n = len(masks)
    nb = C.c_int(0)
    check(lib().vpc_step_small_f32(ptr(x), ptr(enc_img), ptr(dec_img), n, ptr_array(masks), ptr_array(maskB), co,
                                   ptr_array(eps), ptr(eps_ml), inv_B, x_logvar, ptr(partE),
                                   ptr(partD), ptr(loss_part), C.byref(nb), x.shape[0], d, Ld, stream_ptr()), "vpc_step_small_f32")
    return nb.value


def step_small_draw_f32(x, enc_img, dec_img, masks, maskB, co, eps, eps_ml, inv_B, x_logvar, partE, partD, loss_part, d, Ld, mask_in, keep_prob, eps_out, seed, offset_mask, offset_eps, state=None, elem_lo=0,
                        eps_shard=None):
    """step_small_f32 that also makes the step's draws (mask_p = mask_in & keep into masks[1], eps into eps_out = eps[0]...)
    inside the same launch, with vpc_draw_step's counters."""
    n = len(masks)
    nb = C.c_int(0)
    check(lib().vpc_step_small_draw_f32(ptr(x), ptr(enc_img), ptr(dec_img), n, ptr_array(masks), ptr_array(maskB), co,
                                        ptr_array(eps), ptr(eps_ml), inv_B, x_logvar, ptr(partE),
                                        ptr(partD), ptr(loss_part), C.byref(nb), x.shape[0], d, Ld, ptr(mask_in),
                                        float(keep_prob), ptr(eps_out), eps_out.numel(), int(seed), int(offset_mask),
                                        int(offset_eps), ptr(state), int(elem_lo), *_shard4(eps_shard), stream_ptr()),
          "vpc_step_small_draw_f32")
    return nb.value


def small_aug_pitch(d):
    """Row pitch of x / mask / mask_p on the small-batch path of the mask-augmented classes: 4 * ceil(d / 4), the plain
    models' rule (mask 0 in the padding)."""
    return 4 * ((d + 3) // 4)


def small_aug_tiles(d):
    """(DTI, DT) of the step_small_aug_kernel instantiation that serves obs_dim d: 16-wide tiles of the encoder input
    [x*mask | mask] (2 d wide) and of the decoder output (d wide); None past the kernels' reach (2 d > 128)."""
    dt_for = lambda n: 1 if n <= 16 else 2 if n <= 32 else 4 if n <= 64 else 8
    return (dt_for(2 * d), dt_for(d)) if 1 <= d and 2 * d <= 128 else None


def step_small_aug_f32(x, enc_img, dec_img, masks, maskB, co, eps, eps_ml, inv_B, x_logvar, partE, partD, loss_part, d, d_real,
                       Ld):
    """step_small_f32 of Reg_VAE_mask / vanilla_VAE_mask: `d` is the row pitch small_aug_pitch(d_real) of x and the masks,
    the images are those of the mask-augmented layout; the kernel builds [x*mask | mask] itself."""
    n = len(masks)
    nb = C.c_int(0)
    check(lib().vpc_step_small_aug_f32(ptr(x), ptr(enc_img), ptr(dec_img), n, ptr_array(masks), ptr_array(maskB), co,
                                       ptr_array(eps), ptr(eps_ml), inv_B, x_logvar, ptr(partE),
                                       ptr(partD), ptr(loss_part), C.byref(nb), x.shape[0], d, d_real, Ld, stream_ptr()),
          "vpc_step_small_aug_f32")
    return nb.value


def step_small_aug_draw_f32(x, enc_img, dec_img, masks, maskB, co, eps, eps_ml, inv_B, x_logvar, partE, partD, loss_part, d,
                            d_real, Ld, mask_in, keep_prob, eps_out, seed, offset_mask, offset_eps, state=None, elem_lo=0,
                            eps_shard=None):
    """step_small_aug_f32 that also makes the step's draws inside the launch (as step_small_draw_f32, at the pitch `d`)."""
    n = len(masks)
    nb = C.c_int(0)
    check(lib().vpc_step_small_aug_draw_f32(ptr(x), ptr(enc_img), ptr(dec_img), n, ptr_array(masks), ptr_array(maskB), co,
                                            ptr_array(eps), ptr(eps_ml), inv_B, x_logvar, ptr(partE),
                                            ptr(partD), ptr(loss_part), C.byref(nb), x.shape[0], d, d_real, Ld, ptr(mask_in),
                                            float(keep_prob), ptr(eps_out), eps_out.numel(), int(seed), int(offset_mask),
                                            int(offset_eps), ptr(state), int(elem_lo), *_shard4(eps_shard), stream_ptr()),
          "vpc_step_small_aug_draw_f32")
    return nb.value


def small_eddi_tiles(d, K):
    """(DTI, DT) of the step_small_eddi_kernel instantiation that serves obs_dim d and emb_dim K: 16-wide tiles of the trunk's
    input agg (K wide) and of the decoder output (d wide); None where there is none (K > 32 or d > 64)."""
    if not (1 <= K <= 32 and 1 <= d <= 64):
        return None
    return (1 if K <= 16 else 2), (1 if d <= 16 else 2 if d <= 32 else 4)


def step_small_eddi_f32(x, enc_img, dec_img, masks, maskB, co, eps, eps_ml, inv_B, x_logvar, partE, partD, loss_part, d, d_real,
                        Ld, K, front, partF, snap):
    """step_small_f32 of Reg_EDDI / vanilla_EDDI: `d` is the row pitch small_aug_pitch(d_real) of x and the masks, the images
    are those of the point-net layout, `front` the front-end parameters in flat order; the tiles' (dA | dC) blocks go to partF,
    a copy of `front` to snap (include/vpc.h)."""
    n = len(masks)
    nb = C.c_int(0)
    check(lib().vpc_step_small_eddi_f32(ptr(x), ptr(enc_img), ptr(dec_img), n, ptr_array(masks), ptr_array(maskB), co,
                                        ptr_array(eps), ptr(eps_ml), inv_B, x_logvar, ptr(partE), ptr(partD), ptr(loss_part),
                                        C.byref(nb), x.shape[0], d, d_real, Ld, K, ptr(front), ptr(partF), ptr(snap),
                                        stream_ptr()), "vpc_step_small_eddi_f32")
    return nb.value


def step_small_eddi_draw_f32(x, enc_img, dec_img, masks, maskB, co, eps, eps_ml, inv_B, x_logvar, partE, partD, loss_part, d,
                             d_real, Ld, K, front, partF, snap, mask_in, keep_prob, eps_out, seed, offset_mask, offset_eps,
                             state=None, elem_lo=0, eps_shard=None):
    """step_small_eddi_f32 that also makes the step's draws inside the launch (as step_small_draw_f32, at the pitch `d`)."""
    n = len(masks)
    nb = C.c_int(0)
    check(lib().vpc_step_small_eddi_draw_f32(ptr(x), ptr(enc_img), ptr(dec_img), n, ptr_array(masks), ptr_array(maskB), co,
                                             ptr_array(eps), ptr(eps_ml), inv_B, x_logvar, ptr(partE), ptr(partD),
                                             ptr(loss_part), C.byref(nb), x.shape[0], d, d_real, Ld, K, ptr(front), ptr(partF),
                                             ptr(snap), ptr(mask_in), float(keep_prob), ptr(eps_out), eps_out.numel(), int(seed),
                                             int(offset_mask), int(offset_eps), ptr(state), int(elem_lo), *_shard4(eps_shard),
                                             stream_ptr()), "vpc_step_small_eddi_draw_f32")
    return nb.value


def reduce_step_adam_eddi(partE, partD, nb, strideE, strideD, inv_maps, grad, n, loss_part, co, B_local, B_global, d, out9, accum,
                          params, m, v, lr, beta1, beta2, eps, step, pack_idx, img, partF, snap, K, d_pitch):
    """The tail of the small-batch EDDI step in one launch: trunk / decoder blocks and loss as reduce_step_adam, the front-end
    blocks partF summed, chained back to the four front-end tensors and stepped (include/vpc.h).  `nb` blocks of each kind."""
    check(lib().vpc_reduce_step_adam_eddi(ptr(partE), nb, strideE, ptr(partD), nb, strideD, ptr(inv_maps), ptr(grad), n,
                                          ptr(loss_part), nb, co, B_local, B_global, d, ptr(out9), ptr(accum), ptr(params),
                                          ptr(m), ptr(v), lr, beta1, beta2, eps, int(step), ptr(pack_idx), ptr(img), ptr(partF),
                                          nb, ptr(snap), K, d_pitch, stream_ptr()), "vpc_reduce_step_adam_eddi")


# Slots of the member-stride vectors of include/vpc.h: VPC_MS_* (ensemble step, evaluation, imputation), VPC_RM_* (reward)
MS_X, MS_MASK, MS_MASK_P, MS_EPS, MS_IMG, MS_PARTE, MS_PARTD, MS_LOSS, MS_PARAM, MS_COUNT = range(10)
MS_PART = MS_LOSS  # the evaluation's per-tile sums [tiles][5] doubles travel in the loss slot
RM_X, RM_MASK, RM_IM, RM_PARAM, RM_IMG, RM_PRE, RM_STAT, RM_W1T, RM_R, RM_COUNT = range(10)


def stride_vector(count, slots):
    """A member-stride vector of `count` slots: `slots` = {slot: stride in elements}, every slot not named is 0."""
    v = [0] * count
    for k, s in slots.items():
        v[k] = s
    return v


def _member_strides(strides):
    return (C.c_long * len(strides))(*[int(v) for v in strides])


def step_small_multi_f32(x, mask, mask_p, eps, enc_img, dec_img, members, G, npass, nplanes, draw, offset_mask, offset_eps,
                         inv_B, x_logvar, partE, partD, loss_part, strides, B, d, Ld, order=0):
    """The small-batch step of G members in one launch (include/vpc.h: ensemble step).  Pointers are member 0's, `strides`
    the VPC_MS_* member strides in elements, `members` the device-resident VpcMember table."""
    check(lib().vpc_step_small_multi_f32(ptr(x), ptr(mask), ptr(mask_p), ptr(eps), ptr(enc_img), ptr(dec_img), ptr(members),
                                         G, npass, nplanes, int(bool(draw)), int(offset_mask), int(offset_eps), inv_B, x_logvar,
                                         ptr(partE), ptr(partD), ptr(loss_part), _member_strides(strides), B, d, Ld, int(order),
                                         stream_ptr()), "vpc_step_small_multi_f32")


def reduce_step_adam_multi(partE, partD, loss_part, blocks, strideE, strideD, strides, inv_maps, members, G, grad, B, d, out9,
                           accum, params, m, v, beta1, beta2, eps, step, pack_idx, img):
    """reduce_step_adam of G members in one launch (blockIdx.y = member; lr and loss coefficients from the member table)."""
    check(lib().vpc_reduce_step_adam_multi(ptr(partE), ptr(partD), ptr(loss_part), blocks, strideE, strideD,
                                           _member_strides(strides), ptr(inv_maps), ptr(members), G, ptr(grad), B, d, ptr(out9),
                                           ptr(accum), ptr(params), ptr(m), ptr(v), beta1, beta2, eps, int(step), ptr(pack_idx),
                                           ptr(img), stream_ptr()), "vpc_reduce_step_adam_multi")


# the slots the mask-augmented / point-net ensemble entries read behind the nine above (VPC_MS_PARTF, VPC_MS_SNAP)
MS_PARTF, MS_SNAP, MS_COUNT_FAMILIES = MS_COUNT, MS_COUNT + 1, MS_COUNT + 2


def _family_strides(strides):
    if len(strides) < MS_COUNT_FAMILIES:
        raise L.VpcError(f"the point-net ensemble entries read {MS_COUNT_FAMILIES} member strides, got {len(strides)}")
    return _member_strides(strides)


def step_small_multi_aug_f32(x, mask, mask_p, eps, enc_img, dec_img, members, G, npass, nplanes, draw, offset_mask, offset_eps,
                             inv_B, x_logvar, partE, partD, loss_part, strides, B, d, d_real, Ld, order=0):
    """step_small_multi_f32 for G Reg_VAE_mask / vanilla_VAE_mask members: `d` is the row pitch small_aug_pitch(d_real) of x and
    the masks, the images are those of the mask-augmented layout."""
    check(lib().vpc_step_small_multi_aug_f32(ptr(x), ptr(mask), ptr(mask_p), ptr(eps), ptr(enc_img), ptr(dec_img), ptr(members),
                                             G, npass, nplanes, int(bool(draw)), int(offset_mask), int(offset_eps), inv_B,
                                             x_logvar, ptr(partE), ptr(partD), ptr(loss_part), _member_strides(strides), B, d,
                                             d_real, Ld, int(order), stream_ptr()), "vpc_step_small_multi_aug_f32")


def step_small_multi_eddi_f32(x, mask, mask_p, eps, enc_img, dec_img, members, G, npass, nplanes, draw, offset_mask, offset_eps,
                              inv_B, x_logvar, partE, partD, loss_part, strides, B, d, d_real, Ld, K, front, partF, snap, order=0):
    """step_small_multi_f32 for G Reg_EDDI / vanilla_EDDI members: images of the point-net layout; front / partF / snap are member
    0's (step_small_eddi_f32), `strides` has MS_COUNT_FAMILIES slots (MS_PARAM: front, MS_PARTF, MS_SNAP)."""
    check(lib().vpc_step_small_multi_eddi_f32(ptr(x), ptr(mask), ptr(mask_p), ptr(eps), ptr(enc_img), ptr(dec_img), ptr(members),
                                              G, npass, nplanes, int(bool(draw)), int(offset_mask), int(offset_eps), inv_B,
                                              x_logvar, ptr(partE), ptr(partD), ptr(loss_part), _family_strides(strides), B, d,
                                              d_real, Ld, K, ptr(front), ptr(partF), ptr(snap), int(order), stream_ptr()),
          "vpc_step_small_multi_eddi_f32")


def reduce_step_adam_eddi_multi(partE, partD, loss_part, blocks, strideE, strideD, strides, inv_maps, members, G, grad, n, B, d,
                                out9, accum, params, m, v, beta1, beta2, eps, step, pack_idx, img, partF, snap, K, d_pitch):
    """reduce_step_adam_eddi of G members in one launch (blockIdx.y = member); n = trunk + decoder parameters of a row."""
    check(lib().vpc_reduce_step_adam_eddi_multi(ptr(partE), ptr(partD), ptr(loss_part), blocks, strideE, strideD,
                                                _family_strides(strides), ptr(inv_maps), ptr(members), G, ptr(grad), n, B, d,
                                                ptr(out9), ptr(accum), ptr(params), ptr(m), ptr(v), beta1, beta2, eps, int(step),
                                                ptr(pack_idx), ptr(img), ptr(partF), ptr(snap), K, d_pitch, stream_ptr()),
          "vpc_reduce_step_adam_eddi_multi")


def eval_small_multi_f32(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar, part,
                         strides, d, d_real, Ld, max_blocks=0):
    """The evaluate-stage forward of G members over the tiles of a tile table (include/vpc.h: ensemble evaluation): one record of
    5 doubles per (member, tile) into `part`.  Pointers are member 0's, `strides` the VPC_MS_* member strides in elements."""
    check(lib().vpc_eval_small_multi_f32(ptr(x), ptr(mask), ptr(eps), ptr(enc_img), ptr(dec_img), ptr(members), G, ptr(tiles),
                                         int(n_tiles), int(N), int(R), int(bool(draw)), int(offset), x_logvar, ptr(part),
                                         _member_strides(strides), d, d_real, Ld, int(max_blocks), stream_ptr()),
          "vpc_eval_small_multi_f32")


def eval_small_multi_aug_f32(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar, part,
                             strides, d, d_real, Ld, max_blocks=0):
    """eval_small_multi_f32 for G Reg_VAE_mask / vanilla_VAE_mask members: `d` is the row pitch small_aug_pitch(d_real) of x and
    the mask, the images are those of the mask-augmented layout."""
    check(lib().vpc_eval_small_multi_aug_f32(ptr(x), ptr(mask), ptr(eps), ptr(enc_img), ptr(dec_img), ptr(members), G, ptr(tiles),
                                             int(n_tiles), int(N), int(R), int(bool(draw)), int(offset), x_logvar, ptr(part),
                                             _member_strides(strides), d, d_real, Ld, int(max_blocks), stream_ptr()),
          "vpc_eval_small_multi_aug_f32")


def eval_small_multi_eddi_f32(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar, part,
                              strides, d, d_real, Ld, K, front, max_blocks=0):
    """eval_small_multi_f32 for G Reg_EDDI / vanilla_EDDI members: images of the point-net layout; `front` is member 0's
    front-end parameters, member g's strides[MS_PARAM] floats further (its row of the parameter stack)."""
    check(lib().vpc_eval_small_multi_eddi_f32(ptr(x), ptr(mask), ptr(eps), ptr(enc_img), ptr(dec_img), ptr(members), G, ptr(tiles),
                                              int(n_tiles), int(N), int(R), int(bool(draw)), int(offset), x_logvar, ptr(part),
                                              _member_strides(strides), d, d_real, Ld, int(K), ptr(front), int(max_blocks),
                                              stream_ptr()), "vpc_eval_small_multi_eddi_f32")


def eval_reduce_multi(part, batches, n_batches, passes, M, members, G, part_stride, n_tiles, d_real, out):
    """The tile records -> out[G][4] = (rmse, elbo, negll, negll_imp): per batch, mean over a pass's batches, mean over passes."""
    check(lib().vpc_eval_reduce_multi(ptr(part), ptr(batches), int(n_batches), ptr(passes), int(M), ptr(members), G,
                                      int(part_stride), int(n_tiles), d_real, ptr(out), stream_ptr()), "vpc_eval_reduce_multi")


def impute_small_multi_f32(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar, mode, out,
                           out_stride, strides, d, d_real, Ld, max_blocks=0):
    """The forward of eval_small_multi_f32, written instead of summed (include/vpc.h: ensemble acquisition): mode 0 x_hat
    [R][d_real] per member, mode 1 the target column's squared error [R] per member; members out_stride floats apart."""
    check(lib().vpc_impute_small_multi_f32(ptr(x), ptr(mask), ptr(eps), ptr(enc_img), ptr(dec_img), ptr(members), G, ptr(tiles),
                                           int(n_tiles), int(N), int(R), int(bool(draw)), int(offset), x_logvar, int(mode),
                                           ptr(out), int(out_stride), _member_strides(strides), d, d_real, Ld, int(max_blocks),
                                           stream_ptr()), "vpc_impute_small_multi_f32")


def impute_small_multi_aug_f32(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar, mode, out,
                               out_stride, strides, d, d_real, Ld, max_blocks=0):
    """impute_small_multi_f32 for G Reg_VAE_mask / vanilla_VAE_mask members (the forward of eval_small_multi_aug_f32)."""
    check(lib().vpc_impute_small_multi_aug_f32(ptr(x), ptr(mask), ptr(eps), ptr(enc_img), ptr(dec_img), ptr(members), G,
                                               ptr(tiles), int(n_tiles), int(N), int(R), int(bool(draw)), int(offset), x_logvar,
                                               int(mode), ptr(out), int(out_stride), _member_strides(strides), d, d_real, Ld,
                                               int(max_blocks), stream_ptr()), "vpc_impute_small_multi_aug_f32")


def impute_small_multi_eddi_f32(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar, mode, out,
                                out_stride, strides, d, d_real, Ld, K, front, max_blocks=0):
    """impute_small_multi_f32 for G Reg_EDDI / vanilla_EDDI members (the forward of eval_small_multi_eddi_f32: `front` is member
    0's front-end parameters, member g's strides[MS_PARAM] floats further)."""
    check(lib().vpc_impute_small_multi_eddi_f32(ptr(x), ptr(mask), ptr(eps), ptr(enc_img), ptr(dec_img), ptr(members), G,
                                                ptr(tiles), int(n_tiles), int(N), int(R), int(bool(draw)), int(offset), x_logvar,
                                                int(mode), ptr(out), int(out_stride), _member_strides(strides), d, d_real, Ld,
                                                int(K), ptr(front), int(max_blocks), stream_ptr()),
          "vpc_impute_small_multi_eddi_f32")


def target_mse_multi(sq, sq_stride, R, G, out, out_stride):
    """out[g * out_stride] = mean of sq[g * sq_stride + 0..R) in fp64, fixed order."""
    check(lib().vpc_target_mse_multi(ptr(sq), int(sq_stride), int(R), G, ptr(out), int(out_stride), stream_ptr()),
          "vpc_target_mse_multi")


def reward_scratch_multi(n, d, M):
    """(pre, stat, w1t) workspace floats PER MEMBER of reward_matrix_multi."""
    sizes = [C.c_long() for _ in range(3)]
    check(lib().vpc_reward_scratch_multi(n, d, M, *[C.byref(s) for s in sizes]), "vpc_reward_scratch_multi")
    return tuple(s.value for s in sizes)


def reward_matrix_multi(x, mask, im, W1, b1, enc_img, pre, stat, w1t, R, G, chunk, strides, n, d, Ld, M):
    """vpc_reward_matrix with blockIdx.y = member; `strides` the VPC_RM_* member strides, the workspaces hold `chunk` members."""
    check(lib().vpc_reward_matrix_multi(ptr(x), ptr(mask), ptr(im), ptr(W1), ptr(b1), ptr(enc_img), ptr(pre), ptr(stat), ptr(w1t),
                                        ptr(R), G, int(chunk), _member_strides(strides), n, d, Ld, M, stream_ptr()),
          "vpc_reward_matrix_multi")


REWARD_DENSE, REWARD_DENSE_MASK, REWARD_POINTNET = range(3)  # first-layer kinds (VPC_REWARD_* of include/vpc.h)
RM_AC, RM_COUNT_EX = RM_COUNT, RM_COUNT + 1  # the slot reward_matrix_multi_ex reads behind the nine above (VPC_RM_AC)


def reward_scratch_multi_ex(kind, n, d, M, K=0):
    """(pre, stat, w1t) workspace floats PER MEMBER of reward_matrix_multi_ex."""
    sizes = [C.c_long() for _ in range(3)]
    check(lib().vpc_reward_scratch_multi_ex(kind, n, d, M, K, *[C.byref(s) for s in sizes]), "vpc_reward_scratch_multi_ex")
    return tuple(s.value for s in sizes)


def reward_matrix_multi_ex(kind, x, mask, im, W1, b1, AC, K, w23, pre, stat, w1t, R, G, chunk, strides, n, d, Ld, M):
    """vpc_reward_matrix_ex with blockIdx.y = member (REWARD_DENSE_MASK / REWARD_POINTNET); `strides` has RM_COUNT_EX slots."""
    if len(strides) < RM_COUNT_EX:
        raise L.VpcError(f"reward_matrix_multi_ex reads {RM_COUNT_EX} member strides, got {len(strides)}")
    check(lib().vpc_reward_matrix_multi_ex(kind, ptr(x), ptr(mask), ptr(im), ptr(W1), ptr(b1), ptr(AC), int(K), ptr(w23), ptr(pre),
                                           ptr(stat), ptr(w1t), ptr(R), G, int(chunk), _member_strides(strides), n, d, Ld, M,
                                           stream_ptr()), "vpc_reward_matrix_multi_ex")


def eddi_fold_multi(front, front_stride, AC, AC_stride, G, d, K):
    """AC[g] [2][K][d] = the fold of member g's front-end (eddi.eddi_fold), read in place from the parameter stack."""
    check(lib().vpc_eddi_fold_multi(ptr(front), int(front_stride), ptr(AC), int(AC_stride), G, d, K, stream_ptr()),
          "vpc_eddi_fold_multi")


def acquire_multi(R, R_stride, mask, mask_stride, mask_pitch, mask2, mask2_stride, mask2_pitch, action, action_stride,
                  action_pitch, G, n, d):
    """Per (member, row): argmax of R (lowest index among the maxima) -> mask byte(s) set, action written."""
    check(lib().vpc_acquire_multi(ptr(R), int(R_stride), ptr(mask), int(mask_stride), mask_pitch, ptr(mask2), int(mask2_stride),
                                  mask2_pitch, ptr(action), int(action_stride), action_pitch, G, n, d, stream_ptr()),
          "vpc_acquire_multi")


def step_fused_applicable(B, d, Ld, npass):
    return bool(lib().vpc_step_fused_applicable(int(B), d, Ld, npass))


def step_pack_weights_bf16(flat, pack_idx_c, img_c):
    check(lib().vpc_step_pack_weights_bf16(ptr(flat), ptr(pack_idx_c), ptr(img_c), flat.numel(), stream_ptr()),
          "vpc_step_pack_weights_bf16")


def step_workspace_floats(B):
    return int(lib().vpc_step_workspace_floats(int(B)))


def step_fused_bf16(x, img_c, masks, maskB, co, eps, eps_ml, inv_B, x_logvar, partE, partD, loss_part, ws, d, Ld):
    """Whole step (encoder fwd + decoder + loss + all backward) in one launch; returns the number of partial blocks."""
    n = len(masks)
    nb = C.c_int(0)
    check(lib().vpc_step_fused_bf16(ptr(x), ptr(img_c), n, ptr_array(masks), ptr_array(maskB), co,
                                    ptr_array(eps), ptr(eps_ml), inv_B, x_logvar, ptr(partE), ptr(partD),
                                    ptr(loss_part), ptr(ws), C.byref(nb), x.shape[0], d, Ld, stream_ptr()), "vpc_step_fused_bf16")
    return nb.value


def loss_finalize(loss_part, nblocks, co, B_local, B_global, d, out9, accum=None):
    check(lib().vpc_loss_finalize(ptr(loss_part), nblocks, co, B_local, B_global, d, ptr(out9), ptr(accum), stream_ptr()),
          "vpc_loss_finalize")


def reduce_step(partE, nbE, strideE, partD, nbD, strideD, grad_idx, grad, n_enc, loss_part, nbL, co, B_local, B_global, d,
                out9, accum=None, state=None, rng_inc=0, inv_maps=None):
    check(lib().vpc_reduce_step(ptr(partE), nbE, strideE, ptr(partD), nbD, strideD, ptr(grad_idx), ptr(inv_maps),
                                ptr(grad), n_enc, grad.numel(), ptr(loss_part), nbL, co, B_local, B_global, d,
                                ptr(out9), ptr(accum), ptr(state), int(rng_inc), stream_ptr()), "vpc_reduce_step")


def reduce_step_adam(partE, nbE, strideE, partD, nbD, strideD, grad_idx, grad, n_enc, loss_part, nbL, co, B_local, B_global,
                     d, out9, accum, params, m, v, lr, beta1, beta2, eps, step, pack_idx, img, inv_maps=None, bf16c=False):
    """bf16c: (pack_idx, img) are the compact bf16 image tables of the whole-step kernel (re-packed instead of the fp32 images)."""
    fn = lib().vpc_reduce_step_adam_bf16c if bf16c else lib().vpc_reduce_step_adam
    check(fn(ptr(partE), nbE, strideE, ptr(partD), nbD, strideD, ptr(grad_idx), ptr(inv_maps), ptr(grad), n_enc, grad.numel(),
             ptr(loss_part), nbL, co, B_local, B_global, d, ptr(out9), ptr(accum), ptr(params), ptr(m), ptr(v), lr, beta1,
             beta2, eps, int(step), ptr(pack_idx), ptr(img), stream_ptr()), "vpc_reduce_step_adam")


def draw_mask(mask_in, mask_out, keep_prob, seed, offset, elem_lo=0):
    """elem_lo: index of mask_out[0] inside the global [B_global, d] array (data parallel: row_lo * d)."""
    check(lib().vpc_draw_mask(ptr(mask_in), ptr(mask_out), mask_out.numel(), float(keep_prob), int(seed), int(offset),
                              int(elem_lo), stream_ptr()), "vpc_draw_mask")


def _shard4(shard):
    """(rows_local, rows_global, row_lo, pitch) of a row-sharded eps array, or the flat form."""
    return (0, 0, 0, 4) if shard is None else tuple(int(v) for v in shard)


def draw_step(mask_in, mask_out, keep_prob, eps_out, seed, offset_mask, offset_eps, state=None, elem_lo=0,
              eps_shard=None):
    check(lib().vpc_draw_step(ptr(mask_in), ptr(mask_out), mask_out.numel(), float(keep_prob), ptr(eps_out),
                              eps_out.numel(), int(seed), int(offset_mask), int(offset_eps), ptr(state), int(elem_lo),
                              *_shard4(eps_shard), stream_ptr()), "vpc_draw_step")


def fill_normal(out, seed, offset, state=None, shard=None):
    check(lib().vpc_fill_normal(ptr(out), out.numel(), int(seed), int(offset), ptr(state), *_shard4(shard),
                                stream_ptr()), "vpc_fill_normal")


# ------------------------------------------------------------------------------------------------ autograd
class EncoderFn(torch.autograd.Function):
    """(x, mask, eps, 6 encoder tensors) -> (z, mean, logvar).  Reference: VAE.py:387-395."""

    @staticmethod
    def forward(ctx, model, x, mask_u8, eps, *weights):
        lay = model._lay()
        d, Ld = lay.d, lay.L
        require_cuda(x, mask_u8, eps, *weights)
        B = x.shape[0]
        dev = x.device
        h1 = torch.empty(B, H1P, device=dev)
        h2 = torch.empty(B, H2P, device=dev)
        mean = torch.empty(B, Ld, device=dev)
        logvar = torch.empty(B, Ld, device=dev)
        z = torch.empty(B, Ld, device=dev)
        encoder_fwd(x, model._enc_img(), [mask_u8], [eps], [h1], [h2], [mean], [logvar], [z], d, Ld,
                    mask_augm=lay.mask_augm)
        ctx.model = model
        ctx.save_for_backward(x, mask_u8, eps if eps is not None else torch.empty(0, device=dev), h1, h2, logvar)
        ctx.has_eps = eps is not None
        ctx.mark_non_differentiable()
        return z, mean, logvar

    @staticmethod
    def backward(ctx, dz, dmean, dlogvar):
        model = ctx.model
        lay = model._lay()
        x, mask_u8, eps, h1, h2, logvar = ctx.saved_tensors
        dev = x.device
        zero = None
        dm = dmean if dmean is not None else zero
        dl = dlogvar if dlogvar is not None else zero
        if dz is not None:
            dm = dz if dm is None else dm + dz
            if ctx.has_eps:  # z = mean + eps * exp(logvar / 2)
                t = dz * eps * (0.5 * torch.exp(0.5 * logvar))
                dl = t if dl is None else dl + t
        if dm is None:
            dm = torch.zeros_like(logvar)
        if dl is None:
            dl = torch.zeros_like(logvar)
        dm, dl = dm.contiguous(), dl.contiguous()
        part = model._partials(dev, "enc")
        nb = encoder_bwd(x, model._enc_img(), [mask_u8], [h1], [h2], [dm], [dl], part, lay.d, lay.L,
                         mask_augm=lay.mask_augm)
        flat = torch.empty(lay.n_enc, device=dev)
        _, gidx = lay.device_tables(dev)
        reduce_partials(part, nb, lay.enc_part, gidx[:lay.n_enc], flat)
        grads = model._split_flat(flat, 0, 6)
        return (None, None, None, None) + tuple(grads)


class RegEncoderFn(torch.autograd.Function):
    """Both encoder passes of Reg_VAE.forward (VAE.py:496-507: q with `mask`, p with `mask_p`) as ONE autograd node:
    one vpc_encoder_fwd launch forward (x is read once per tile for both passes), one vpc_encoder_bwd launch + one
    reduction backward - half the launches of two EncoderFn nodes, which is what the API path is bound by at the
    reference's batch sizes.  (x, mask, mask_p, eps_q, eps_p, 6 encoder tensors) -> (z_q, mean_q, logvar_q, z_p, mean_p,
    logvar_p)."""

    @staticmethod
    def forward(ctx, model, x, mq_u8, mp_u8, eps_q, eps_p, *weights):
        lay = model._lay()
        d, Ld = lay.d, lay.L
        require_cuda(x, mq_u8, mp_u8, eps_q, eps_p, *weights)
        B, dev = x.shape[0], x.device
        h1 = [torch.empty(B, H1P, device=dev) for _ in range(2)]
        h2 = [torch.empty(B, H2P, device=dev) for _ in range(2)]
        lat = torch.empty(2, 3, B, Ld, device=dev)  # [pass][mean | logvar | z]
        mean, logvar, z = [lat[0, 0], lat[1, 0]], [lat[0, 1], lat[1, 1]], [lat[0, 2], lat[1, 2]]
        encoder_fwd(x, model._enc_img(), [mq_u8, mp_u8], [eps_q, eps_p], h1, h2, mean, logvar, z, d, Ld,
                    mask_augm=lay.mask_augm)
        # d z / d logvar = eps * exp(logvar / 2) / 2 for both passes (None eps: z = mean)
        eps = torch.stack([e if e is not None else torch.zeros(B, Ld, device=dev) for e in (eps_q, eps_p)])
        fac = eps * torch.exp(0.5 * lat[:, 1]) * 0.5
        ctx.model = model
        ctx.save_for_backward(x, mq_u8, mp_u8, h1[0], h1[1], h2[0], h2[1], fac)
        return z[0], mean[0], logvar[0], z[1], mean[1], logvar[1]

    @staticmethod
    def backward(ctx, dzq, dmq, dlq, dzp, dmp, dlp):
        model = ctx.model
        lay = model._lay()
        x, mq_u8, mp_u8, h1q, h1p, h2q, h2p, fac = ctx.saved_tensors
        dev, B, Ld = x.device, x.shape[0], lay.L
        seeds = torch.zeros(2, 2, B, Ld, device=dev)  # [pass][dmean | dlogvar], reparameterisation path folded in
        for p, (dz, dm, dl) in enumerate(((dzq, dmq, dlq), (dzp, dmp, dlp))):
            if dm is not None:
                seeds[p, 0] += dm
            if dl is not None:
                seeds[p, 1] += dl
            if dz is not None:
                seeds[p, 0] += dz
                seeds[p, 1].addcmul_(dz, fac[p])
        part = model._partials(dev, "enc")
        nb = encoder_bwd(x, model._enc_img(), [mq_u8, mp_u8], [h1q, h1p], [h2q, h2p], [seeds[0, 0], seeds[1, 0]],
                         [seeds[0, 1], seeds[1, 1]], part, lay.d, lay.L, mask_augm=lay.mask_augm)
        flat = torch.empty(lay.n_enc, device=dev)
        _, gidx = lay.device_tables(dev)
        reduce_partials(part, nb, lay.enc_part, gidx[:lay.n_enc], flat)
        grads = model._split_flat(flat, 0, 6)
        return (None, None, None, None, None, None) + tuple(grads)


class DecoderFn(torch.autograd.Function):
    """(z, 6 decoder tensors) -> xhat.  Reference: VAE.py:397-401."""

    @staticmethod
    def forward(ctx, model, z, *weights):
        lay = model._lay()
        require_cuda(z, *weights)
        z = _f32c(z)
        xhat = torch.empty(z.shape[0], lay.d, device=z.device)
        decoder_fwd(z, model._dec_img(), xhat, lay.d, lay.L)
        ctx.model = model
        ctx.save_for_backward(z)
        return xhat

    @staticmethod
    def backward(ctx, dxhat):
        model = ctx.model
        lay = model._lay()
        (z,) = ctx.saved_tensors
        dev = z.device
        dz = torch.empty_like(z)
        part = model._partials(dev, "dec")
        nb = decoder_bwd(z, dxhat.contiguous(), model._dec_img(), dz, part, lay.d, lay.L)
        flat = torch.empty(lay.n_params - lay.n_enc, device=dev)
        _, gidx = lay.device_tables(dev)
        reduce_partials(part, nb, lay.dec_part, gidx[lay.n_enc:], flat)
        grads = model._split_flat(flat, 6, 12)
        return (None, dz) + tuple(grads)


class LossFn(torch.autograd.Function):
    """K4: fused ELBO / consistency loss on materialised tensors.  Returns (loss, sums[8]) where loss is the
    reference's train_loss (already / B) and sums are the raw partial sums (see include/vpc.h)."""

    @staticmethod
    def forward(ctx, cfg, x, xq, xp, mq, lq, mp, lp, eps_ml):
        # cfg: dict(maskA=[..], maskB=[..], cA=[..], cE=[..], bq, bp, cr, wml, x_logvar, d, L)
        two = xp is not None
        xs = [xq, xp] if two else [xq]
        ms = [mq, mp] if two else [mq]
        ls = [lq, lp] if two else [lq]
        require_cuda(x, *xs, *ms, *ls)
        B, d, Ld = x.shape[0], cfg["d"], cfg["L"]
        dev = x.device
        need_grad = any(t.requires_grad for t in xs + ms + ls)
        dx = [torch.empty_like(t) for t in xs] if need_grad else None
        dm = [torch.empty_like(t) for t in ms] if need_grad else None
        dl = [torch.empty_like(t) for t in ls] if need_grad else None
        max_blocks = L.num_cus() * 8
        lp_buf = torch.empty(max_blocks, 8, dtype=torch.float64, device=dev)
        n = len(xs)  # (the entries of the passes that run)
        co = L.VpcLossCoef(cfg["cA"][:n], cfg["cE"][:n], cfg["bq"], cfg["bp"], cfg["cr"], cfg["wml"])
        nb = loss_fwd_bwd(x, xs, cfg["maskA"], cfg["maskB"], co, ms, ls, eps_ml, 1.0 / B, cfg["x_logvar"], dx, dm, dl, lp_buf,
                          d, Ld)
        # block partials -> [loss | 8 raw sums] in ONE launch (vpc_loss_finalize: doubles inside, fixed order): the torch
        # expression it replaces was ~15 tiny launches per loss() call - the API path is launch-bound at the reference's
        # batch sizes
        out9 = torch.empty(9, device=dev)
        loss_finalize(lp_buf, nb, co, B, B, d, out9)
        loss, sums = out9[0], out9[1:]
        ctx.two = two
        if need_grad:
            ctx.save_for_backward(*(dx + dm + dl))
        ctx.need_grad = need_grad
        ctx.mark_non_differentiable(sums)
        return loss, sums

    @staticmethod
    def backward(ctx, gloss, _gsums):
        if not ctx.need_grad:
            return (None,) * 9
        t = ctx.saved_tensors
        n = 2 if ctx.two else 1
        g = torch._foreach_mul(list(t), gloss)  # one launch for all seeds (gloss is a device scalar: usually 1)
        if ctx.two:
            dxq, dxp, dmq, dmp, dlq, dlp = g
            return None, None, dxq, dxp, dmq, dlq, dmp, dlp, None
        dxq, dmq, dlq = g
        return None, None, dxq, None, dmq, dlq, None, None, None
