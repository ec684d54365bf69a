"""Reg_VAE / vanilla_VAE for encoder inputs wider than the 128 columns the register-chained kernels tile
(obs_dim > 128, or the mask-augmented classes with 2 * obs_dim > 128) - the reference takes any obs_dim
(src/models/VAE.py:366-376, 527-533; "UCI gas" with its target column appended is d = 129).

Same API path, same loss kernel (K4: vpc_loss_fwd_bwd has no width limit); the six affine layers run on the generic
fp32 MFMA GEMMs of the MNAR path (vpc_linear_fwd / _dgrad / _wgrad: any M, N, K, bias + ReLU / Sigmoid epilogues, ReLU'
and Sigmoid' gates in the backward GEMMs), the encoder input x * mask and the reparameterisation on the small
elementwise kernels of that path (vpc_nm_mul, vpc_nm_sample with K = 1).  Activations go through HBM between layers,
so this is the unfused design of SURVEY.md section 8(d) - correct at any width, not the throughput path.
The API path is the chain-family autograd frame (chainfamily.ChainEncoderFn / ChainDecoderFn) with FAMILY below; the chains
themselves are _VAEBase._build_chains.  `WideTrainer` is the training-step object for these models (train.py:53-117):
device-side draws, the API-path forward, K4, backward, flat Adam, no host synchronisation.
"""
from __future__ import annotations

import torch

from . import ops
from .chainfamily import ChainDecoderFn, ChainEncoderFn, Family, gauss_sample, gauss_sample_bwd, nm_mul
from .linear import _f32c
from .models import _W6
from .ops import as_mask_u8
from .trainer import _FlatAdamTrainer, draw_counters


def _enc_input(x, mask_u8, out, B, d):
    """x * mask, or [x * mask | mask] for the mask-augmented classes (VAE.py:388, 545-548), into the chain's input buffer."""
    mf = mask_u8.float()
    if out.shape[1] == d:
        nm_mul(x, mf, out)
    else:
        xin = torch.empty_like(x)
        nm_mul(x, mf, xin)
        torch.cat([xin, mf], 1, out=out)


# the decoder returns xhat, one [M, d] buffer behind the chain's Sigmoid gate (VAE.py:397-401)
FAMILY = Family(_W6[:6], _W6[6:], _enc_input, gauss_sample, gauss_sample_bwd, 1)


def encode(model, x, mask_u8, eps):
    """_VAEBase._encode of a wide model: (z, mean, logvar), the statistics as the two halves of the encoder's heads."""
    z, heads = ChainEncoderFn.apply(FAMILY, model, x, mask_u8, None if eps is None else _f32c(eps), 1, *model._enc_weights())
    return (z, *heads.chunk(2, dim=1))  # mean first (VAE.py:391); one split node, whose backward is one cat


def decode(model, z):
    return ChainDecoderFn.apply(FAMILY, model, z, *model._dec_weights())


class WideTrainer(_FlatAdamTrainer):
    """Training step (train.py:53-117) for the wide models: on-device mask_p / eps draws, the API-path forward and K4
    loss, backward, flat Adam (vpc_adam_step on the flat parameter buffer), loss accumulated on the device.  Mirrors
    FusedTrainer's interface (step / loss_value / epoch_total); data parallel as there: ONE all-reduce of [grads | loss]."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, process_group=None, world_size=1, rank=0):
        super().__init__(model, lr, betas, eps, seed, process_group, world_size, rank, 1)
        self.loss = self.tail
        self.vanilla = not model.regularised

    def step(self, x, mask, mask_p=None, eps_q=None, eps_p=None, *, epoch=1, alpha=1.0, beta=1.0, beta_annealing=False,
             p_missingness=30, global_batch=None, row_lo=None):
        m = self.model
        x = _f32c(x)
        B, d, Ld = x.shape[0], m.obs_dim, m.latent_dim
        Bg, row_lo = self._batch_rows(B, global_batch, row_lo)
        mu8 = as_mask_u8(mask)
        two = not self.vanilla
        n_eps = 2 if two else 1
        draw_mask, draw_eps = two and mask_p is None, eps_q is None or (two and eps_p is None)
        # Philox counters of the GLOBAL row
        dr = draw_counters(self.rng_offset, draw_mask, n_eps if draw_eps else 0, B, Bg, row_lo, 4 * ((Ld + 3) // 4), d)
        self.rng_offset = dr.next_offset
        if draw_mask:
            mask_p = torch.empty(B, d, dtype=torch.uint8, device=self.dev)
            ops.draw_mask(mu8, mask_p, 1.0 - p_missingness / 100.0, self.seed, dr.offset_mask, dr.elem_lo)
        if draw_eps:
            e = torch.empty(n_eps, B, dr.eps_shard[3], device=self.dev)
            ops.fill_normal(e, self.seed, dr.offset_eps, None, dr.eps_shard)
            eps_q = e[0, :, :Ld].contiguous() if eps_q is None else eps_q
            eps_p = (e[1, :, :Ld].contiguous() if eps_p is None else eps_p) if two else None
        for p in m.trainable():
            p.grad = None
        t = m.trainable()
        zq, mq, lq = m._encode(x, mu8, eps=eps_q)
        xq = decode(m, zq)
        if two:
            mpu8 = as_mask_u8(mask_p)
            zp, mp_, lp = m._encode(x, mpu8, eps=eps_p)
            xp = decode(m, zp)
            _, tl = m.loss(x, xp, m.x_logvar, mp_, lp, xq, m.x_logvar, mq, lq, mu8, mpu8, epoch, beta_annealing=beta_annealing,
                           beta=beta, alpha=alpha, stage="train")
        else:
            _, tl = m.loss(x, xq, m.x_logvar, mq, lq, epoch, mu8, beta_annealing=beta_annealing, beta=beta, stage="train")
        tl = tl * (B / Bg)  # every rank normalises by the GLOBAL batch: SUM over ranks = the concatenated batch
        tl.backward()
        off = 0
        for p in t:
            self.grad[off:off + p.numel()].copy_(p.grad.reshape(-1))
            off += p.numel()
        self.loss.copy_(tl.detach().reshape(1))
        if self.world_size > 1:
            self._allreduce()
        self._adam(None, self.loss, self.accum)
