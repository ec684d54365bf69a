"""Flow path (Data/imputation_args.json runs vanilla_flow* / reg_flow*): drop-in classes for the reference's

    VAEFlow       src/models/VAE.py:1860-1996
    REG_VAEFlow   src/models/VAE.py:1999-2124

with the same constructor arguments, `encoder` / `decoder` / `forward` / `loss` signatures, return order and state_dict
keys (prior_mean, prior_std, flow.flows.{0,1,2}.unnormalized_pdf, seq_encoder.{0,2,4}, encoder_mean, encoder_logvar,
seq_decoder.{0,2,4,6}, decoder_mean.0, decoder_logvar.0).  The eight live layers run as fp32 MFMA GEMMs
(csrc/vpc_gemm.hip, ELU between layers, Sigmoid on decoder_mean); the per-step draws, the three-layer piecewise-linear
CDF posterior (Flow :1816-1854) and the loss with all of its gradients are csrc/vpc_flow.hip.  The 16 tensors that get
a gradient are views of one flat fp32 buffer; the 9 that never get one in the reference (the three unnormalized_pdf,
encoder_mean, encoder_logvar, decoder_logvar) stay ordinary parameters outside it, so no optimiser touches them.  No CPU
fallback: CPU tensors raise.

The reference's spline quirks are reproduced, not fixed (csrc/vpc_flow.hip): the context is masked in place with the
latent mask on the bin axis, inputs outside [-1, 1] are zeroed and splined, and a pass with no inside draw is the
identity.  latent_dim must be 10 (the reference's hard-coded 10 x 10 reshape).

FlowEvaluator (below, csrc/vpc_floweval.hip) is eval_vae's estimator for one flow model with every batch of every Monte-Carlo
pass in one set of launches: eval_vae(engine="batched").

What this family shares with notmiwae.py and miwae.py lives in chainfamily.py: the encoder / decoder autograd frame (driven
by FAMILY below) and the trainer frame.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import check, lib, ptr, require_cuda, stream_ptr
from .chainfamily import ChainDecoderFn, ChainEncoderFn, Family, _ChainTrainer
from .images import FlatParams, mlp_spec
from .linear import (ACT_ELU, ACT_NONE, ACT_SIGMOID_HARDTANH, _f32c, chain, chain_bwd, chain_bwd_rows, chain_fwd,
                     chain_fwd_rows)
from .trainer import chain_draw_increment, flow_eval_draw_counters

FLOW_L = 10      # VPC_FLOW_LATENT: latent dim = spline bins
CTX = 100        # seq_encoder output = the 10 x 10 spline contexts
OBS_LOGVAR = -8.0  # VAE.py:1875 / :2014
STAGE_TRAIN, STAGE_EVAL = 0, 1


# ------------------------------------------------------------------------------------------------ raw ops
def flow_prep(x, mask, mask_p_in, mask_p_out, xin, eps_out, B, d, keep_prob=1.0, seed=0, offset=0, offset_eps=0):
    check(lib().vpc_flow_prep(ptr(x), ptr(mask), ptr(mask_p_in), ptr(mask_p_out), ptr(xin), ptr(eps_out),
                              0 if eps_out is None else eps_out.numel(), int(B), int(d), float(keep_prob), int(seed),
                              int(offset), int(offset_eps), stream_ptr()), "vpc_flow_prep")


def flow_fwd(t, eps, z, zlp, R, B, ldt=CTX):
    check(lib().vpc_flow_fwd(ptr(t), int(ldt), ptr(eps), ptr(z), ptr(zlp), int(R), int(B), stream_ptr()), "vpc_flow_fwd")


def flow_bwd(t, eps, dz, dz2, dzlp, dt, R, B, ldt=CTX, lddt=CTX):
    """ldt / lddt: row pitch in floats of t / dt (>= CTX)."""
    check(lib().vpc_flow_bwd(ptr(t), int(ldt), ptr(eps), ptr(dz), ptr(dz2), ptr(dzlp), ptr(dt), int(lddt), int(R), int(B),
                             stream_ptr()), "vpc_flow_bwd")


def flow_loss_scratch(B, device):
    nbytes = int(lib().vpc_flow_loss_scratch(int(B)))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def flow_loss(x, mask, mask_p, xm, z, zlp, g, scratch, out8, loss_f32, accum, B, d, stage, alpha, beta, gscale, gated,
              ldxm=None, ldg=None):
    """xm, z, zlp: (q, p) pairs (p may be None); g: None or (gxm_q, gxm_p, gz_q, gz_p, gzlp_q, gzlp_p)."""
    g = (None,) * 6 if g is None else g
    check(lib().vpc_flow_loss(ptr(x), ptr(mask), ptr(mask_p), ptr(xm[0]), ptr(xm[1]), int(ldxm or d), ptr(z[0]),
                              ptr(z[1]), ptr(zlp[0]), ptr(zlp[1]), *[ptr(t) for t in g[:2]], int(ldg or d),
                              *[ptr(t) for t in g[2:]], ptr(scratch), scratch.numel() * scratch.element_size(),
                              ptr(out8), ptr(loss_f32), ptr(accum), int(B), int(d), int(stage), float(alpha),
                              float(beta), float(gscale), int(gated), stream_ptr()), "vpc_flow_loss")


def _host_table(values):
    """A table as the batched-evaluation entries take its host side: an int64 CPU tensor (the library checks it before it
    launches anything; the kernels read a device copy)."""
    return torch.tensor([int(v) for v in values], dtype=torch.int64)


def flow_fwd_tiles(t, eps, z, zlp, R, tab, tab_dev, ldt=CTX):
    """tab / tab_dev: tile_row0 [n_tiles + 1] as an int64 CPU tensor and its device copy."""
    check(lib().vpc_flow_fwd_tiles(ptr(t), int(ldt), ptr(eps), ptr(z), ptr(zlp), int(R), ptr(tab), ptr(tab_dev),
                                   (0 if tab is None else tab.numel()) - 1, stream_ptr()), "vpc_flow_fwd_tiles")


def flow_eval_tiles_scratch(max_tile_rows, n_tiles, device):
    nbytes = int(lib().vpc_flow_eval_tiles_scratch(int(max_tile_rows), int(n_tiles)))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def flow_eval_tiles(x, mask, xm, z, zlp, R, d, tab, tab_dev, beta, scratch, stats, ldxm=None):
    check(lib().vpc_flow_eval_tiles(ptr(x), ptr(mask), ptr(xm), int(ldxm or d), ptr(z), ptr(zlp), int(R), int(d), ptr(tab),
                                    ptr(tab_dev), (0 if tab is None else tab.numel()) - 1, float(beta), ptr(scratch),
                                    0 if scratch is None else scratch.numel() * scratch.element_size(), ptr(stats),
                                    stream_ptr()), "vpc_flow_eval_tiles")


def flow_eval_finalize(stats, n_tiles, ptab, ptab_dev, out4):
    check(lib().vpc_flow_eval_finalize(ptr(stats), int(n_tiles), ptr(ptab), ptr(ptab_dev),
                                       (0 if ptab is None else ptab.numel()) - 1, ptr(out4), stream_ptr()),
          "vpc_flow_eval_finalize")


def _mask_f32(m, d, device):
    return _f32c(m.reshape(-1, d).to(device))


# ------------------------------------------------------------------------------------------------ autograd
_ENC_NAMES = ("We1", "be1", "We2", "be2", "We3", "be3")
_DEC_NAMES = ("Wd1", "bd1", "Wd2", "bd2", "Wd3", "bd3", "Wd4", "bd4", "Wm", "bm")


def _chains(v):
    """(encoder, decoder) chains on the named views v: ELU between layers, raw contexts, Sigmoid on decoder_mean."""
    return (chain([v[k] for k in _ENC_NAMES], (ACT_ELU, ACT_ELU, ACT_NONE)),
            chain([v[k] for k in _DEC_NAMES], (ACT_ELU,) * 4 + (ACT_SIGMOID_HARDTANH,), v["Wm"].shape[0]))


def _sample(t, eps, B, S, Ld):
    """Flow.forward on the contexts t (VAE.py:1924-1931) -> (z, z_log_prob) [B, 10]."""
    z, zlp = torch.empty(B, FLOW_L, device=t.device), torch.empty(B, FLOW_L, device=t.device)
    flow_fwd(t, eps, z, zlp, B, B)
    return z, zlp


# encoder input cat[x * mask, mask]; the decoder returns x_mean = sigmoid(decoder_mean(seq_decoder(z))) (VAE.py:1943-1948)
FAMILY = Family(_ENC_NAMES, _DEC_NAMES, lambda x, mask, out, B, d: flow_prep(x, mask, None, None, out, None, B, d), _sample,
                lambda t, eps, dz, dzlp, dt, B, S, Ld: flow_bwd(t, eps, dz, None, dzlp, dt, B, B), 1)


class FlowLossFn(torch.autograd.Function):
    """The loss and, with grad enabled, every gradient in the same launch pair (vpc_flow_loss, gated = 0).
    Returns (loss = the unscaled sum, fp32; out8)."""

    @staticmethod
    def forward(ctx, cfg, x, mask, mask_p, xm_q, z_q, zlp_q, xm_p, z_p, zlp_p):
        reg = mask_p is not None
        require_cuda(x, mask, mask_p, xm_q, z_q, zlp_q, xm_p, z_p, zlp_p)
        B, d, dev = cfg["B"], cfg["d"], x.device
        need_grad = cfg["grad"] and any(ctx.needs_input_grad)
        e = lambda *s: torch.empty(*s, device=dev)
        g = None
        if need_grad:
            g = (e(B, d), e(B, d) if reg else None, e(B, FLOW_L), e(B, FLOW_L) if reg else None, e(B, FLOW_L),
                 e(B, FLOW_L) if reg else None)
        out8 = torch.empty(8, dtype=torch.float64, device=dev)
        flow_loss(x, mask, mask_p, (xm_q, xm_p), (z_q, z_p), (zlp_q, zlp_p), g, flow_loss_scratch(B, dev), out8, None,
                  None, B, d, cfg["stage"], cfg["alpha"], cfg["beta"], 1.0, 0)
        ctx.reg, ctx.need_grad = reg, need_grad
        if need_grad:
            ctx.save_for_backward(*[t for t in g if t is not None])
        ctx.mark_non_differentiable(out8)
        return out8[0].float(), out8

    @staticmethod
    def backward(ctx, gloss, _g8):
        if not ctx.need_grad:
            return (None,) * 10
        t = [u * gloss for u in ctx.saved_tensors]
        if ctx.reg:  # saved: gxm_q, gxm_p, gz_q, gz_p, gzlp_q, gzlp_p
            return None, None, None, None, t[0], t[2], t[4], t[1], t[3], t[5]
        return None, None, None, None, t[0], t[1], t[2], None, None, None


# ------------------------------------------------------------------------------------------------ model classes
class _PiecewiseLinearCDF(nn.Module):
    """Holds the reference's never-read `unnormalized_pdf` (VAE.py:1781-1789: the context replaces it)."""

    def __init__(self, shape, num_bins=10):
        super().__init__()
        self.unnormalized_pdf = nn.Parameter(torch.randn(*shape, num_bins))


class _Flow(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.flows = nn.ModuleList([_PiecewiseLinearCDF((dim,)) for _ in range(3)])


class _FlowBase(FlatParams, nn.Module):
    regularised, X_MEAN_Q = False, 2  # forward takes mask_p; index of the q pass's reconstruction mean in forward's tuple
    _ENC_NAMES, _DEC_NAMES = _ENC_NAMES, _DEC_NAMES
    # flat parameter buffer: [We1 be1 We2 be2 We3 be3 | Wd1 bd1 .. Wd4 bd4 Wm bm] = state_dict order of the 16 tensors that get
    # a gradient; the other 9 stay ordinary parameters outside it
    _flat_spec = mlp_spec(_ENC_NAMES, "seq_encoder", "enc") + mlp_spec(_DEC_NAMES[:8], "seq_decoder", "dec") + \
        mlp_spec(_DEC_NAMES[8:], "decoder_mean", "dec")
    _build_chains = staticmethod(_chains)

    def __init__(self, obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples=1, num_estimates=1):
        super().__init__()
        if latent_dim != FLOW_L:
            raise L.VpcError(f"latent_dim {latent_dim}: the flow posterior reshapes its context to [B, 10, 10] "
                             "(VAE.py:1793); only latent_dim = 10 exists in the reference")
        self.obs_dim = obs_dim
        self.hid_dim = hid_dim
        self.latent_dim = latent_dim
        self.K = K
        self.num_samples = num_samples
        self.num_estimates = num_estimates
        self.obs_logvar = -8
        self.training_parameters = training_parameters
        d, H, Ld = obs_dim, hid_dim, latent_dim
        # created in the reference's order (same seed -> same initial weights)
        self.flow = _Flow(Ld)
        self.seq_encoder = nn.Sequential(nn.Linear(2 * d, H), nn.ELU(), nn.Linear(H, H), nn.ELU(), nn.Linear(H, CTX))
        self.encoder_mean = nn.Linear(H, Ld)
        self.encoder_logvar = nn.Linear(H, Ld)
        self.seq_decoder = nn.Sequential(nn.Linear(Ld, H), nn.ELU(), nn.Linear(H, H), nn.ELU(), nn.Linear(H, H),
                                         nn.ELU(), nn.Linear(H, H), nn.ELU())
        self.decoder_mean = nn.Sequential(nn.Linear(H, d), nn.Sigmoid())
        self.decoder_logvar = nn.Sequential(nn.Linear(H, d))
        self.prior_mean = nn.Parameter(torch.zeros(Ld), requires_grad=False)
        self.prior_std = nn.Parameter(torch.ones(Ld), requires_grad=False)
        self._flat = None

    @property
    def prior(self):  # VAE.py:1920 (Normal(prior_mean, prior_std))
        return torch.distributions.Normal(self.prior_mean, self.prior_std)

    # ---- reference API
    def _encode(self, x, mask, sample=True, eps=None):
        """encoder() with an optional injected draw eps [B, 10] (Flow.forward's rsample, VAE.py:1824-1827)."""
        if not sample:
            raise NotImplementedError("encoder(sample=False) reads an undefined `mean` in the reference (VAE.py:1930)")
        L.require_cuda(x)
        d = self.obs_dim
        xf = _f32c(x.reshape(-1, d))
        mf = _mask_f32(mask, d, xf.device)
        B = xf.shape[0]
        if eps is None:
            eps = torch.randn(B, FLOW_L, device=xf.device)
        return ChainEncoderFn.apply(FAMILY, self, xf, mf, _f32c(eps), 1, *self._enc_weights())

    def encoder(self, x, mask, sample=True):
        """VAE.py:1924-1931 / :2047-2056 -> (z, z_log_prob), each [B, 10]."""
        return self._encode(x, mask, sample)

    def backward(self, z, x, mask):
        raise NotImplementedError("the flow inverse (VAE.py:1933-1941) is not on the accelerated path: no reference "
                                  "driver calls it")

    def decoder(self, z_int):
        """VAE.py:1943-1948 -> (x_mean, x_logvar); x_logvar is the constant obs_logvar (the decoder_logvar GEMM, whose
        result the reference discards, is not run)."""
        L.require_cuda(z_int)
        x_mean = ChainDecoderFn.apply(FAMILY, self, z_int, *self._dec_weights())
        return x_mean, torch.full_like(x_mean, float(self.obs_logvar))

    def _loss(self, x, mask, mask_p, q, p, alpha, beta, stage):
        d = self.obs_dim
        xf = _f32c(x.reshape(-1, d))
        B = xf.shape[0]
        mf = _mask_f32(mask, d, xf.device)
        mpf = None if mask_p is None else _mask_f32(mask_p, d, xf.device)
        cfg = dict(B=B, d=d, alpha=alpha, beta=beta, stage=stage, grad=torch.is_grad_enabled())
        c = lambda t: None if t is None else _f32c(t).reshape(B, -1)
        xm_p, z_p, zlp_p = (None, None, None) if p is None else p
        return FlowLossFn.apply(cfg, xf, mf, mpf, c(q[0]), c(q[1]), c(q[2]), c(xm_p), c(z_p), c(zlp_p))

    def forward_loss(self, x, mask, mask_p=None, *, epoch=1, alpha=1.0, beta=1.0, beta_annealing=False, alpha_annealing=True,
                     stage="train", llh_eval=False):
        """forward, then loss, wired as the reference's drivers wire them: the flows take neither
        epoch nor beta from the schedule."""
        if self.regularised:  # train.py:53-55, 77-81; evaluate.py:172-173, 189-195
            o = self.forward(x, mask, mask_p)
            return o, self.loss(x, o[6], o[7], o[4], o[5], o[2], o[3], o[0], o[1], mask, mask_p, alpha, llh_eval=llh_eval,
                                stage=stage)
        o = self.forward(x, mask)  # train.py:82-85; evaluate.py:196-200
        return o, self.loss(x, o[2], o[3], o[0], o[1], mask, llh_eval=llh_eval)

    @staticmethod
    def neg_gaussian_log_likelihood(targets, mean, log_var):  # VAE.py:1987-1989 (elementwise; not on the hot path)
        return -torch.distributions.Normal(mean, torch.exp(log_var / 2.)).log_prob(targets)


class VAEFlow(_FlowBase):
    """VAE with a three-layer piecewise-linear CDF flow posterior.  Reference: src/models/VAE.py:1860-1996."""

    def forward(self, data, mask):
        z, z_log_prob = self.encoder(data, mask)
        x_mean, x_logvar = self.decoder(z)
        return z, z_log_prob, x_mean, x_logvar

    def loss(self, x, x_recon, x_logvar, z, z_log_prob, mask, vae_elbo=False, beta=1.0, llh_eval=False):
        """VAE.py:1950-1969 -> (print_loss = the unscaled sum, train_loss = sum / B) [+ (RE_ / B, RE_q_imputed / B)]."""
        loss, out8 = self._loss(x, mask, None, (x_recon, z, z_log_prob), None, 0.0, beta, STAGE_TRAIN)
        B = x.reshape(-1, self.obs_dim).shape[0]
        train_loss = loss / B
        if llh_eval:
            return loss, train_loss, (out8[1] / B).float(), (out8[7] / B).float()
        return loss, train_loss


class REG_VAEFlow(_FlowBase):
    """Posterior-consistency regularised VAEFlow.  Reference: src/models/VAE.py:1999-2124."""
    regularised, X_MEAN_Q = True, 6

    def forward(self, data, mask, mask_p):
        # VAE.py:2118-2124: both encoders first (RNG order q, p), p outputs returned first
        z_q, z_log_prob_q = self.encoder(data, mask)
        z_p, z_log_prob_p = self.encoder(data, mask_p)
        x_mean_q, x_logvar_q = self.decoder(z_q)
        x_mean_p, x_logvar_p = self.decoder(z_p)
        return z_p, z_log_prob_p, x_mean_p, x_logvar_p, z_q, z_log_prob_q, x_mean_q, x_logvar_q

    def loss(self, x, x_recon_q, x_logvar_q, z_q, z_log_prob_q, x_recon_p, x_logvar_p, z_p, z_log_prob_p, mask, mask_p,
             alpha, beta=1.0, llh_eval=False, stage="train"):
        """VAE.py:2075-2111.  train: loss_q + alpha (KL_reg - loss_q + loss_p + NLL(x*mask*~mask_p)); otherwise loss_q.
        Returns (train_loss, train_loss) [+ (RE_q / B, RE_q_imputed / B)], train_loss = loss / B."""
        st = STAGE_TRAIN if stage == "train" else STAGE_EVAL
        loss, out8 = self._loss(x, mask, mask_p, (x_recon_q, z_q, z_log_prob_q), (x_recon_p, z_p, z_log_prob_p), alpha,
                                beta, st)
        B = x.reshape(-1, self.obs_dim).shape[0]
        train_loss = loss / B
        if llh_eval:
            imp = (out8[7] / B).float() if st == STAGE_EVAL else 0 / B  # RE_q_imputed = 0 in the train stage
            return train_loss, train_loss, (out8[1] / B).float(), imp
        return train_loss, train_loss


# ------------------------------------------------------------------------------------------------ fused step
# timer names of the chain launches, per layer, and the weight gradients' (timer name, index in the trainer's workspace)
_T_ENC_FWD, _T_ENC_BWD, _T_DEC_FWD, _T_DEC_BWD = ("enc_fwd",) * 3, ("enc_bwd",) * 3, ("dec_fwd",) * 5, ("dec_bwd",) * 5
_DEC_WKEYS = tuple(("dec_bwd", 4 - i) for i in range(5))
_ENC_WKEYS = tuple(("enc_bwd", 7 - i) for i in range(3))

SMALL_MAX_ROWS, SMALL_MAX_WIDTH = 128, 1024  # limits of csrc/vpc_rows.hip (vpc_rows_max_rows(); N, K <= 1024)
# The row limit of the small-batch step, in stacked rows R = P * B.  The step without VPC_FLOW_SMALL in the environment stays the
# launch chain (tests/test_trainer_images.py pins the chain's 29 calls as FlowTrainer's step at B = 64), so the default is 0;
# SMALL_ROWS_MEASURED is the largest R at which the small path's worst block beat the chain's best block
# (profiles/flow_small_notes.md) - the value to put into VPC_FLOW_SMALL.
SMALL_ROWS_DEFAULT = 0
SMALL_ROWS_MEASURED = 128


def small_max_rows():
    """The row limit of the small-batch step: VPC_FLOW_SMALL in the environment (stacked rows P * B; 0 = never), read per
    step; SMALL_ROWS_DEFAULT (0: the chain) without it."""
    v = os.environ.get("VPC_FLOW_SMALL")
    if v is None or v == "":
        return SMALL_ROWS_DEFAULT
    try:
        return int(v)
    except ValueError:
        raise L.VpcError(f"VPC_FLOW_SMALL={v!r}: expected a number of stacked rows (0 keeps the launch chain)") from None


def small_step_route(R, d, hid, max_rows):
    """Whether FlowTrainer.step takes the small-batch step (the few-row layer ops of csrc/vpc_rows.hip): 0 < R <= max_rows
    stacked rows (small_max_rows()) and at most 128, every layer at most 1024 wide (the encoder input 2 d, hid_dim).
    Everything else keeps the launch chain."""
    return 0 < R <= min(max_rows, SMALL_MAX_ROWS) and 0 < 2 * d <= SMALL_MAX_WIDTH and 0 < hid <= SMALL_MAX_WIDTH


class FlowTrainer(_ChainTrainer):
    """The whole training step of the flow path (train.py:77-86 + :114-116) as a fixed sequence of HIP launches with no
    host synchronisation: mask_p draw + stacked encoder input + eps draws (one launch), the encoder GEMMs with the q and
    p passes stacked along the batch (one GEMM per layer), the flow, the five decoder GEMMs, the loss (two launches, the
    gradients gated through Sigmoid'), the backward GEMM chain with the flow backward between decoder and encoder, the
    eight weight gradients summed by one launch, flat Adam.  fp32 only; 30 launches.

    Few rows (small_step_route: R = P * B <= small_max_rows() and <= 128 stacked rows, layers at most 1024 wide) run the same
    step on the few-row layer ops (csrc/vpc_rows.hip): a forward launch per layer split over output features, and ONE
    backward launch per layer that writes the complete weight gradient next to the data gradient - no partials, no
    reduction launch: prep, 3 + 5 rows_fwd around the flow, the loss, 5 + 3 rows_bwd around the flow backward, Adam = 21 calls,
    22 launches, on the chain's workspace buffers and with the same draws.  VPC_FLOW_SMALL in the environment is the row
    limit and switches the path on (unset or 0 keeps the chain; SMALL_ROWS_MEASURED is the measured value); `last_path`
    names what the last step ran: "small" or "chain".

    Single process only: the reference's torch.any(inside) (VAE.py:1698) is a predicate over the whole batch of an
    encoder call, so a sharded step would need a cross-rank vote before the flow."""
    family, model_base, model_names = FAMILY, _FlowBase, "VAEFlow and REG_VAEFlow"
    single_process = ("the flow's torch.any(inside) is a predicate over the whole batch (no data-parallel form without a "
                      "cross-rank vote)")

    last_path = None

    def _wgrad_workspace(self, shapes, grads, sized=True):
        """The per-layer partials are the chain path's alone: allocated by its first step on this workspace
        (_chain_workspace), never for a trainer that only takes the small path, whose rows_bwd launches write the complete
        gradients `grads` (backward order: the decoder's last layer first, then the encoder's)."""
        self._wg_spec, self._wg = (shapes, grads), None
        n = len(self.dec_layers)
        self._dec_grads, self._enc_grads = grads[:n][::-1], grads[n:][::-1]

    def _chain_workspace(self):
        if self._wg is None:
            super()._wgrad_workspace(*self._wg_spec)

    def _buffers(self, B, e):
        m, dev = self.model, self.dev
        d, H = m.obs_dim, m.hid_dim
        P = 2 if self.reg else 1
        R = P * B
        self.xin, self.mask_p, self.eps = e(R, 2 * d), e(B, d), e(R, FLOW_L)
        self.h1, self.h2, self.t = e(R, H), e(R, H), e(R, CTX)
        self.z, self.zlp = e(R, FLOW_L), e(R, FLOW_L)
        self.gd = [e(R, H) for _ in range(4)]
        self.Y, self.G = e(R, d), e(R, d)
        self.gz, self.gzlp, self.dzd = e(R, FLOW_L), e(R, FLOW_L), e(R, FLOW_L)
        self.dgd = [e(R, H) for _ in range(4)]
        self.dt, self.dh2, self.dh1 = e(R, CTX), e(R, H), e(R, H)
        self.scratch = flow_loss_scratch(B, dev)
        pq = lambda a: (a[:B], a[B:] if self.reg else None)
        self._sl = dict(xm=pq(self.Y), z=pq(self.z), zlp=pq(self.zlp),
                        g=(*pq(self.G), *pq(self.gz), *pq(self.gzlp)))
        return (R, R, [self.xin, self.h1, self.h2, self.t], [None, self.dh1, self.dh2, self.dt],
                [self.z, *self.gd, self.Y], [self.dzd, *self.dgd, self.G])

    def train_step(self, x, mask, *, alpha, p_missingness, stage, **schedule):
        return self.step(x, mask, alpha=alpha, p_missingness=p_missingness, stage=stage)

    def step(self, x, mask, mask_p=None, eps=None, *, alpha=1.0, beta=1.0, p_missingness=30, stage="train"):
        """One optimiser step.  mask_p [B,d] (REG_VAEFlow) and eps [P,B,10] (the q pass, then the p pass) may be
        injected for parity tests; otherwise they are drawn on the device."""
        m = self.model
        v = m._views()
        d, H = m.obs_dim, m.hid_dim
        xf = _f32c(x.reshape(-1, d))
        L.require_cuda(xf)
        mf = _mask_f32(mask, d, xf.device)
        B = xf.shape[0]
        self._ws(B, v)
        reg = self.reg
        R = (2 if reg else 1) * B
        t, sl = self._timed, self._sl
        mp_in = _mask_f32(mask_p, d, xf.device) if (reg and mask_p is not None) else None
        mp = mp_in if mp_in is not None else (self.mask_p if reg else None)
        t("prep", flow_prep, xf, mf, mp_in, self.mask_p if (reg and mp_in is None) else None, self.xin,
          self.eps if eps is None else None, B, d, 1.0 - p_missingness / 100.0, self.seed, self.rng_offset,
          self.rng_offset + (1 << 40))
        if eps is not None:
            self.eps.copy_(eps.reshape(self.eps.shape))
        self.rng_offset += chain_draw_increment(self.eps.numel(), B, d)
        if small_step_route(R, d, H, small_max_rows()):
            return self._step_small(xf, mf, mp, R, B, d, alpha, beta, stage)
        self.last_path = "chain"
        self._chain_workspace()
        # ---- forward
        chain_fwd(self.enc_layers, self.enc_acts, R, 0, t, _T_ENC_FWD)
        t("flow", flow_fwd, self.t, self.eps, self.z, self.zlp, R, B)
        chain_fwd(self.dec_layers, self.dec_acts, R, 0, t, _T_DEC_FWD)
        # ---- loss: G = d train_loss / d decoder_mean pre-activation, gz / gzlp = d train_loss / d (z, z_log_prob)
        t("loss", flow_loss, xf, mf, mp, sl["xm"], sl["z"], sl["zlp"], sl["g"], self.scratch, self.out8, self.tail,
          self.accum, B, d, STAGE_TRAIN if stage == "train" else STAGE_EVAL, alpha, beta, 1.0 / B, 1)
        # ---- backward: weight-gradient partials per layer, all summed by one launch
        # (G already holds the gradient of decoder_mean's pre-activation: no gate pass over Y)
        chain_bwd(self.dec_layers, self.dec_acts, self.dec_dacts, R, self._wgrad, _DEC_WKEYS, run=t, names=_T_DEC_BWD)
        t("flow_bwd", flow_bwd, self.t, self.eps, self.dzd, self.gz, self.gzlp, self.dt, R, B)
        chain_bwd(self.enc_layers, self.enc_acts, self.enc_dacts, R, self._wgrad, _ENC_WKEYS, input_grad=False, run=t,
                  names=_T_ENC_BWD)
        self._wgrad_reduce()
        self._adam()

    def _step_small(self, xf, mf, mp, R, B, d, alpha, beta, stage):
        """The step behind the draws on the few-row layer ops, on the chain's workspace buffers: every rows_bwd writes its
        layer's complete weight gradient into the flat gradient, so Adam follows the last of them."""
        t, sl = self._timed, self._sl
        self.last_path = "small"
        chain_fwd_rows(self.enc_layers, self.enc_acts, R, t, _T_ENC_FWD)
        t("flow", flow_fwd, self.t, self.eps, self.z, self.zlp, R, B)
        chain_fwd_rows(self.dec_layers, self.dec_acts, R, t, _T_DEC_FWD)
        t("loss", flow_loss, xf, mf, mp, sl["xm"], sl["z"], sl["zlp"], sl["g"], self.scratch, self.out8, self.tail,
          self.accum, B, d, STAGE_TRAIN if stage == "train" else STAGE_EVAL, alpha, beta, 1.0 / B, 1)
        chain_bwd_rows(self.dec_layers, self.dec_acts, self.dec_dacts, R, self._dec_grads, run=t, names=_T_DEC_BWD)
        t("flow_bwd", flow_bwd, self.t, self.eps, self.dzd, self.gz, self.gzlp, self.dt, R, B)
        chain_bwd_rows(self.enc_layers, self.enc_acts, self.enc_dacts, R, self._enc_grads, input_grad=False, run=t,
                       names=_T_ENC_BWD)
        self._adam()


# ------------------------------------------------------------------------------------------------ batched evaluation
# Rows per chunk of FlowEvaluator's layer chain when the caller names none.  A MEMORY bound, not a measured optimum: a chunk row
# holds 6 hid_dim + 120 + obs_dim activation floats (two encoder and four decoder hidden layers, the contexts, z, z_log_prob,
# x_mean), 12.5 KB at hid_dim 500 and obs_dim 12, so a full chunk of 131 072 rows is 1.6 GB (a workspace is sized by its
# longest chunk, not by this bound).  What was measured (profiles/flow_eval_notes.md; 80 000 rows = M 50 x 1 600, d 12, hid 500):
# chunks of at most 8 192 / 32 768 / 65 536 / 131 072 rows took 3.47 / 2.42 / 2.27 / 2.18 ms - fewer chunks were never slower, so
# the bound is the largest of the four, under which that evaluation is one chunk; nothing above 80 000 rows was measured.
EVAL_MAX_ROWS = 1 << 17


def tile_tables(batches):
    """The tables of a batched evaluation from harness._gather_passes' ranges (M lists of (row_lo, row_hi) that follow each
    other without a gap, starting at row 0) -> (tile_row0 [n_tiles + 1], pass_tile0 [M + 1]) as lists: tile t = rows
    tile_row0[t] .. tile_row0[t + 1] - 1, pass p = tiles pass_tile0[p] .. pass_tile0[p + 1] - 1."""
    tile_row0, pass_tile0 = [0], [0]
    for ranges in batches:
        for lo, hi in ranges:
            if int(lo) != tile_row0[-1] or int(hi) <= int(lo):
                raise L.VpcError(f"batch ({lo}, {hi}) does not follow row {tile_row0[-1]}: the batches of all passes must "
                                 "lie behind each other, none of them empty")
            tile_row0.append(int(hi))
        if len(tile_row0) - 1 == pass_tile0[-1]:
            raise L.VpcError("a Monte-Carlo pass without a batch")
        pass_tile0.append(len(tile_row0) - 1)
    if len(pass_tile0) < 2:
        raise L.VpcError("no Monte-Carlo pass")
    return tile_row0, pass_tile0


def eval_chunks(tile_row0, max_rows):
    """Split the tiles into runs of at most max_rows rows, greedily and at tile boundaries only -> [(tile_lo, tile_hi)].  A
    single tile above max_rows raises: a batch is the unit of the flow's predicate and of the statistics."""
    out, lo = [], 0
    n = len(tile_row0) - 1
    for t in range(n):
        rows = tile_row0[t + 1] - tile_row0[t]
        if rows > max_rows:
            raise L.VpcError(f"tile {t} has {rows} rows, max_rows is {max_rows}: a chunk breaks only at tile boundaries")
        if tile_row0[t + 1] - tile_row0[lo] > max_rows:
            out.append((lo, t))
            lo = t
    return out + [(lo, n)]


class _EvalChunk:
    """One chunk's tiles [t0, t1) = stacked rows [r0, r1): its tile table counted from its own first row, host and device."""

    def __init__(self, tile_row0, t0, t1, dev):
        self.t0, self.t1, self.r0, self.r1 = t0, t1, tile_row0[t0], tile_row0[t1]
        self.rows = self.r1 - self.r0
        self.tab = _host_table(v - self.r0 for v in tile_row0[t0:t1 + 1])
        self.tab_dev = self.tab.to(dev)


class FlowEvaluator:
    """eval_vae's estimator for ONE VAEFlow / REG_VAEFlow model with every batch of every Monte-Carlo pass in one set of
    launches (csrc/vpc_floweval.hip): the rows of all batches stand behind each other, the eight layers
    run once over all of them, and a tile table keeps what is per batch per batch - the flow's torch.any(inside) (VAE.py:1698)
    and the statistics, whose means over a pass's batches and then over the passes are evaluate.py:232-245's.  One evaluate
    call that fits in one chunk is 12 library calls: prep, 3 encoder GEMMs, the flow, 5 decoder GEMMs, the tile statistics (2
    launches), the finalize - whatever M and the number of batches.

    What differs from eval_vae(engine="chain"): no p pass and no mask_p draw - the evaluate-stage loss of REG_VAEFlow is loss_q
    (VAE.py:2099-2104), which reads nothing of the p pass, and under Philox there is no stream position that the unused draws
    would have to preserve; eps comes from the evaluator's Philox stream (flow_eval_draw_counters), not from torch.randn.  The
    estimator and its distribution are the same.  The reference's drivers pass neither beta nor epoch into the flow losses
    (forward_loss): beta = 1.

    seed: of the Philox stream (None: 0); the evaluator owns an offset that every drawing call advances.  max_rows: rows per
    chunk of the layer chain (None: EVAL_MAX_ROWS).  tile_stats: the [n_tiles][8] table of the last call (vpc.h,
    vpc_flow_eval_tiles) and eps: the [R][10] normals it used, both valid until the next call on the same layout."""

    def __init__(self, model, seed=None, max_rows=None):
        if not isinstance(model, _FlowBase):
            raise L.VpcError(f"FlowEvaluator evaluates VAEFlow and REG_VAEFlow, not {type(model).__name__}")
        self.model = model
        self.seed = 0 if seed is None else int(seed)
        self.max_rows = EVAL_MAX_ROWS if max_rows is None else int(max_rows)
        if self.max_rows < 1:
            raise L.VpcError(f"max_rows = {max_rows}")
        self.rng_offset = 0
        self.tile_stats = self.eps = None
        self._layouts = {}

    def _layout(self, tile_row0, pass_tile0, dev):
        """The workspace of a layout, kept for the next call on it: tables, chunks, activation buffers, scratch, statistics."""
        key = (tuple(tile_row0), tuple(pass_tile0), str(dev))
        ws = self._layouts.get(key)
        if ws is not None:
            return ws
        m = self.model
        d, H = m.obs_dim, m.hid_dim
        R, n_tiles = tile_row0[-1], len(tile_row0) - 1
        ws = self._layouts[key] = {}
        chunks = ws["chunks"] = [_EvalChunk(tile_row0, t0, t1, dev) for t0, t1 in eval_chunks(tile_row0, self.max_rows)]
        C = max(c.rows for c in chunks)
        e = lambda *s: torch.empty(*s, device=dev)
        ws["ptab"] = _host_table(pass_tile0)
        ws["ptab_dev"] = ws["ptab"].to(dev)
        ws["xin"], ws["eps"] = e(R, 2 * d), e(R, FLOW_L)
        ws["enc"] = [None, e(C, H), e(C, H), e(C, CTX)]
        ws["dec"] = [e(C, FLOW_L), *[e(C, H) for _ in range(4)], e(C, d)]
        ws["zlp"] = e(C, FLOW_L)
        ws["scratch"] = flow_eval_tiles_scratch(max(tile_row0[t + 1] - tile_row0[t] for t in range(n_tiles)), n_tiles, dev)
        ws["stats"] = torch.zeros(n_tiles, 8, dtype=torch.float64, device=dev)
        ws["out4"] = torch.empty(4, dtype=torch.float64, device=dev)
        return ws

    def evaluate(self, x, mask, batches, eps=None):
        """x, mask: [R, d], the batches of all passes behind each other (harness._gather_passes); batches: M lists of
        (row_lo, row_hi).  eps: [R, 10] normals, or None: drawn on the device at the next flow_eval_draw_counters offset.
        Returns a float64 tensor [4] on the device = (rmse on ~mask, elbo, negll, negll_imp) as eval_vae averages them; no host
        synchronisation."""
        m = self.model
        d = m.obs_dim
        xf = _f32c(x.reshape(-1, d))
        L.require_cuda(xf)
        dev = xf.device
        mf = _mask_f32(mask, d, dev)
        tile_row0, pass_tile0 = tile_tables(batches)
        R, n_tiles = tile_row0[-1], len(tile_row0) - 1
        if xf.shape[0] != R or mf.shape[0] != R:
            raise L.VpcError(f"x has {xf.shape[0]} rows and mask {mf.shape[0]}, the batches cover {R}")
        ws = self._layout(tile_row0, pass_tile0, dev)
        if eps is None:
            off, self.rng_offset = flow_eval_draw_counters(self.rng_offset, R)
            flow_prep(xf, mf, None, None, ws["xin"], ws["eps"], R, d, 1.0, self.seed, 0, off)
            ef = ws["eps"]
        else:
            ef = _f32c(eps.reshape(-1, FLOW_L).to(dev))
            if ef.shape[0] != R:
                raise L.VpcError(f"eps has {ef.shape[0]} rows, the batches cover {R}")
            flow_prep(xf, mf, None, None, ws["xin"], None, R, d)
        enc, dec = m._build_chains(m._views())
        ea, da, zlp, stats = ws["enc"], ws["dec"], ws["zlp"], ws["stats"]
        for c in ws["chunks"]:
            n = c.rows
            ea[0] = ws["xin"][c.r0:c.r1]
            chain_fwd(enc, ea, n)
            flow_fwd_tiles(ea[3], ef[c.r0:c.r1], da[0], zlp, n, c.tab, c.tab_dev)
            chain_fwd(dec, da, n)
            flow_eval_tiles(xf[c.r0:c.r1], mf[c.r0:c.r1], da[5], da[0], zlp, n, d, c.tab, c.tab_dev, 1.0, ws["scratch"],
                            stats[c.t0:c.t1])
        flow_eval_finalize(stats, n_tiles, ws["ptab"], ws["ptab_dev"], ws["out4"])
        self.tile_stats, self.eps = stats, ef
        return ws["out4"].clone()
