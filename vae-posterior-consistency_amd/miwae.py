"""MIWAE path (Data/imputation_args.json runs reg_MIWAE* / vanilla_MIWAE*): drop-in classes for the reference's

    MIWAE       src/models/VAE.py:3011-3134
    Reg_MIWAE   src/models/VAE.py:3137-3301

with the same constructor arguments, `encoder` / `decoder` / `forward` / `loss` signatures, return order and state_dict
keys (seq_encoder.{0,2,4}, seq_decoder.{0,2,4}).  The six layers run as fp32 MFMA GEMMs (csrc/vpc_gemm.hip, ReLU
between layers); the softplus sampler, the Student-t decoder heads and the importance-weighted bound with all of its
gradients are csrc/vpc_miw.hip.  All twelve trainable tensors are views of one flat fp32 buffer.  No CPU fallback: CPU
tensors raise.

The reference's row / sample mix-up is reproduced, not fixed.  `logpxobsgivenz` is built in (row, sample) order and
reshaped to [S, B] (VAE.py:3078-3081, :3209-3212, :3230-3233), while `logpz - logq` is [B, S].permute(1, 0)
(:3089-3090, :3218-3219, :3239-3240).  For B > 1 and S > 1, slot (i, j) of the bound therefore pairs the likelihood of
data row (i*B + j) // S, sample (i*B + j) % S with the prior / posterior terms of row j, sample i; the loss, its gradients
and the llh_eval weights (applied to the un-mixed x_mean, :3096-3098 / :3267-3269) are those of this pairing.  With
B == 1 (eval_miwae, one row per call) the pairing is the natural one, and the batched eval_miwae uses the per-row pairing
(VPC_MIW_PAIR_PER_ROW), which equals N single-row calls.

What this family shares with notmiwae.py and flow.py lives in chainfamily.py: the encoder / decoder autograd frame (driven
by FAMILY below), the trainer frame and the host side of impute_stream.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _lib as L
from . import chainfamily as cf
from ._lib import check, lib, ptr, require_cuda, stream_ptr
from .chainfamily import STREAM_MAX_L, ChainDecoderFn, ChainEncoderFn, Family, _ChainTrainer, _joined, _ReferenceAttrs, nm_mul
from .chainfamily import impute_chunk, impute_draws, miw_impute_draws  # noqa: F401  (defined in chainfamily.py only; the names
# stay importable from here)
from .images import FlatParams, mlp_spec
from .linear import ACT_NONE, ACT_RELU, _f32c, chain, chain_bwd, chain_fwd
from .trainer import chain_draw_increment

HID = 128  # VAE.py:3027-3042 / :3153-3168 hard-code 128 (hid_dim is ignored by the reference too)
PAIR_REFERENCE, PAIR_PER_ROW = 0, 1


# ------------------------------------------------------------------------------------------------ raw ops
def miw_sample(heads, hact, eps, z, R, S, Ld):
    check(lib().vpc_miw_sample(ptr(heads), ptr(hact), ptr(eps), ptr(z), int(R), int(S), int(Ld), stream_ptr()),
          "vpc_miw_sample")


def miw_sample_bwd(dz, eps, heads, g_hact, out, R, S, Ld):
    check(lib().vpc_miw_sample_bwd(ptr(dz), ptr(eps), ptr(heads), ptr(g_hact), ptr(out), int(R), int(S), int(Ld),
                                   stream_ptr()), "vpc_miw_sample_bwd")


def miw_heads(y_raw, y_act, M, d):
    check(lib().vpc_miw_heads(ptr(y_raw), ptr(y_act), int(M), int(d), stream_ptr()), "vpc_miw_heads")


def miw_heads_bwd(y_raw, g_act, g_raw, M, d):
    check(lib().vpc_miw_heads_bwd(ptr(y_raw), ptr(g_act), ptr(g_raw), int(M), int(d), stream_ptr()), "vpc_miw_heads_bwd")


def miw_loss_scratch(B, S, device):
    nbytes = int(lib().vpc_miw_loss_scratch(int(B), int(S)))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def miw_loss(x, mask, mask_p, y_q, y_p, ldy, raw, hq, hp, eq, ep, g_q, g_p, ldg, ghq, ghp, xm_imp, scratch, out8,
             loss_f32, accum, B, S, d, Ld, alpha, pairing=PAIR_REFERENCE):
    check(lib().vpc_miw_loss(ptr(x), ptr(mask), ptr(mask_p), ptr(y_q), ptr(y_p), int(ldy), int(raw), ptr(hq), ptr(hp),
                             ptr(eq), ptr(ep), ptr(g_q), ptr(g_p), int(ldg), ptr(ghq), ptr(ghp), ptr(xm_imp),
                             ptr(scratch), scratch.numel() * scratch.element_size(), ptr(out8), ptr(loss_f32),
                             ptr(accum), int(B), int(S), int(d), int(Ld), float(alpha), int(pairing), stream_ptr()),
          "vpc_miw_loss")


def miw_small_workspace(d, Ld):
    """Floats of the partial buffer of the small-batch step (0: the shape is outside its limits)."""
    return int(lib().vpc_miw_small_workspace(int(d), int(Ld)))


def miw_small_fwd(flat, xin, eps, h1, h2, heads, hact, z, g1, g2, Y, R, S, d, Ld, RB):
    check(lib().vpc_miw_small_fwd(ptr(flat), ptr(xin), ptr(eps), ptr(h1), ptr(h2), ptr(heads), ptr(hact), ptr(z), ptr(g1),
                                  ptr(g2), ptr(Y), int(R), int(S), int(d), int(Ld), int(RB), stream_ptr()),
          "vpc_miw_small_fwd")


def miw_small_bwd(flat, xin, eps, h1, h2, heads, z, g1, g2, G, gh, dht, part, R, S, d, Ld, RB):
    check(lib().vpc_miw_small_bwd(ptr(flat), ptr(xin), ptr(eps), ptr(h1), ptr(h2), ptr(heads), ptr(z), ptr(g1), ptr(g2),
                                  ptr(G), ptr(gh), ptr(dht), ptr(part), part.numel(), int(R), int(S), int(d), int(Ld),
                                  int(RB), stream_ptr()), "vpc_miw_small_bwd")


def miw_small_tail(part, R, RB, d, Ld, grad, flat, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
    check(lib().vpc_miw_small_tail(ptr(part), part.numel(), int(R), int(RB), int(d), int(Ld), ptr(grad), ptr(flat),
                                   ptr(exp_avg), ptr(exp_avg_sq), lr, beta1, beta2, eps, int(step), stream_ptr()),
          "vpc_miw_small_tail")


def miw_impute_scratch(B, S, d, Ld, s_chunk):
    """Floats of the partial buffer of the streaming imputation, B * ceil(S / s_chunk16) * (2 + d) with s_chunk16 =
    s_chunk rounded up to a multiple of 16 (0: the shape is outside the limits)."""
    return int(lib().vpc_miw_impute_scratch(int(B), int(S), int(d), int(Ld), int(s_chunk)))


def miw_impute(flat, x, mask, eps, seed, offset, row0, part, xm, lse, B, S, d, Ld, s_chunk):
    check(lib().vpc_miw_impute(ptr(flat), ptr(x), ptr(mask), ptr(eps), int(seed), int(offset), int(row0), ptr(part),
                               part.numel(), ptr(xm), ptr(lse), int(B), int(S), int(d), int(Ld), int(s_chunk),
                               stream_ptr()), "vpc_miw_impute")


# ------------------------------------------------------------------------------------------------ autograd
_ENC_NAMES = ("We1", "be1", "We2", "be2", "Wh", "bh")
_DEC_NAMES = ("Wd1", "bd1", "Wd2", "bd2", "Wx", "bx")


def _chains(v):
    """(encoder, decoder) chains on the named views v: ReLU between layers, raw heads."""
    return (chain([v[k] for k in _ENC_NAMES], (ACT_RELU, ACT_RELU, ACT_NONE)),
            chain([v[k] for k in _DEC_NAMES], (ACT_RELU, ACT_RELU, ACT_NONE)))


def _sample(heads, eps, B, S, Ld):
    """-> (z [B,S,L], hact [B, mean L | scale L]).  VAE.py:3059-3070 / :3188-3200."""
    hact, z = torch.empty(B, 2 * Ld, device=heads.device), torch.empty(B * S, Ld, device=heads.device)
    miw_sample(heads, hact, eps, z, B, S, Ld)
    return z.view(B, S, Ld), hact


def _heads_fwd(y_raw, M, d):
    Ya = torch.empty(M, 3 * d, device=y_raw.device)
    miw_heads(y_raw, Ya, M, d)
    return Ya


# the decoder returns (mean, scale, df) as the three column blocks of ONE activated [M, 3d] buffer (VAE.py:3072-3076)
FAMILY = Family(_ENC_NAMES, _DEC_NAMES, lambda x, mask, out, B, d: nm_mul(x, mask, out), _sample,
                lambda heads, eps, dz, dhact, out, B, S, Ld: miw_sample_bwd(dz, eps, heads, dhact, out, B, S, Ld), 3,
                (_heads_fwd, miw_heads_bwd))


class MIWLossFn(torch.autograd.Function):
    """The bound on activated heads + every gradient (vpc_miw_loss, raw = 0).  Returns (loss fp32, out8, xm_imp)."""

    @staticmethod
    def forward(ctx, cfg, x, mask, mask_p, Yq, hq, eq, Yp, hp, ep):
        reg = mask_p is not None
        require_cuda(x, mask, mask_p, Yq, hq, eq, Yp, hp, ep)
        B, S, d, Ld = cfg["B"], cfg["S"], cfg["d"], cfg["L"]
        dev = x.device
        need_grad = cfg["grad"] and any(ctx.needs_input_grad)
        Gq = Gp = ghq = ghp = None
        if need_grad:
            Gq, ghq = torch.empty(B * S, 3 * d, device=dev), torch.empty(B, 2 * Ld, device=dev)
            if reg:
                Gp, ghp = torch.empty(B * S, 3 * d, device=dev), torch.empty(B, 2 * Ld, device=dev)
        xm_imp = torch.empty(B, d, device=dev) if cfg["impute"] else None
        out8 = torch.empty(8, dtype=torch.float64, device=dev)
        miw_loss(x, mask, mask_p, Yq, Yp, 3 * d, 0, hq, hp, eq, ep, Gq, Gp, 3 * d, ghq, ghp, xm_imp,
                 miw_loss_scratch(B, S, dev), out8, None, None, B, S, d, Ld, cfg["alpha"], cfg["pairing"])
        ctx.reg, ctx.need_grad = reg, need_grad
        if need_grad:
            ctx.save_for_backward(*[t for t in (Gq, ghq, Gp, ghp) if t is not None])
        imp = xm_imp if xm_imp is not None else torch.empty(0, device=dev)
        ctx.mark_non_differentiable(out8, imp)
        return out8[0].float(), out8, imp

    @staticmethod
    def backward(ctx, gloss, _g8, _gi):
        if not ctx.need_grad:
            return (None,) * 10
        t = [u * gloss for u in ctx.saved_tensors]
        if ctx.reg:
            return None, None, None, None, t[0], t[1], None, t[2], t[3], None
        return None, None, None, None, t[0], t[1], None, None, None, None


# ------------------------------------------------------------------------------------------------ model classes
class _MIWBase(_ReferenceAttrs, FlatParams, nn.Module):
    regularised = False
    # flat parameter buffer: [We1 be1 We2 be2 Wh bh | Wd1 bd1 Wd2 bd2 Wx bx] = state_dict order
    _flat_spec = mlp_spec(_ENC_NAMES, "seq_encoder", "enc") + mlp_spec(_DEC_NAMES, "seq_decoder", "dec")
    _build_chains = staticmethod(_chains)

    def __init__(self, obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates):
        super().__init__()
        self._init_reference_attrs("MIWAE", obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates)
        d, Ld = obs_dim, latent_dim
        # created in the reference's order (same seed -> same initial weights)
        self.seq_encoder = nn.Sequential(nn.Linear(d, HID), nn.ReLU(), nn.Linear(HID, HID), nn.ReLU(),
                                         nn.Linear(HID, 2 * Ld))
        self.seq_decoder = nn.Sequential(nn.Linear(Ld, HID), nn.ReLU(), nn.Linear(HID, HID), nn.ReLU(),
                                         nn.Linear(HID, 3 * d))
        self.max_epoch = 2800
        self._flat = None
        self.last_impute_engine = None  # "chain" / "stream": what the last impute() ran

    @property
    def prior(self):  # VAE.py:3047 (a CPU distribution in the reference; kept for attribute parity)
        return torch.distributions.Normal(torch.zeros(self.latent_dim), torch.ones(self.latent_dim))

    # ---- reference API
    def _encode(self, x, mask, sample=True, eps=None, S=None):
        L.require_cuda(x)
        d, Ld = self.obs_dim, self.latent_dim
        S = self.num_samples if S is None else S
        xf = _f32c(x.reshape(-1, d))
        mf = _f32c(mask.reshape(-1, d).to(xf.device))
        B = xf.shape[0]
        if sample and eps is None:
            eps = torch.randn(B, S, Ld, device=xf.device)  # Normal(mean, scale).rsample()
        z, hact = ChainEncoderFn.apply(FAMILY, self, xf, mf, _f32c(eps) if sample else None, S, *self._enc_weights())
        mean = hact[:, :Ld].unsqueeze(1).expand(B, S, Ld)
        scale = hact[:, Ld:].unsqueeze(1).expand(B, S, Ld)
        mean._vpc_hact = hact
        scale._vpc_hact = hact
        return z, mean, scale

    def encoder(self, x, mask, sample=True):
        """VAE.py:3049-3070 / :3178-3200 -> (z, mean, scale), each [B, num_samples, latent_dim]."""
        return self._encode(x, mask, sample)

    def decoder(self, z_int):
        """VAE.py:3072-3076 / :3202-3206 -> (mean, scale, deg_free)."""
        L.require_cuda(z_int)
        return ChainDecoderFn.apply(FAMILY, self, z_int, *self._dec_weights())

    @staticmethod
    def _hact_of(mean, scale):
        h = getattr(mean, "_vpc_hact", None)
        if h is not None and h is getattr(scale, "_vpc_hact", None):
            return h
        return torch.cat([mean[:, 0, :], scale[:, 0, :]], 1)  # any [B,S,L] pair replicated over S

    def _heads_Y(self, xm, xs, df, M):
        d = self.obs_dim
        # the decoder's three outputs are column blocks of one buffer: without autograd, pass that buffer itself (an
        # as_strided view under autograd would route the whole gradient to the first output)
        Y = None if torch.is_grad_enabled() else _joined((xm, xs, df), M, d)
        return Y if Y is not None else torch.cat([_f32c(t).reshape(M, d) for t in (xm, xs, df)], 1)

    def _loss(self, x, mask, mask_p, outs_q, outs_p, alpha, eps, llh_eval, pairing=PAIR_REFERENCE, S=None):
        d, Ld = self.obs_dim, self.latent_dim
        S = self.num_samples if S is None else S
        xf = _f32c(x.reshape(-1, d))
        B = xf.shape[0]
        if eps is None:  # the fresh rsample() of loss(): q pass, then p pass (VAE.py:3216, :3237)
            eps = [torch.randn(B, S, Ld, device=xf.device) for _ in range(1 if mask_p is None else 2)]
        cfg = dict(B=B, S=S, d=d, L=Ld, alpha=alpha, grad=torch.is_grad_enabled(), impute=bool(llh_eval),
                   pairing=pairing)
        mf = _f32c(mask.reshape(-1, d).to(xf.device))
        xm, xs, df, mean, scale = outs_q
        Yq, hq = self._heads_Y(xm, xs, df, B * S), self._hact_of(mean, scale)
        Yp = hp = mpf = ep = None
        if outs_p is not None:
            xm, xs, df, mean, scale = outs_p
            Yp, hp = self._heads_Y(xm, xs, df, B * S), self._hact_of(mean, scale)
            mpf = _f32c(mask_p.reshape(-1, d).to(xf.device))
            ep = _f32c(eps[1])
        return MIWLossFn.apply(cfg, xf, mf, mpf, Yq, hq, _f32c(eps[0]), Yp, hp, ep)

    def forward_loss(self, x, mask, mask_p=None, *, epoch=1, alpha=1.0, beta=1.0, beta_annealing=False, alpha_annealing=True,
                     stage="train", llh_eval=False):
        """forward, then loss, wired as the reference's drivers wire them.  With llh_eval the
        imputation is loss's first return (evaluate.py:97-112): no X_MEAN_Q here."""
        if self.regularised:  # train.py:53-55, 102-108
            o = self.forward(x, mask, mask_p)
            return o, self.loss(x, o[2], o[3], o[4], o[0], o[1], o[7], o[8], o[9], o[5], o[6], mask, mask_p, epoch,
                                llh_eval=llh_eval, beta_annealing=beta_annealing, beta=beta, alpha=alpha)
        o = self.forward(x, mask)  # train.py:109-113 (evaluate.py:108-112 adds beta_annealing / beta, which MIWAE.loss ignores)
        return o, self.loss(x, o[2], o[3], o[4], o[0], o[1], mask, epoch, llh_eval=llh_eval)

    @torch.no_grad()
    def impute(self, x, mask, mask_p=None, num_samples=None, pairing=PAIR_PER_ROW, engine="chain", **stream_args):
        """llh_eval imputation of every row of x with num_samples draws, rows independent (per-row pairing): what
        eval_miwae computes one row at a time (evaluate.py:89-111), for a whole chunk of rows in one launch sequence.
        engine="stream" forwards to impute_stream (two launches, no decoder row in memory; mask_p is not read, the
        per-row pairing is the only one, stream_args = its eps / seed / offset / row0 / s_chunk / return_lse).
        `last_impute_engine` names what the last call ran."""
        if engine == "stream":
            if pairing != PAIR_PER_ROW:
                raise L.VpcError("engine='stream' imputes with the per-row pairing only")
            self.last_impute_engine = "stream"
            return impute_stream(self, x, mask, num_samples=num_samples, **stream_args)
        if engine != "chain" or stream_args:
            raise L.VpcError(f"impute: engine {engine!r} with {sorted(stream_args)} (engines: 'chain', 'stream'; eps / seed / "
                             "offset / row0 / s_chunk / return_lse belong to 'stream')")
        self.last_impute_engine = "chain"
        S = self.num_samples if num_samples is None else num_samples
        z_q, mean_q, scale_q = self._encode(x, mask, S=S)
        outs_q = (*self.decoder(z_q), mean_q, scale_q)
        outs_p = None
        if self.regularised:
            z_p, mean_p, scale_p = self._encode(x, mask_p, S=S)
            outs_p = (*self.decoder(z_p), mean_p, scale_p)
        _, _, xm = self._loss(x, mask, mask_p if self.regularised else None, outs_q, outs_p, 0.5, None, True, pairing, S)
        return xm


class MIWAE(_MIWBase):
    """MIWAE with a Student-t decoder.  Reference: src/models/VAE.py:3011-3134."""

    def forward(self, data, mask):
        z, mean, scale = self.encoder(data, mask)
        x_mean, x_scale, deg_free = self.decoder(z)
        return mean, scale, x_mean, x_scale, deg_free

    def loss(self, x, x_mean, x_scale, deg_free, mean, scale, mask, epoch, vae_elbo=False, llh_eval=False, MI=False,
             beta_annealing=True, beta=1.0, stage="train", eps=None):
        """VAE.py:3078-3114; draws the fresh z of :3087 on the device unless eps [B,S,L] is given."""
        if MI:
            raise NotImplementedError("the MI branch of the reference reads undefined names (VAE.py:3101-3106)")
        loss, out8, xm = self._loss(x, mask, None, (x_mean, x_scale, deg_free, mean, scale), None, 0.0,
                                    None if eps is None else [eps], llh_eval)
        if llh_eval:  # VAE.py:3095-3099
            return xm, loss, out8[5].float()
        return loss, loss  # (print_loss, train_loss)


class Reg_MIWAE(_MIWBase):
    """Posterior-consistency regularised MIWAE.  Reference: src/models/VAE.py:3137-3301."""
    regularised = True

    def forward(self, data, mask, mask_p, stage="train"):
        # VAE.py:3295-3301: q pass first (RNG order), p outputs returned first
        z_q, mean_q, scale_q = self.encoder(data, mask)
        x_mean_q, x_scale_q, deg_free_q = self.decoder(z_q)
        z_p, mean_p, scale_p = self.encoder(data, mask_p)
        x_mean_p, x_scale_p, deg_free_p = self.decoder(z_p)
        return mean_p, scale_p, x_mean_p, x_scale_p, deg_free_p, mean_q, scale_q, x_mean_q, x_scale_q, deg_free_q

    def loss(self, x, x_mean_p, x_scale_p, deg_free_p, mean_p, scale_p, x_mean_q, x_scale_q, deg_free_q, mean_q,
             scale_q, mask, mask_p, epoch, vae_elbo=False, llh_eval=False, MI=False, beta_annealing=True, beta=1.0,
             alpha=1.0, stage="train", eps=None):
        """VAE.py:3208-3265; eps = (eps_q, eps_p) [B,S,L] for the two fresh draws of :3216 / :3237 (device draws
        otherwise).  loss = nb_q + alpha * (KL_reg - nb_q + nb_p - reg_like)."""
        if MI:
            raise NotImplementedError("the MI branch of the reference reads undefined names (VAE.py:3271-3276)")
        loss, out8, xm = self._loss(x, mask, mask_p, (x_mean_q, x_scale_q, deg_free_q, mean_q, scale_q),
                                    (x_mean_p, x_scale_p, deg_free_p, mean_p, scale_p), alpha, eps, llh_eval)
        if llh_eval:  # VAE.py:3266-3270
            return xm, loss, loss
        return loss, loss


# ------------------------------------------------------------------------------------------------ streaming imputation
def impute_stream(model, x, mask, num_samples=None, eps=None, seed=None, offset=0, row0=0, s_chunk=None,
                  return_lse=False):
    """The llh_eval imputation of every row of x with num_samples draws (evaluate.py:89-113 through VAE.py:3078-3099 /
    :3204-3258, per-row pairing) in two launches: csrc/vpc_miw_impute.hip runs encoder, sampler, decoder, log-weights and
    an online softmax per (row, chunk of s_chunk samples) and never writes a decoder row; the merge combines a row's
    chunks in chunk order.  Returns xm [B, d], or (xm, lse [B]) with return_lse: lse = the per-row log-sum-exp of the
    log-weights, the IW bound before the mean.

    mask_p is not an argument, for Reg_MIWAE too: the reference's imputation takes the q pass's weights and the q pass's
    x_mean only (VAE.py:3255-3257, MIWAE :3095-3098), so the whole p pass - which evaluate.py:99-104 computes and drops
    with the loss - is skipped.

    eps [2, B, S, L] injects the sampler's draw and the fresh draw of :3087 / :3216; otherwise both are drawn in the
    kernel from (seed, offset, row0) - seed None takes one from torch's generator - by the rule of
    trainer.impute_draw_counter, which does not depend on s_chunk: impute_draws returns those values, and rows [a, b) of
    a call equal the call on x[a:b] with row0 = a.  s_chunk None: impute_chunk.  For a given s_chunk the result is
    bit-reproducible.  obs_dim <= 32, latent_dim <= 16; anything else, CPU tensors, a wrong eps shape or s_chunk < 1
    raise VpcError (no fallback)."""
    return cf.impute_stream(model, x, mask, num_samples, eps, seed, offset, row0, s_chunk, return_lse, SMALL_MAX_D,
                            SMALL_MAX_L, miw_impute_scratch, miw_impute)


# ------------------------------------------------------------------------------------------------ fused step
# timer names of the chain launches, per layer, and the weight gradients' (timer name, index in the trainer's workspace)
_T_ENC_FWD, _T_ENC_BWD, _T_DEC_FWD, _T_DEC_BWD = ("enc_fwd",) * 3, ("enc_bwd",) * 3, ("dec_fwd",) * 3, ("dec_bwd",) * 3
_DEC_WKEYS = (("dec_bwd", 2), ("dec_bwd", 1), ("dec_bwd", 0))
_ENC_WKEYS = (("enc_bwd", 5), ("enc_bwd", 4), ("enc_bwd", 3))


SMALL_MAX_D, SMALL_MAX_L = 32, STREAM_MAX_L  # limits of csrc/vpc_miw_small.hip and csrc/vpc_miw_impute.hip
# The row limit of the small-batch step, in decoder rows P * B * S.  The step without VPC_MIW_SMALL in the environment stays the
# launch chain (tests/test_trainer_images.py pins the chain's launch sequence as MIWTrainer's step at the wine shape), so the
# default is 0; SMALL_ROWS_MEASURED is the largest size at which the small path's worst block beat the chain's best block
# (profiles/miw_small_notes.md) - the value to put into VPC_MIW_SMALL.
SMALL_ROWS_DEFAULT = 0
SMALL_ROWS_MEASURED = 163840


def small_max_rows():
    """The row limit of the small-batch step: VPC_MIW_SMALL in the environment (decoder rows P * B * S; 0 = never), read
    per step; SMALL_ROWS_DEFAULT (0: the chain) without it."""
    v = os.environ.get("VPC_MIW_SMALL")
    if v is None or v == "":
        return SMALL_ROWS_DEFAULT
    try:
        return int(v)
    except ValueError:
        raise L.VpcError(f"VPC_MIW_SMALL={v!r}: expected a number of decoder rows (0 keeps the launch chain)") from None


def small_step_route(d, L, B, S, P, max_rows):
    """Whether MIWTrainer.step takes the small-batch step (csrc/vpc_miw_small.hip): obs_dim <= 32, latent_dim <= 16 and
    0 < P * B * S <= max_rows decoder rows (small_max_rows()).  Everything else keeps the launch chain."""
    return 0 < d <= SMALL_MAX_D and 0 < L <= SMALL_MAX_L and S >= 1 and 0 < P * B * S <= max_rows


def small_rows_per_workgroup(R, S):
    """RB, the data rows of the stacked passes one workgroup of the small-batch step owns: the smallest of 1, 2, 4 that
    leaves at most one workgroup per CU (the grid of the backward kernel: vpc_miw_small_workspace / n_params blocks; 256 on
    an MI355X), 4 beyond.  Measured at S = 20 only (profiles/miw_small_notes.md): S does not enter the rule."""
    cus = L.max_blocks() // 2
    return 1 if R <= cus else 2 if R <= 2 * cus else 4


class MIWTrainer(_ChainTrainer):
    """The whole training step of the MIWAE path (train.py:102-117 for 'reg_MIWAE*' / the final branch for
    'vanilla_MIWAE*') as a fixed sequence of HIP launches with no host synchronisation: mask_p draw + stacked encoder
    input + Philox normals (one launch), the encoder and decoder GEMM chains with the q and p passes stacked along the
    batch (one GEMM per layer), the three loss launches on the raw decoder heads, the backward GEMM chain into one flat
    gradient, flat Adam.  fp32 only.

    Small shapes (small_step_route: obs_dim <= 32, latent_dim <= 16, P * B * S <= small_max_rows() decoder rows) run the two
    GEMM chains, the sampler and their backward passes as two kernels and close with one tail (csrc/vpc_miw_small.hip):
    prep -> miw_small_fwd -> the three loss launches -> miw_small_bwd -> miw_small_tail (partial blocks summed in a fixed
    order, flat Adam), seven launches of this library instead of 25, on the same workspace buffers and with the same draws.  VPC_MIW_SMALL
    in the environment is the row limit and switches the path on (unset or 0 keeps the chain; SMALL_ROWS_MEASURED is the
    measured value); `last_path` names what the last step ran: "small" or "chain".

    Single process only: the reference's row / sample pairing (module docstring) couples rows across the whole batch, so
    a step sharded over ranks cannot equal the single-process step without an all-gather of the per-row sums."""
    family, model_base, model_names = FAMILY, _MIWBase, "MIWAE and Reg_MIWAE"
    single_process = ("the reference's row/sample pairing couples rows across the global batch (no data-parallel form "
                      "without an all-gather)")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, process_group=None, world_size=1, rank=0):
        super().__init__(model, lr, betas, eps, seed, process_group, world_size, rank)
        self._part = None  # partial blocks of the small-batch step: made on its first use
        self.small_rb = None  # rows per workgroup of the small-batch step; None: small_rows_per_workgroup
        self.last_path = None

    def _buffers(self, B, e):
        m = self.model
        d, Ld, S = m.obs_dim, m.latent_dim, m.num_samples
        P = 2 if self.reg else 1
        R, M = P * B, P * B * S
        self.xin, self.mask_p = e(R, d), e(B, d)
        self.h1, self.h2, self.heads, self.hact = e(R, HID), e(R, HID), e(R, 2 * Ld), e(R, 2 * Ld)
        self.eps = e(2 * P, B, S, Ld)  # sampling draws of the P passes, then the loss-time draws
        self.z, self.g1, self.g2, self.Y = e(M, Ld), e(M, HID), e(M, HID), e(M, 3 * d)
        self.G, self.gh, self.dht = e(M, 3 * d), e(R, 2 * Ld), e(R, 2 * Ld)
        self.dg2, self.dg1, self.dz, self.dh2, self.dh1 = e(M, HID), e(M, HID), e(M, Ld), e(R, HID), e(R, HID)
        self.scratch = miw_loss_scratch(B, S, self.dev)
        BS = B * S
        self._sl = dict(Yp=self.Y[BS:] if self.reg else None, Gp=self.G[BS:] if self.reg else None,
                        hp=self.hact[B:] if self.reg else None, ghp=self.gh[B:] if self.reg else None,
                        eq=self.eps[P], ep=self.eps[P + 1] if self.reg else None, es=self.eps[:P])
        return (R, M, [self.xin, self.h1, self.h2, self.heads], [None, self.dh1, self.dh2, self.dht],
                [self.z, self.g1, self.g2, self.Y], [self.dz, self.dg1, self.dg2, self.G])

    def step(self, x, mask, mask_p=None, eps=None, *, alpha=1.0, p_missingness=30):
        """One optimiser step.  mask_p [B,d] and eps ([4,B,S,L] = forward q, forward p, loss q, loss p for Reg_MIWAE;
        [2,B,S,L] = forward, loss for MIWAE) may be injected for parity tests; otherwise they are drawn on the device."""
        m = self.model
        v = m._views()
        d, Ld, S = m.obs_dim, m.latent_dim, m.num_samples
        xf, mf = _f32c(x.reshape(-1, d)), _f32c(mask.reshape(-1, d))
        L.require_cuda(xf, mf)
        B = xf.shape[0]
        self._ws(B, v)
        reg = self.reg
        P = 2 if reg else 1
        R, M = P * B, P * B * S
        t, sl = self._timed, self._sl
        mp = self._draw_inputs(xf, mf, mask_p, eps, B, d, p_missingness, chain_draw_increment(self.eps.numel(), B, d))
        if small_step_route(d, Ld, B, S, P, small_max_rows()):
            return self._step_small(xf, mf, mp, R, S, d, Ld, alpha)
        self.last_path = "chain"
        # ---- forward
        chain_fwd(self.enc_layers, self.enc_acts, R, 0, t, _T_ENC_FWD)
        t("sample", miw_sample, self.heads, self.hact, sl["es"], self.z, R, S, Ld)
        chain_fwd(self.dec_layers, self.dec_acts, M, 0, t, _T_DEC_FWD)
        # ---- loss on the raw heads: G = d loss / d raw decoder heads, gh = d loss / d (mean | scale)
        t("loss", miw_loss, xf, mf, mp, self.Y, sl["Yp"], 3 * d, 1, self.hact, sl["hp"], sl["eq"], sl["ep"], self.G,
          sl["Gp"], 3 * d, self.gh, sl["ghp"], None, self.scratch, self.out8, self.tail, self.accum, B, S, d, Ld, alpha,
          PAIR_REFERENCE)
        # ---- backward: weight-gradient partials per layer, all summed by one launch
        chain_bwd(self.dec_layers, self.dec_acts, self.dec_dacts, M, self._wgrad, _DEC_WKEYS, run=t, names=_T_DEC_BWD)
        t("sample_bwd", miw_sample_bwd, self.dz, sl["es"], self.heads, self.gh, self.dht, R, S, Ld)
        chain_bwd(self.enc_layers, self.enc_acts, self.enc_dacts, R, self._wgrad, _ENC_WKEYS, input_grad=False, run=t,
                  names=_T_ENC_BWD)
        self._wgrad_reduce()
        self._adam()

    def _step_small(self, xf, mf, mp, R, S, d, Ld, alpha):
        """The step behind the draws as miw_small_fwd -> the loss's three launches on the raw heads -> miw_small_bwd ->
        miw_small_tail (csrc/vpc_miw_small.hip), on the chain's workspace buffers."""
        t, sl, flat = self._timed, self._sl, self.model._flat
        self.last_path = "small"
        if self._part is None:
            self._part = torch.empty(miw_small_workspace(d, Ld), device=self.dev)
        RB = self.small_rb if self.small_rb else small_rows_per_workgroup(R, S)
        B = R // (2 if self.reg else 1)
        t("small_fwd", miw_small_fwd, flat, self.xin, sl["es"], self.h1, self.h2, self.heads, self.hact, self.z, self.g1,
          self.g2, self.Y, R, S, d, Ld, RB)
        t("loss", miw_loss, xf, mf, mp, self.Y, sl["Yp"], 3 * d, 1, self.hact, sl["hp"], sl["eq"], sl["ep"], self.G,
          sl["Gp"], 3 * d, self.gh, sl["ghp"], None, self.scratch, self.out8, self.tail, self.accum, B, S, d, Ld, alpha,
          PAIR_REFERENCE)
        t("small_bwd", miw_small_bwd, flat, self.xin, sl["es"], self.h1, self.h2, self.heads, self.z, self.g1, self.g2,
          self.G, self.gh, self.dht, self._part, R, S, d, Ld, RB)
        self.step_count += 1
        t("tail", miw_small_tail, self._part, R, RB, d, Ld, self.grad, flat, self.exp_avg, self.exp_avg_sq, self.lr,
          self.betas[0], self.betas[1], self.adam_eps, self.step_count)
        self._flat_written(None)
