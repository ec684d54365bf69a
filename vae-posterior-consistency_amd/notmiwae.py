"""MNAR path (BASELINE config 3): drop-in classes for the reference's

    REG_notMIWAE_v2      src/models/VAE.py:2327-2505
    notMIWAE_myversion   src/models/VAE.py:2691-2847

with the same constructor arguments, `encoder` / `decoder` / `forward` / `loss` signatures, return order and
state_dict keys (W, b, seq_encoder.{0,2}, q_mu.0, q_logstd.0, seq_decoder.{0,2}, x_mean.0, x_logvar.0 and, for the
regularised class, the unused float64 `logits.0`).  Every layer runs as an fp32 MFMA GEMM (csrc/vpc_gemm.hip), the
importance-weighted loss with the self-masking missingness model and all of its gradients in one fused kernel
(csrc/vpc_nm.hip).  The two heads of the encoder (q_mu | q_logstd) and of the decoder (x_mean | x_logvar) are
adjacent in one flat parameter buffer, so each pair is ONE GEMM.  No CPU fallback: CPU tensors raise.

What this family shares with miwae.py and flow.py lives in chainfamily.py: the encoder / decoder autograd frame (driven by
FAMILY below), the trainer frame, the host side of impute_stream, and the nm_* elementwise ops, which started here.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import check, lib, ptr, require_cuda, stream_ptr
from . import chainfamily as cf
from .chainfamily import STREAM_MAX_L, ChainDecoderFn, ChainEncoderFn, Family, _ChainTrainer, _ReferenceAttrs
from .chainfamily import impute_chunk, nm_mul, nm_prep, nm_sample, nm_sample_bwd  # noqa: F401  (defined in chainfamily.py
# only; the names stay importable from here)
from .images import FlatParams, PackedImage
from .linear import ACT_ELU, ACT_NONE, ACT_SIGMOID_HARDTANH, _f32c, chain, chain_bwd, chain_fwd
from .linear import ACT_RELU, linear_dgrad, linear_fwd, linear_wgrad, wgrad_reduce  # noqa: F401  (the GEMM ops were first
# reached as vpc_amd.notmiwae.linear_*: the names stay importable from here; they are defined in linear.py only)
from .models import Reg_VAE, vanilla_VAE
from .ops import PRECISIONS, step_pack_weights_bf16
from .trainer import chain_draw_increment

HID = 128  # VAE.py:2343-2363 hard-codes 128 (hid_dim is ignored by the reference too)


# ------------------------------------------------------------------------------------------------ raw ops
def nm_loss(x, mask, mask_p, xm_q, xl_q, ldq, xm_p, xl_p, ldp, hq, hp, W, b, eps_kl, g_xm_q, g_xl_q, g_xm_p, g_xl_p,
            ldg, ghq, ghp, gW, gb, xm_imp, scratch, out8, loss_f32, accum, B, B_global, K, d, Ld, alpha, state=None,
            rng_inc=0, gated=False):
    check(lib().vpc_nm_loss(ptr(x), ptr(mask), ptr(mask_p), ptr(xm_q), ptr(xl_q), ldq, ptr(xm_p), ptr(xl_p), ldp,
                            ptr(hq), ptr(hp), 2 * Ld, ptr(W), ptr(b), ptr(eps_kl), ptr(g_xm_q), ptr(g_xl_q), ldg,
                            ptr(g_xm_p), ptr(g_xl_p), ldg, ptr(ghq), ptr(ghp), 2 * Ld, ptr(gW), ptr(gb), 0,
                            ptr(xm_imp), ptr(scratch), scratch.numel() * scratch.element_size(), ptr(out8),
                            ptr(loss_f32), ptr(accum), ptr(state), int(rng_inc), int(gated), B, B_global, K, d, Ld,
                            float(alpha), stream_ptr()),
          "vpc_nm_loss")


def nmdec_applicable(B, K, d, Ld):
    return bool(lib().vpc_nmdec_applicable(int(B), int(K), int(d), int(Ld)))


def nmdec_tables(model, device):
    """(pack_idx, grad_idx) on the device + image size in floats for the layer-fused decoder kernel (csrc/vpc_nmdec.hip)."""
    import numpy as np
    d, Ld = model.obs_dim, model.latent_dim
    n = 2 * d + model._n_enc + model._n_dec
    pidx, gidx = np.empty(n, np.int32), np.empty(n, np.int32)
    check(lib().vpc_nmdec_build_indices(d, Ld, HID, pidx.ctypes.data_as(L.P), gidx.ctypes.data_as(L.P), n),
          "vpc_nmdec_build_indices")
    # inverse table for the layout-order reduction of the partial blocks: parameter index of a block position, -1 where none
    npart = C.c_long()
    check(lib().vpc_nmdec_layout(1, 8, d, Ld, None, C.byref(npart), None), "vpc_nmdec_layout")
    inv = np.full(npart.value, -1, np.int32)
    own = np.nonzero(gidx >= 0)[0]
    inv[gidx[own]] = own.astype(np.int32)
    # the same for the encoder-backward kernel's partial blocks
    nparte = C.c_long()
    check(lib().vpc_nmenc_build_indices(d, Ld, HID, None, C.byref(nparte), n), "vpc_nmenc_build_indices")
    inve = np.empty(nparte.value, np.int32)
    check(lib().vpc_nmenc_build_indices(d, Ld, HID, inve.ctypes.data_as(L.P), C.byref(nparte), n), "vpc_nmenc_build_indices")
    return tuple(torch.from_numpy(a).to(device) for a in (pidx, gidx, inv, inve))


def nmenc_fwd(img, xin, h1, h2, heads, R, d, Ld):
    check(lib().vpc_nmenc_fwd(ptr(img), ptr(xin), ptr(h1), ptr(h2), ptr(heads), R, d, Ld, stream_ptr()), "vpc_nmenc_fwd")


def nmenc_bwd(img, xin, h1, h2, dht, part, inv, grad, R, d, Ld):
    check(lib().vpc_nmenc_bwd(ptr(img), ptr(xin), ptr(h1), ptr(h2), ptr(dht), ptr(part), part.numel(), ptr(inv), ptr(grad),
                              R, d, Ld, stream_ptr()), "vpc_nmenc_bwd")


def nm_fused_bwd_step(img, x, mask, mask_p, xin, h1, h2, heads, eps, dht, part, stat, part_e, inv, inv_e, grad, out8, loss_f32, accum,
                      B, B_global, K, d, Ld, alpha, params, exp_avg, exp_avg_sq, lr, beta1, beta2, eps_adam, step, pack_idx):
    check(lib().vpc_nm_fused_bwd_step(ptr(img), ptr(x), ptr(mask), ptr(mask_p), ptr(xin), ptr(h1), ptr(h2), ptr(heads), 2 * Ld,
                                      ptr(eps), ptr(dht), ptr(part), ptr(stat), ptr(part_e), part_e.numel(), ptr(inv), ptr(inv_e),
                                      ptr(grad), grad.numel(), ptr(out8), ptr(loss_f32), ptr(accum), B, B_global, K, d, Ld,
                                      float(alpha), ptr(params), ptr(exp_avg), ptr(exp_avg_sq), lr, beta1, beta2, eps_adam,
                                      int(step), ptr(pack_idx), stream_ptr()), "vpc_nm_fused_bwd_step")


def nmdec_step(img, x, mask, mask_p, heads, eps, dht, part, stat, gidx, inv, grad, out8, loss_f32, accum, B, B_global, K, d,
               Ld, alpha, state=None, rng_inc=0):
    check(lib().vpc_nmdec_step(ptr(img), ptr(x), ptr(mask), ptr(mask_p), ptr(heads), 2 * Ld, ptr(eps), ptr(dht),
                               ptr(part), ptr(stat), ptr(gidx), ptr(inv), ptr(grad), grad.numel(), ptr(out8), ptr(loss_f32),
                               ptr(accum), ptr(state), int(rng_inc), B, B_global, K, d, Ld, float(alpha), stream_ptr()),
          "vpc_nmdec_step")


def _rows_view(t, B, K, d):
    """[B, K, d] tensor -> (tensor to pass, row pitch) without copying when rows b*K+k are equally spaced."""
    if t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1 and t.stride(0) == K * t.stride(1) \
            and t.stride(1) >= d:
        return t, t.stride(1)
    t = _f32c(t).reshape(B, K, d)
    return t, d


# ------------------------------------------------------------------------------------------------ autograd
_ENC_NAMES = ("We1", "be1", "We2", "be2", "Wh", "bh")
_DEC_NAMES = ("Wd1", "bd1", "Wd2", "bd2", "Wx", "bx")


def _chains(v):
    """(encoder, decoder) chains on the named views v: ELU between layers, raw heads | Sigmoid on x_mean, Hardtanh on x_logvar."""
    return (chain([v[k] for k in _ENC_NAMES], (ACT_ELU, ACT_ELU, ACT_NONE)),
            chain([v[k] for k in _DEC_NAMES], (ACT_ELU, ACT_ELU, ACT_SIGMOID_HARDTANH), v["Wxm"].shape[0]))


def _sample(heads, eps, B, K, Ld):
    """-> (z [B,K,L], heads [B, mean L | logvar L]).  VAE.py:2378-2391 / :2749-2765."""
    z = torch.empty(B * K, Ld, device=heads.device)
    nm_sample(heads, eps, z, B, K, Ld)
    return z.view(B, K, Ld), heads


def _sample_bwd(heads, eps, dz, dheads, out, B, K, Ld):
    nm_sample_bwd(torch.zeros(B * K, Ld, device=heads.device) if dz is None else dz, eps, heads, dheads, out, B, K, Ld)


# the decoder returns (x_mean, x_logvar) as the two halves of ONE [M, 2d] buffer (VAE.py:2393-2397 / :2767-2772)
FAMILY = Family(_ENC_NAMES, _DEC_NAMES, lambda x, mask, out, B, d: nm_mul(x, mask, out), _sample, _sample_bwd, 2)


class NMLossFn(torch.autograd.Function):
    """Fused importance-weighted loss + every gradient.  Returns (loss fp32, out8 fp64, xm_imp or empty)."""

    @staticmethod
    def forward(ctx, cfg, x, mask, mask_p, xm_q, xl_q, heads_q, xm_p, xl_p, heads_p, W, b, eps_kl):
        reg = mask_p is not None
        require_cuda(x, mask, mask_p, xm_q, xl_q, heads_q, xm_p, xl_p, heads_p, W, b, eps_kl)
        B, K, d, Ld = cfg["B"], cfg["K"], cfg["d"], cfg["L"]
        dev = x.device
        xm_q, ldq = _rows_view(xm_q, B, K, d)
        xl_q, ldq2 = _rows_view(xl_q, B, K, d)
        if ldq2 != ldq:
            xm_q, xl_q = xm_q.contiguous(), xl_q.contiguous()
            ldq = d
        ldp = d
        if reg:
            xm_p, ldp = _rows_view(xm_p, B, K, d)
            xl_p, ldp2 = _rows_view(xl_p, B, K, d)
            if ldp2 != ldp:
                xm_p, xl_p = xm_p.contiguous(), xl_p.contiguous()
                ldp = d
        heads_q = _f32c(heads_q)
        heads_p = _f32c(heads_p) if reg else None
        need_grad = cfg["grad"] and any(ctx.needs_input_grad)
        Gq = Gp = ghq = ghp = gW = gb = None
        if need_grad:
            Gq = torch.empty(B * K, 2 * d, device=dev)
            ghq = torch.empty(B, 2 * Ld, device=dev)
            gW = torch.empty(d, device=dev)
            gb = torch.empty(d, device=dev)
            if reg:
                Gp = torch.empty(B * K, 2 * d, device=dev)
                ghp = torch.empty(B, 2 * Ld, device=dev)
        xm_imp = torch.empty(B, d, device=dev) if cfg["impute"] else None
        nbytes = int(lib().vpc_nm_loss_scratch(B, d))
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        out8 = torch.empty(8, dtype=torch.float64, device=dev)
        half = lambda G: None if G is None else G[:, d:]
        nm_loss(x, mask, mask_p, xm_q, xl_q, ldq, xm_p, xl_p, ldp, heads_q, heads_p, W, b, eps_kl, Gq, half(Gq), Gp,
                half(Gp), 2 * d, ghq, ghp, gW, gb, xm_imp, scratch, out8, None, None, B, cfg.get("B_global", B), K, d,
                Ld, cfg["alpha"])
        ctx.reg, ctx.need_grad, ctx.dims = reg, need_grad, (B, K, d, Ld)
        ctx.wshape = W.shape
        if need_grad:
            ctx.save_for_backward(*[t for t in (Gq, ghq, gW, gb, Gp, ghp) if t is not None])
        loss = out8[0].float()
        imp = xm_imp if xm_imp is not None else torch.empty(0, device=dev)
        ctx.mark_non_differentiable(out8, imp)
        return loss, out8, imp

    @staticmethod
    def backward(ctx, gloss, _g8, _gi):
        if not ctx.need_grad:
            return (None,) * 13
        B, K, d, Ld = ctx.dims
        t = ctx.saved_tensors
        Gq, ghq, gW, gb = t[:4]
        Gq, ghq, gW, gb = Gq * gloss, ghq * gloss, gW * gloss, gb * gloss
        Gq3 = Gq.view(B, K, 2 * d)
        gWs, gbs = gW.view(ctx.wshape), gb.view(ctx.wshape)
        if ctx.reg:
            Gp, ghp = t[4] * gloss, t[5] * gloss
            Gp3 = Gp.view(B, K, 2 * d)
            return (None, None, None, None, Gq3[..., :d], Gq3[..., d:], ghq, Gp3[..., :d], Gp3[..., d:], ghp, gWs, gbs,
                    None)
        return None, None, None, None, Gq3[..., :d], Gq3[..., d:], ghq, None, None, None, gWs, gbs, None


# ------------------------------------------------------------------------------------------------ model classes
class _NMBase(_ReferenceAttrs, FlatParams, nn.Module):
    regularised = False
    # flat parameter buffer: [W b | We1 be1 We2 be2 Wmu Wls bmu bls | Wd1 bd1 Wd2 bd2 Wxm Wxl bxm bxl]; the two heads of the
    # encoder and of the decoder are adjacent, so each pair is one GEMM operand (Wh / bh, Wx / bx)
    _flat_spec = (("W", "W", "wb", (-1,)), ("b", "b", "wb", (-1,)),
                  ("We1", "seq_encoder.0.weight", "enc"), ("be1", "seq_encoder.0.bias", "enc"),
                  ("We2", "seq_encoder.2.weight", "enc"), ("be2", "seq_encoder.2.bias", "enc"),
                  ("Wmu", "q_mu.0.weight", "enc"), ("Wls", "q_logstd.0.weight", "enc"),
                  ("bmu", "q_mu.0.bias", "enc"), ("bls", "q_logstd.0.bias", "enc"),
                  ("Wd1", "seq_decoder.0.weight", "dec"), ("bd1", "seq_decoder.0.bias", "dec"),
                  ("Wd2", "seq_decoder.2.weight", "dec"), ("bd2", "seq_decoder.2.bias", "dec"),
                  ("Wxm", "x_mean.0.weight", "dec"), ("Wxl", "x_logvar.0.weight", "dec"),
                  ("bxm", "x_mean.0.bias", "dec"), ("bxl", "x_logvar.0.bias", "dec"))
    _flat_aliases = {"Wh": ("Wmu", "Wls"), "bh": ("bmu", "bls"), "Wx": ("Wxm", "Wxl"), "bx": ("bxm", "bxl")}
    _build_chains = staticmethod(_chains)

    def __init__(self, obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates):
        super().__init__()
        self._init_reference_attrs("MNAR", obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates)
        d, Ld = obs_dim, latent_dim
        # parameter containers, created in the reference's order (same seed -> same initial weights)
        self.seq_encoder = nn.Sequential(nn.Linear(d, HID), nn.ELU(), nn.Linear(HID, HID), nn.ELU())
        self.q_mu = nn.Sequential(nn.Linear(HID, Ld))
        self.q_logstd = nn.Sequential(nn.Linear(HID, Ld))
        self.seq_decoder = nn.Sequential(nn.Linear(Ld, HID), nn.ELU(), nn.Linear(HID, HID), nn.ELU())
        self.x_mean = nn.Sequential(nn.Linear(HID, d), nn.Sigmoid())
        self.x_logvar = nn.Sequential(nn.Linear(HID, d), nn.Hardtanh(min_val=-10.0, max_val=0))
        emb1 = torch.empty([1, 1, d])
        nn.init.xavier_uniform_(emb1)
        self.W = nn.Parameter(emb1)
        emb2 = torch.empty([1, 1, d])
        nn.init.xavier_uniform_(emb2)
        self.b = nn.Parameter(emb2)
        self.activation = nn.Softplus()
        self._flat = None

    # ---- reference API
    def _encode(self, x, mask, sample=True, eps=None):
        L.require_cuda(x)
        d, Ld, K = self.obs_dim, self.latent_dim, self.num_samples
        xf = _f32c(x.reshape(-1, d))
        mf = _f32c(mask.reshape(-1, d).to(x.device))
        B = xf.shape[0]
        if sample and eps is None:
            eps = torch.randn(B, K, Ld, device=xf.device)  # Normal(mean, std).rsample(), VAE.py:2387 / :2761
        z, heads = ChainEncoderFn.apply(FAMILY, self, xf, mf, _f32c(eps) if sample else None, K, *self._enc_weights())
        mean = heads[:, :Ld].unsqueeze(1).expand(B, K, Ld)
        log_var = heads[:, Ld:].unsqueeze(1).expand(B, K, Ld)
        mean._vpc_heads = heads
        log_var._vpc_heads = heads
        return z, mean, log_var

    def encoder(self, x, mask, sample=True):
        """VAE.py:2378-2391 / :2749-2765 -> (z, mean, log_var), each [B, num_samples, latent_dim]."""
        return self._encode(x, mask, sample)

    def decoder(self, z_int):
        """VAE.py:2393-2397 / :2767-2772 -> (x_mean, x_logvar)."""
        L.require_cuda(z_int)
        return ChainDecoderFn.apply(FAMILY, self, z_int, *self._dec_weights())

    @staticmethod
    def _heads_of(mean, logvar):
        h = getattr(mean, "_vpc_heads", None)
        if h is not None and h is getattr(logvar, "_vpc_heads", None):
            return h
        return torch.cat([mean[:, 0, :], logvar[:, 0, :]], 1)  # any [B,K,L] pair replicated over K

    def _loss(self, x, mask, mask_p, outs_q, outs_p, alpha, eps_kl, llh_eval):
        d, Ld, K = self.obs_dim, self.latent_dim, self.num_samples
        xf = _f32c(x.reshape(-1, d))
        B = xf.shape[0]
        cfg = dict(B=B, K=K, d=d, L=Ld, alpha=alpha, grad=torch.is_grad_enabled(), impute=bool(llh_eval))
        xm_q, xl_q, mean_q, logvar_q = outs_q
        hq = self._heads_of(mean_q, logvar_q)
        mf = _f32c(mask.reshape(-1, d).to(xf.device))
        if outs_p is not None:
            xm_p, xl_p, mean_p, logvar_p = outs_p
            hp = self._heads_of(mean_p, logvar_p)
            mpf = _f32c(mask_p.reshape(-1, d).to(xf.device))
        else:
            xm_p = xl_p = hp = mpf = None
        loss, out8, imp = NMLossFn.apply(cfg, xf, mf, mpf, xm_q, xl_q, hq, xm_p, xl_p, hp, self.W, self.b, eps_kl)
        if llh_eval:  # VAE.py:2458-2461 / :2810-2813
            return imp, loss, out8[5].float()
        return loss, loss  # (print_loss, train_loss)

    def forward_loss(self, x, mask, mask_p=None, **schedule):
        """forward, then loss, in the order and with the keywords of the dense classes: the reference's drivers call the MNAR
        pair through the same branches (train.py:87-101; evaluate.py:33-50).  With llh_eval the imputation is loss's first
        return, so there is no X_MEAN_Q here."""
        return (Reg_VAE if self.regularised else vanilla_VAE).forward_loss(self, x, mask, mask_p, **schedule)


class REG_notMIWAE_v2(_NMBase):
    """Posterior-consistency regularised not-MIWAE.  Reference: src/models/VAE.py:2327-2505."""
    regularised = True

    def __init__(self, obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates):
        super().__init__(obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates)
        self.logits = nn.Sequential(nn.Linear(obs_dim, obs_dim)).double()  # VAE.py:2371: unused, but in state_dict
        self.max_epoch = 2800

    def forward(self, data, mask, mask_p, stage="train"):
        # VAE.py:2500-2505: q pass first (RNG order), p outputs returned first
        z_q, mean_q, logvar_q = self.encoder(data, mask)
        x_mean_q, x_logvar_q = self.decoder(z_q)
        z_p, mean_p, logvar_p = self.encoder(data, mask_p)
        x_mean_p, x_logvar_p = self.decoder(z_p)
        return mean_p, logvar_p, x_mean_p, x_logvar_p, mean_q, logvar_q, x_mean_q, x_logvar_q

    def loss(self, x, x_recon_p, x_logvar_p, mean_p, logvar_p, x_recon_q, x_logvar_q, mean_q, logvar_q, mask, mask_p,
             epoch, vae_elbo=False, llh_eval=False, MI=False, beta_annealing=False, beta=1.0, alpha=1.0,
             alpha_annealing=False, stage="train", missing_process="selfmasking_known"):
        """VAE.py:2398-2471.  epoch / beta / annealing flags are accepted and, as in the reference, unused."""
        if missing_process != "selfmasking_known":
            raise NotImplementedError("only the reference's default missing_process='selfmasking_known' is accelerated")
        if MI:
            raise NotImplementedError("the MI branch of the reference reads undefined names (VAE.py:2463-2467)")
        return self._loss(x, mask, mask_p, (x_recon_q, x_logvar_q, mean_q, logvar_q),
                          (x_recon_p, x_logvar_p, mean_p, logvar_p), alpha, None, llh_eval)


class notMIWAE_myversion(_NMBase):
    """not-MIWAE with a Monte-Carlo KL.  Reference: src/models/VAE.py:2691-2847."""

    def forward(self, data, mask, stage="train"):
        z, mean, logvar = self.encoder(data, mask)
        x_mean, x_logvar = self.decoder(z)
        return mean, logvar, x_mean, x_logvar

    def loss(self, x, x_recon, x_logvar, mean, logvar, epoch, mask, vae_elbo=False, llh_eval=False, MI=False,
             beta_annealing=False, beta=1.0, stage="train", missing_process="selfmasking_known", eps_kl=None):
        """VAE.py:2774-2823; draws the fresh z of :2791-2793 on the device unless eps_kl [B,K,L] is given."""
        if missing_process != "selfmasking_known":
            raise NotImplementedError("only the reference's default missing_process='selfmasking_known' is accelerated")
        if MI:
            raise NotImplementedError("the MI branch of the reference reads undefined names (VAE.py:2815-2819)")
        B = x.reshape(-1, self.obs_dim).shape[0]
        if eps_kl is None:
            eps_kl = torch.randn(B, self.num_samples, self.latent_dim, device=x.device)
        return self._loss(x, mask, None, (x_recon, x_logvar, mean, logvar), None, 0.0, _f32c(eps_kl), llh_eval)


# ------------------------------------------------------------------------------------------------ streaming imputation
STREAM_MAX_D = 128  # obs_dim limit of csrc/vpc_nm_impute.hip (latent_dim: chainfamily.STREAM_MAX_L)


def nm_impute_scratch(B, S, d, Ld, s_chunk):
    """Floats of the partial buffer of nm_impute: B * ceil(S / s_chunk16) * (2 + d); 0 for a shape outside the kernel's
    limits (obs_dim <= 128, latent_dim <= 16, B, S, s_chunk >= 1)."""
    return int(lib().vpc_nm_impute_scratch(int(B), int(S), int(d), int(Ld), int(s_chunk)))


def nm_impute(flat, x, mask, eps, seed, offset, row0, part, xm, lse, B, S, d, Ld, s_chunk, regularised):
    check(lib().vpc_nm_impute(ptr(flat), ptr(x), ptr(mask), ptr(eps), int(seed), int(offset), int(row0), ptr(part),
                              part.numel(), ptr(xm), ptr(lse), int(B), int(S), int(d), int(Ld), int(s_chunk),
                              int(bool(regularised)), stream_ptr()), "vpc_nm_impute")


def impute_stream(model, x, mask, num_samples=None, eps=None, seed=None, offset=0, row0=0, s_chunk=None,
                  return_lse=False, missing_process="selfmasking_known"):
    """The llh_eval imputation of every row of x with num_samples draws (evaluate.py:13-69 through VAE.py:2398-2461 /
    :2774-2813) in two launches: csrc/vpc_nm_impute.hip runs encoder, sampler, decoder, log-weights and an online softmax
    per (row, chunk of s_chunk samples) and never writes a decoder row; the merge combines a row's chunks in chunk order.
    Returns xm [B, d], or (xm, lse [B]) with return_lse: lse = the per-row log-sum-exp of -l_w.

    mask_p is not an argument, for REG_notMIWAE_v2 too: the reference's imputation takes the q pass's weights and the q
    pass's x_mean only (VAE.py:2458-2461), so the whole p pass - which evaluate.py:33-42 computes and drops - is skipped.

    eps [2, B, S, L] injects the sampler's draw and, for notMIWAE_myversion, the fresh draw of :2791-2798 (plane 1 is not
    read for the regularised class); otherwise both are drawn in the kernel from (seed, offset, row0) - seed None takes
    one from torch's generator - by the rule of trainer.impute_draw_counter, which does not depend on s_chunk:
    miwae.impute_draws returns those values, and rows [a, b) of a call equal the call on x[a:b] with row0 = a.  s_chunk
    None: impute_chunk.  For a given s_chunk the result is bit-reproducible.  obs_dim <= 128, latent_dim <= 16; anything
    else, CPU tensors, a wrong eps shape, s_chunk < 1 or a missing_process other than the default raise VpcError (no
    fallback to the chain)."""
    if not isinstance(model, _NMBase):
        raise L.VpcError("notmiwae.impute_stream supports REG_notMIWAE_v2 and notMIWAE_myversion")
    if missing_process != "selfmasking_known":
        raise L.VpcError("impute_stream: only the reference's default missing_process='selfmasking_known' is accelerated")
    d, Ld = model.obs_dim, model.latent_dim

    def launch(flat, *args):
        if flat.numel() != 2 * d + model._n_enc + model._n_dec:  # the kernel reads the buffer by the offsets of _flat_spec
            raise L.VpcError(f"impute_stream: flat parameter buffer of {flat.numel()} floats for (d, L) = {(d, Ld)}")
        nm_impute(flat, *args, model.regularised)
    return cf.impute_stream(model, x, mask, num_samples, eps, seed, offset, row0, s_chunk, return_lse, STREAM_MAX_D,
                            STREAM_MAX_L, nm_impute_scratch, launch)


# ------------------------------------------------------------------------------------------------ fused step
# timer names of the chain launches, per layer, and the weight gradients' (timer name, index in the trainer's workspace)
_ENC_FWD, _ENC_BWD = ("enc_fwd",) * 3, ("enc_bwd",) * 3
_DEC_FWD, _DEC_DGRAD = ("dec_fwd1", "dec_fwd2", "dec_fwd3"), ("dec_dgrad1", "dec_dgrad2", "dec_dgrad3")
_DEC_WKEYS = (("dec_wgrad1", 2), ("dec_wgrad2", 1), ("dec_wgrad3", 0))
_ENC_WKEYS = (("enc_bwd", 5), ("enc_bwd", 4), ("enc_bwd", 3))


class NMTrainer(_ChainTrainer):
    """The whole training step of the MNAR path (train.py:28-117 for 'reg_notMIWAE*' / 'vanilla_notMIWAE*') as a
    fixed sequence of HIP launches, no host synchronisation: float mask_p draw + stacked encoder input, Philox
    normals, encoder / decoder GEMM chains with the q and p passes STACKED along the batch (one GEMM per layer for
    both passes), the fused loss kernel, the backward GEMM chain writing straight into one flat gradient buffer,
    one all-reduce of [grads | loss] under data parallelism, flat Adam."""
    family, model_base, model_names = FAMILY, _NMBase, "REG_notMIWAE_v2 and notMIWAE_myversion"

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, process_group=None, world_size=1, rank=0,
                 precision="f32"):
        """precision: "f32", "bf16x3" or "bf16" for the 17 GEMMs of the step (csrc/vpc_bf16.h; operands stay fp32 in
        memory and are converted in registers); the loss kernel and Adam are fp32 in every mode.  (`eps` is Adam's
        epsilon, `self.adam_eps`; `self.eps` is the step's workspace of normals.)"""
        super().__init__(model, lr, betas, eps, seed, process_group, world_size, rank)
        if precision not in PRECISIONS:
            raise ValueError(f"precision {precision!r}: expected one of {sorted(PRECISIONS)}")
        self.precision, self.prec = precision, PRECISIONS[precision]
        self.loss = self.tail  # [grads | loss] -> ONE all-reduce per step

    def invalidate_image(self):
        """Alias of model.invalidate_images(): after writing parameters behind torch's version counters."""
        self.model.invalidate_images()

    def _buffers(self, B, e):
        m, dev = self.model, self.dev
        d, Ld, K = m.obs_dim, m.latent_dim, m.num_samples
        P = 2 if self.reg else 1
        R, M = P * B, P * B * K
        self.xin, self.mask_p = e(R, d), e(B, d)
        self.h1, self.h2, self.heads = e(R, HID), e(R, HID), e(R, 2 * Ld)
        self.eps = e(2, B, K, Ld)  # reg: eps_q, eps_p; vanilla: eps (sampling), eps_kl (MC KL)
        # layer-fused decoder (plain bf16, obs_dim 128, both model classes): nothing of B * K rows is materialised
        self.use_nmdec = bool(self.prec == 2 and nmdec_applicable(B, K, d, Ld))
        Mg = 0 if self.use_nmdec else M  # rows of the GEMM chain's decoder-side workspaces
        self.z, self.g1, self.g2, self.Y = e(Mg, Ld), e(Mg, HID), e(Mg, HID), e(Mg, 2 * d)
        self.G, self.gheads, self.dht = e(Mg, 2 * d), e(R, 2 * Ld), e(R, 2 * Ld)
        self.dg2, self.dg1, self.dz = e(Mg, HID), e(Mg, HID), e(Mg, Ld)
        Rg = 0 if self.use_nmdec else R     # (the fused path's encoder backward is one kernel too: nmenc_bwd)
        self.dh2, self.dh1 = e(Rg, HID), e(Rg, HID)
        nbytes = int(lib().vpc_nm_loss_scratch(B, d))
        self.scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        # the slices the step passes to its launches, made once per batch size (a tensor view costs 1-3 us of host time, and the
        # eager step at the reference's batch 128 is paced by the host)
        BK = B * K
        Y, G = self.Y, self.G
        self._sl = dict(Yl=Y[:, d:], Yp=Y[BK:] if self.reg else None, Ypl=Y[BK:, d:] if self.reg else None, Gl=G[:, d:],
                        Gp=G[BK:] if self.reg else None, Gpl=G[BK:, d:] if self.reg else None,
                        hp=self.heads[B:] if self.reg else None, ghp=self.gheads[B:] if self.reg else None,
                        eps0=self.eps[0], eps1=self.eps[1])
        if self.use_nmdec:  # image, partial blocks, index tables
            nimg, npart, nblk = C.c_int(), C.c_long(), C.c_int()
            check(lib().vpc_nmdec_layout(B, K, d, Ld, C.byref(nimg), C.byref(npart), C.byref(nblk)), "vpc_nmdec_layout")
            if getattr(self, "_nd_tables", None) is None:
                self._nd_tables = nmdec_tables(m, dev)
                self.nd_img = torch.zeros(nimg.value, device=dev)
                # ONE image (decoder, missingness model, encoder), packed lazily under the model's parameter key (images.py)
                pidx = self._nd_tables[0]
                self._nd = PackedImage(self.nd_img, lambda flat, buf: step_pack_weights_bf16(flat, pidx, buf))
            self.nd_part = e(nblk.value * npart.value)
            self.ne_part = e(nblk.value * int(self._nd_tables[3].numel()))  # the encoder-backward kernel's blocks (fused tail)
            self.nd_stat = torch.empty(nblk.value * 5, dtype=torch.float64, device=dev)
        return (R, M, [self.xin, self.h1, self.h2, self.heads], [None, self.dh1, self.dh2, self.dht],
                [self.z, self.g1, self.g2, self.Y], [self.dz, self.dg1, self.dg2, self.G])

    def step(self, x, mask, mask_p=None, eps=None, *, alpha=1.0, p_missingness=30, global_batch=None, row_lo=None,
             _state=None):
        """One optimiser step.  mask_p / eps ([2, B, K, L]: (eps_q, eps_p) or (eps, eps_kl)) may be injected for
        parity tests; otherwise they are drawn on the device (one launch: mask_p + stacked encoder input + normals).
        Data parallel: this rank holds rows [row_lo, row_lo + B) (default rank * B) of `global_batch` rows; the Philox
        counters are those of the global row, so the draws do not depend on the world size."""
        m = self.model
        v = m._views()
        d, Ld, K = m.obs_dim, m.latent_dim, m.num_samples
        xf, mf = _f32c(x.reshape(-1, d)), _f32c(mask.reshape(-1, d))
        L.require_cuda(xf, mf)
        B = xf.shape[0]
        Bg, row_lo = self._batch_rows(B, global_batch or None, row_lo)  # every rank normalises by the GLOBAL batch: SUM over ranks = result
        self._ws(B, v)
        reg = self.reg
        P = 2 if reg else 1
        R, M, BK = P * B, P * B * K, B * K
        t = self._timed
        rng_inc = chain_draw_increment(2 * Bg * K * Ld, Bg, d)  # what the GLOBAL batch consumes
        sharded = (row_lo * d) % 4 == 0 and (K * Ld) % 4 == 0
        # shapes whose shards do not start on a Philox group: per-rank counter streams instead of global-row counters
        rank_off = 0 if sharded else (self.rank << 44)
        eps_shard = (B, Bg, row_lo, K * Ld) if sharded else None
        # ---- inputs
        mp = self._draw_inputs(xf, mf, mask_p, eps, B, d, p_missingness, rng_inc, _state, rank_off, eps_shard,
                               row_lo * d if sharded else 0)
        # ---- forward
        # single device, eager: everything behind the encoder forward is three launches (decoder tiles, encoder-backward tiles, one tail
        # that reduces both sets of blocks, applies Adam and re-packs the image: vpc_nm_fused_bwd_step) and the pack launch goes
        fuse_tail = self.use_nmdec and self.world_size == 1 and _state is None and self.timers is None
        if self.use_nmdec:
            # plain bf16 at obs_dim 128: the encoder forward as one kernel (csrc/vpc_nmdec.hip: nmenc_fwd_kernel) instead of three
            # GEMM launches, on the image the fused tail of the previous step re-packed (or re-packed here)
            key = m._param_key(self._plist)
            if _state is not None:
                self._nd.stamp(None)  # graph capture: every replay re-packs
            t("pack", self._nd.get, key, m._flat)
            t("enc_fwd", nmenc_fwd, self.nd_img, self.xin, self.h1, self.h2, self.heads, R, d, Ld)
        else:
            chain_fwd(self.enc_layers, self.enc_acts, R, self.prec, t, _ENC_FWD)
        if self.use_nmdec:
            # K-fold rsample, decoder, loss, decoder backward and the K-fold sum of dz in ONE kernel (csrc/vpc_nmdec.hip): the
            # decoder / missingness-model gradients land in self.grad, d loss / d heads in self.dht
            pidx, gidx, ginv, einv = self._nd_tables
            if fuse_tail:
                self.step_count += 1
                nm_fused_bwd_step(self.nd_img, xf, mf, mp, self.xin, self.h1, self.h2, self.heads, self.eps, self.dht, self.nd_part,
                                  self.nd_stat, self.ne_part, ginv, einv, self.grad, self.out8, self.loss, self.accum, B, Bg, K, d,
                                  Ld, alpha, m._flat, self.exp_avg, self.exp_avg_sq, self.lr, self.betas[0], self.betas[1],
                                  self.adam_eps, self.step_count, pidx)
                self._flat_written(key, self._nd)
                return
            t("dec_fused", nmdec_step, self.nd_img, xf, mf, mp, self.heads, self.eps, self.dht, self.nd_part, self.nd_stat,
              gidx, ginv, self.grad, self.out8, self.loss, self.accum if self.world_size == 1 else None, B, Bg, K, d, Ld, alpha,
              _state, rng_inc)
            # the encoder's backward in one kernel + its reduction (nmenc_bwd_kernel), through the decoder's partial-block buffer
            t("enc_bwd", nmenc_bwd, self.nd_img, self.xin, self.h1, self.h2, self.dht, self.nd_part, einv, self.grad, R, d, Ld)
        else:
            # weight gradients: partials per layer, all summed by one launch after the last one (6 reduction launches less)
            self._step_decoder_gemms(xf, mf, mp, B, Bg, alpha, _state, rng_inc, t, v)
            chain_bwd(self.enc_layers, self.enc_acts, self.enc_dacts, R, self._wgrad, _ENC_WKEYS, input_grad=False,
                      precision=self.prec, run=t, names=_ENC_BWD)
            self._wgrad_reduce()
        dp = self.world_size > 1
        if dp:
            self._allreduce()
        self._adam(None if _state is None else _state[0:1], self.loss if dp else None, self.accum if dp else None)

    def _step_decoder_gemms(self, xf, mf, mp, B, Bg, alpha, _state, rng_inc, t, v):
        """Decoder forward, loss and decoder backward as the GEMM chain (every precision, both model classes)."""
        m, reg = self.model, self.reg
        d, Ld, K = m.obs_dim, m.latent_dim, m.num_samples
        P = 2 if reg else 1
        R, M, BK = P * B, P * B * K, B * K
        sl = self._sl
        t("sample", nm_sample, self.heads, self.eps if reg else sl["eps0"], self.z, R, K, Ld)
        chain_fwd(self.dec_layers, self.dec_acts, M, self.prec, t, _DEC_FWD)
        # ---- loss + output-side gradients
        Y, G = self.Y, self.G
        t("loss", nm_loss, xf, mf, mp, Y, sl["Yl"], 2 * d, sl["Yp"], sl["Ypl"], 2 * d,
          self.heads, sl["hp"], v["W"], v["b"], None if reg else sl["eps1"], G, sl["Gl"],
          sl["Gp"], sl["Gpl"], 2 * d, self.gheads, sl["ghp"],
          self.g["W"], self.g["b"], None, self.scratch, self.out8, self.loss,
          self.accum if self.world_size == 1 else None,  # data parallel: the epoch total takes the ALL-REDUCED loss (below)
          B, Bg, K, d, Ld, alpha, _state, rng_inc, True)
        # ---- backward (G already holds the head pre-activation gradients: no gate pass over Y)
        chain_bwd(self.dec_layers, self.dec_acts, self.dec_dacts, M, self._wgrad, _DEC_WKEYS, precision=self.prec, run=t,
                  names=_DEC_DGRAD)
        t("sample_bwd", nm_sample_bwd, self.dz, self.eps if reg else sl["eps0"], self.heads, self.gheads, self.dht, R,
          K, Ld)

    def step_graph(self, x, mask, *, alpha=1.0, p_missingness=30):
        """The same step replayed from a captured HIP graph (torch.cuda.CUDAGraph): ONE host call instead of ~30
        launches.  Step count and Philox offsets live on the device (`state`), bumped by the loss kernel's finalize.
        The first call with a new (shape, alpha, p_missingness) runs one eager step and captures.  Measured on
        MI355X this removes the host cost but not the ~10 us dependent-dispatch latency per kernel node, so at
        B = 128 it is no faster than step() (profiles/r01_notes.md).  Single process only."""
        if self.world_size > 1:
            return self.step(x, mask, alpha=alpha, p_missingness=p_missingness)
        d = self.model.obs_dim
        xf, mf = _f32c(x.reshape(-1, d)), _f32c(mask.reshape(-1, d))
        L.require_cuda(xf, mf)
        self._graph_step((tuple(xf.shape), float(alpha), p_missingness), (xf, mf),
                         lambda *a, **k: self.step(*a, alpha=alpha, p_missingness=p_missingness, **k))
