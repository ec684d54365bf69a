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
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import check, lib, ptr, require_cuda, stream_ptr
from .images import ParamKeyMixin
from .notmiwae import ACT_ELU, ACT_NONE, ACT_SIGMOID_HARDTANH, _f32c, linear_dgrad, linear_fwd, linear_wgrad, wgrad_reduce
from .trainer import _FlatAdamTrainer

FLOW_L = 10      # VPC_FLOW_LATENT: latent dim = spline bins
CTX = 100        # seq_encoder output = the 10 x 10 spline contexts
OBS_LOGVAR = -8.0  # VAE.py:1875 / :2014
STAGE_TRAIN, STAGE_EVAL = 0, 1


# ------------------------------------------------------------------------------------------------ raw ops
def flow_prep(x, mask, mask_p_in, mask_p_out, xin, eps_out, B, d, keep_prob=1.0, seed=0, offset=0, offset_eps=0):
    check(lib().vpc_flow_prep(ptr(x), ptr(mask), ptr(mask_p_in), ptr(mask_p_out), ptr(xin), ptr(eps_out),
                              0 if eps_out is None else eps_out.numel(), int(B), int(d), float(keep_prob), int(seed),
                              int(offset), int(offset_eps), stream_ptr()), "vpc_flow_prep")


def flow_fwd(t, eps, z, zlp, R, B):
    check(lib().vpc_flow_fwd(ptr(t), CTX, ptr(eps), ptr(z), ptr(zlp), int(R), int(B), stream_ptr()), "vpc_flow_fwd")


def flow_bwd(t, eps, dz, dz2, dzlp, dt, R, B):
    check(lib().vpc_flow_bwd(ptr(t), CTX, ptr(eps), ptr(dz), ptr(dz2), ptr(dzlp), ptr(dt), CTX, int(R), int(B),
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


def _mask_f32(m, d, device):
    return _f32c(m.reshape(-1, d).to(device))


# ------------------------------------------------------------------------------------------------ autograd
class FlowEncoderFn(torch.autograd.Function):
    """(x, mask, eps) -> (z, z_log_prob) [B, 10].  seq_encoder(cat[x*mask, mask]) then Flow.forward (VAE.py:1924-1931)."""

    @staticmethod
    def forward(ctx, model, x, mask, eps, *weights):
        require_cuda(x, mask, eps, *weights)
        v = model._views()
        d, H = model.obs_dim, model.hid_dim
        B, dev = x.shape[0], x.device
        xin = torch.empty(B, 2 * d, device=dev)
        flow_prep(x, mask, None, None, xin, None, B, d)
        h1, h2, t = torch.empty(B, H, device=dev), torch.empty(B, H, device=dev), torch.empty(B, CTX, device=dev)
        linear_fwd(xin, v["We1"], v["be1"], h1, B, H, 2 * d, ACT_ELU)
        linear_fwd(h1, v["We2"], v["be2"], h2, B, H, H, ACT_ELU)
        linear_fwd(h2, v["We3"], v["be3"], t, B, CTX, H, ACT_NONE)
        z, zlp = torch.empty(B, FLOW_L, device=dev), torch.empty(B, FLOW_L, device=dev)
        flow_fwd(t, eps, z, zlp, B, B)
        ctx.model = model
        ctx.save_for_backward(xin, h1, h2, t, eps)
        return z, zlp

    @staticmethod
    def backward(ctx, dz, dzlp):
        model = ctx.model
        xin, h1, h2, t, eps = ctx.saved_tensors
        v = model._views()
        d, H = model.obs_dim, model.hid_dim
        B, dev = xin.shape[0], xin.device
        dt = torch.empty(B, CTX, device=dev)
        flow_bwd(t, eps, None if dz is None else _f32c(dz), None, None if dzlp is None else _f32c(dzlp), dt, B, B)
        g = model._segment_views(torch.empty(model._n_enc, device=dev), "enc")
        dh2, dh1 = torch.empty(B, H, device=dev), torch.empty(B, H, device=dev)
        linear_wgrad(dt, h2, g["We3"], g["be3"], B, CTX, H)
        linear_dgrad(dt, v["We3"], dh2, B, CTX, H, x_out=h2, act_prev=ACT_ELU)
        linear_wgrad(dh2, h1, g["We2"], g["be2"], B, H, H)
        linear_dgrad(dh2, v["We2"], dh1, B, H, H, x_out=h1, act_prev=ACT_ELU)
        linear_wgrad(dh1, xin, g["We1"], g["be1"], B, H, 2 * d)
        return (None, None, None, None, g["We1"], g["be1"], g["We2"], g["be2"], g["We3"], g["be3"])


class FlowDecoderFn(torch.autograd.Function):
    """z [.., 10] -> x_mean = sigmoid(decoder_mean(seq_decoder(z))) (VAE.py:1943-1948)."""

    @staticmethod
    def forward(ctx, model, z, *weights):
        require_cuda(z, *weights)
        v = model._views()
        d, H = model.obs_dim, model.hid_dim
        lead = z.shape[:-1]
        z2 = _f32c(z).reshape(-1, FLOW_L)
        M, dev = z2.shape[0], z2.device
        gs = [torch.empty(M, H, device=dev) for _ in range(4)]
        Y = torch.empty(M, d, device=dev)
        linear_fwd(z2, v["Wd1"], v["bd1"], gs[0], M, H, FLOW_L, ACT_ELU)
        for i in range(1, 4):
            linear_fwd(gs[i - 1], v[f"Wd{i + 1}"], v[f"bd{i + 1}"], gs[i], M, H, H, ACT_ELU)
        linear_fwd(gs[3], v["Wm"], v["bm"], Y, M, d, H, ACT_SIGMOID_HARDTANH, d)
        ctx.model, ctx.lead = model, lead
        ctx.save_for_backward(z2, *gs, Y)
        return Y.view(*lead, d)

    @staticmethod
    def backward(ctx, gy):
        model = ctx.model
        z2, g1, g2, g3, g4, Y = ctx.saved_tensors
        gs = [g1, g2, g3, g4]
        v = model._views()
        d, H = model.obs_dim, model.hid_dim
        M, dev = z2.shape[0], z2.device
        G = _f32c(gy).reshape(M, d)
        g = model._segment_views(torch.empty(model._n_dec, device=dev), "dec")
        dg = [torch.empty(M, H, device=dev) for _ in range(4)]
        dz = torch.empty(M, FLOW_L, device=dev)
        linear_wgrad(G, g4, g["Wm"], g["bm"], M, d, H, y_gate=Y, gate=ACT_SIGMOID_HARDTANH, gate_split=d)
        linear_dgrad(G, v["Wm"], dg[3], M, d, H, y_gate=Y, gate=ACT_SIGMOID_HARDTANH, gate_split=d, x_out=g4,
                     act_prev=ACT_ELU)
        for i in range(3, 0, -1):  # seq_decoder.{6,4,2}
            linear_wgrad(dg[i], gs[i - 1], g[f"Wd{i + 1}"], g[f"bd{i + 1}"], M, H, H)
            linear_dgrad(dg[i], v[f"Wd{i + 1}"], dg[i - 1], M, H, H, x_out=gs[i - 1], act_prev=ACT_ELU)
        linear_wgrad(dg[0], z2, g["Wd1"], g["bd1"], M, H, FLOW_L)
        linear_dgrad(dg[0], v["Wd1"], dz, M, H, FLOW_L)
        return (None, dz.view(*ctx.lead, FLOW_L), *[g[k] for k in model._DEC_NAMES])


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


class _FlowBase(ParamKeyMixin, nn.Module):
    regularised = False
    _ENC_NAMES = ("We1", "be1", "We2", "be2", "We3", "be3")
    _DEC_NAMES = ("Wd1", "bd1", "Wd2", "bd2", "Wd3", "bd3", "Wd4", "bd4", "Wm", "bm")

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
        self._view_cache = None
        self._n_enc = H * 2 * d + H + H * H + H + CTX * H + CTX
        self._n_dec = H * Ld + H + 3 * (H * H + H) + d * H + d

    @property
    def prior(self):  # VAE.py:1920 (Normal(prior_mean, prior_std))
        return torch.distributions.Normal(self.prior_mean, self.prior_std)

    # ---- flat parameter buffer: [We1 be1 We2 be2 We3 be3 | Wd1 bd1 .. Wd4 bd4 Wm bm] = state_dict order
    def trainable(self):
        se, sd, dm = self.seq_encoder, self.seq_decoder, self.decoder_mean[0]
        return [se[0].weight, se[0].bias, se[2].weight, se[2].bias, se[4].weight, se[4].bias,
                sd[0].weight, sd[0].bias, sd[2].weight, sd[2].bias, sd[4].weight, sd[4].bias, sd[6].weight, sd[6].bias,
                dm.weight, dm.bias]

    def flatten_parameters(self):
        """Make the 16 trainable tensors views of ONE flat fp32 buffer.  Idempotent; call again after .to()."""
        ps = self.trainable()
        flat = self._flat
        ok = flat is not None and flat.device == ps[0].device
        off = 0
        if ok:
            for p in ps:
                if p.data.data_ptr() != flat.data_ptr() + 4 * off or not p.data.is_contiguous():
                    ok = False
                    break
                off += p.numel()
        if not ok:
            flat = torch.cat([p.data.detach().reshape(-1).float() for p in ps]).contiguous()
            off = 0
            for p in ps:
                p.data = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
            self._flat = flat
            self._view_cache = None
        return self._flat

    def _segment_views(self, buf, which):
        d, H = self.obs_dim, self.hid_dim
        if which == "enc":
            spec = [("We1", (H, 2 * d)), ("be1", (H,)), ("We2", (H, H)), ("be2", (H,)), ("We3", (CTX, H)),
                    ("be3", (CTX,))]
        else:
            spec = [("Wd1", (H, FLOW_L)), ("bd1", (H,))]
            for i in (2, 3, 4):
                spec += [(f"Wd{i}", (H, H)), (f"bd{i}", (H,))]
            spec += [("Wm", (d, H)), ("bm", (d,))]
        out, off = {}, 0
        for name, shp in spec:
            n = math.prod(shp)
            out[name] = buf[off:off + n].view(shp)
            off += n
        return out

    def _views(self):
        vc, flat = self._view_cache, self._flat
        if vc is not None and flat is not None and vc[0] is flat and \
                self.seq_encoder[0].weight.data.data_ptr() == flat.data_ptr() and \
                self.decoder_mean[0].bias.data.data_ptr() == flat.data_ptr() + 4 * (flat.numel() - self.obs_dim):
            return vc[1]
        flat = self.flatten_parameters()
        L.require_cuda(flat)
        v = self._segment_views(flat[:self._n_enc], "enc")
        v.update(self._segment_views(flat[self._n_enc:], "dec"))
        self._view_cache = (flat, v)
        return v

    def _enc_weights(self):
        se = self.seq_encoder
        return (se[0].weight, se[0].bias, se[2].weight, se[2].bias, se[4].weight, se[4].bias)

    def _dec_weights(self):
        return tuple(self.trainable()[6:])

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
        return FlowEncoderFn.apply(self, xf, mf, _f32c(eps), *self._enc_weights())

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
        x_mean = FlowDecoderFn.apply(self, z_int, *self._dec_weights())
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
    regularised = True

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
class FlowTrainer(_FlatAdamTrainer):
    """The whole training step of the flow path (train.py:77-86 + :114-116) as a fixed sequence of HIP launches with no
    host synchronisation: mask_p draw + stacked encoder input + eps draws (one launch), the encoder GEMMs with the q and
    p passes stacked along the batch (one GEMM per layer), the flow, the five decoder GEMMs, the loss (two launches, the
    gradients gated through Sigmoid'), the backward GEMM chain with the flow backward between decoder and encoder, the
    eight weight gradients summed by one launch, flat Adam.  fp32 only; 30 launches.

    Single process only: the reference's torch.any(inside) (VAE.py:1698) is a predicate over the whole batch of an
    encoder call, so a sharded step would need a cross-rank vote before the flow."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, process_group=None, world_size=1, rank=0):
        if not isinstance(model, _FlowBase):
            raise TypeError("FlowTrainer supports VAEFlow and REG_VAEFlow")
        if world_size != 1:
            raise L.VpcError("FlowTrainer is single-process: the flow's torch.any(inside) is a predicate over the whole "
                             "batch (no data-parallel form without a cross-rank vote)")
        super().__init__(model, lr, betas, eps, seed, process_group, world_size, rank, 1)
        self.reg = model.regularised
        self.out8 = torch.zeros(8, dtype=torch.float64, device=self.dev)
        self.g = model._segment_views(self.grad[:model._n_enc], "enc")
        self.g.update(model._segment_views(self.grad[model._n_enc:], "dec"))
        self._B = None

    def _ws(self, B):
        if self._B == B:
            return
        m, dev = self.model, self.dev
        d, H = m.obs_dim, m.hid_dim
        P = 2 if self.reg else 1
        R = P * B
        e = lambda *s: torch.empty(*s, device=dev)
        self.xin, self.mask_p, self.eps = e(R, 2 * d), e(B, d), e(R, FLOW_L)
        self.h1, self.h2, self.t = e(R, H), e(R, H), e(R, CTX)
        self.z, self.zlp = e(R, FLOW_L), e(R, FLOW_L)
        self.gd = [e(R, H) for _ in range(4)]
        self.Y, self.G = e(R, d), e(R, d)
        self.gz, self.gzlp, self.dzd = e(R, FLOW_L), e(R, FLOW_L), e(R, FLOW_L)
        self.dgd = [e(R, H) for _ in range(4)]
        self.dt, self.dh2, self.dh1 = e(R, CTX), e(R, H), e(R, H)
        self.wg_shapes = [(R, d, H), (R, H, H), (R, H, H), (R, H, H), (R, H, FLOW_L), (R, CTX, H), (R, H, H),
                          (R, H, 2 * d)]
        sizes = [int(lib().vpc_linear_wgrad_scratch(*sh)) for sh in self.wg_shapes]
        buf = e(sum(sizes))
        self.wg_scratch, o = [], 0
        for n in sizes:
            self.wg_scratch.append(buf[o:o + n])
            o += n
        self._wg_cache = {}
        self.scratch = flow_loss_scratch(B, dev)
        pq = lambda a: (a[:B], a[B:] if self.reg else None)
        self._sl = dict(xm=pq(self.Y), z=pq(self.z), zlp=pq(self.zlp),
                        g=(*pq(self.G), *pq(self.gz), *pq(self.gzlp)))
        self._B = B

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
        self._ws(B)
        reg = self.reg
        R = (2 if reg else 1) * B
        t, sl, g = self._timed, self._sl, self.g
        mp_in = _mask_f32(mask_p, d, xf.device) if (reg and mask_p is not None) else None
        mp = mp_in if mp_in is not None else (self.mask_p if reg else None)
        t("prep", flow_prep, xf, mf, mp_in, self.mask_p if (reg and mp_in is None) else None, self.xin,
          self.eps if eps is None else None, B, d, 1.0 - p_missingness / 100.0, self.seed, self.rng_offset,
          self.rng_offset + (1 << 40))
        if eps is not None:
            self.eps.copy_(eps.reshape(self.eps.shape))
        self.rng_offset += (self.eps.numel() + 3) // 4 + (B * d + 3) // 4 + 1
        # ---- forward
        t("enc_fwd", linear_fwd, self.xin, v["We1"], v["be1"], self.h1, R, H, 2 * d, ACT_ELU)
        t("enc_fwd", linear_fwd, self.h1, v["We2"], v["be2"], self.h2, R, H, H, ACT_ELU)
        t("enc_fwd", linear_fwd, self.h2, v["We3"], v["be3"], self.t, R, CTX, H, ACT_NONE)
        t("flow", flow_fwd, self.t, self.eps, self.z, self.zlp, R, B)
        gd, dgd = self.gd, self.dgd
        t("dec_fwd", linear_fwd, self.z, v["Wd1"], v["bd1"], gd[0], R, H, FLOW_L, ACT_ELU)
        for i in range(1, 4):
            t("dec_fwd", linear_fwd, gd[i - 1], v[f"Wd{i + 1}"], v[f"bd{i + 1}"], gd[i], R, H, H, ACT_ELU)
        t("dec_fwd", linear_fwd, gd[3], v["Wm"], v["bm"], self.Y, R, d, H, ACT_SIGMOID_HARDTANH, d)
        # ---- loss: G = d train_loss / d decoder_mean pre-activation, gz / gzlp = d train_loss / d (z, z_log_prob)
        t("loss", flow_loss, xf, mf, mp, sl["xm"], sl["z"], sl["zlp"], sl["g"], self.scratch, self.out8, self.tail,
          self.accum, B, d, STAGE_TRAIN if stage == "train" else STAGE_EVAL, alpha, beta, 1.0 / B, 1)
        # ---- backward: weight-gradient partials per layer, all summed by one launch
        defer = self.timers is None
        pend = []

        def wgrad(name, i, dy, xx, dw, db):
            Mi, Ni, Ki = self.wg_shapes[i]
            if not defer:
                return t(name, linear_wgrad, dy, xx, dw, db, Mi, Ni, Ki)
            linear_wgrad(dy, xx, None, None, Mi, Ni, Ki, scratch=self.wg_scratch[i])
            pend.append((self.wg_scratch[i], Mi, Ni, Ki, dw, db, False))

        wgrad("dec_bwd", 0, self.G, gd[3], g["Wm"], g["bm"])
        t("dec_bwd", linear_dgrad, self.G, v["Wm"], dgd[3], R, d, H, x_out=gd[3], act_prev=ACT_ELU)
        for i in range(3, 0, -1):
            wgrad("dec_bwd", 4 - i, dgd[i], gd[i - 1], g[f"Wd{i + 1}"], g[f"bd{i + 1}"])
            t("dec_bwd", linear_dgrad, dgd[i], v[f"Wd{i + 1}"], dgd[i - 1], R, H, H, x_out=gd[i - 1], act_prev=ACT_ELU)
        wgrad("dec_bwd", 4, dgd[0], self.z, g["Wd1"], g["bd1"])
        t("dec_bwd", linear_dgrad, dgd[0], v["Wd1"], self.dzd, R, H, FLOW_L)
        t("flow_bwd", flow_bwd, self.t, self.eps, self.dzd, self.gz, self.gzlp, self.dt, R, B)
        wgrad("enc_bwd", 5, self.dt, self.h2, g["We3"], g["be3"])
        t("enc_bwd", linear_dgrad, self.dt, v["We3"], self.dh2, R, CTX, H, x_out=self.h2, act_prev=ACT_ELU)
        wgrad("enc_bwd", 6, self.dh2, self.h1, g["We2"], g["be2"])
        t("enc_bwd", linear_dgrad, self.dh2, v["We2"], self.dh1, R, H, H, x_out=self.h1, act_prev=ACT_ELU)
        wgrad("enc_bwd", 7, self.dh1, self.xin, g["We1"], g["be1"])
        if pend:
            wgrad_reduce(pend, self._wg_cache)
        self.step_count += 1
        from .ops import adam_step
        t("adam", adam_step, m._flat, self.grad, self.exp_avg, self.exp_avg_sq, self.step_count, self.lr, self.betas[0],
          self.betas[1], self.adam_eps)
        self._flat_written(None)
