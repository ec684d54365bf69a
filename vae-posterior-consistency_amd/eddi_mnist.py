"""The MNIST point-net pair: drop-in classes for the reference's

    Reg_EDDI_mnist       src/models/VAE.py:10-201
    vanilla_EDDI_mnist   src/models/VAE.py:204-347

which `model_loader` builds when an '*_EDDI*' vae_type meets data_type == 'mnist' (loaders.py:104-131, 185-218).  Same
constructor arguments, attributes, module construction order (same seed -> same initial weights), `encoder` / `decoder` /
`forward` / `loss` signatures and return order, and state_dict keys in the reference's order:

    type_pars1, type_bias1, prior_mean, prior_std, pnp_encoder1.0.*, pnp_encoder2.{0,2,4,6}.*, seq_decoder.{0,2,4,6}.*

The encoder is the point-net front-end at image width (vpc_eddiw_* of csrc/vpc_eddi.hip: folded per-feature affine + ReLU + mask-weighted
sum over the d features, nothing of size B*d*(2+K) materialised) followed by the trunk K -> 500 -> 500 -> 200 -> 2L; the
decoder is L -> 200 -> 500 -> 500 -> d with a Sigmoid.  The seven wide layers and the two narrow ones run on the generic fp32
MFMA GEMMs (csrc/vpc_gemm.hip); the loss is the width-independent fused loss kernel K4 (vpc_loss_fwd_bwd), which has the
reference's terms unchanged at d = 784: every entry contributes 0.5 log 2 pi, masked or not (the reference multiplies target,
mean AND log-variance by the mask, so a masked entry is -log N(0; 0, 1)), the kl_reg extra term is the NLL on
mask & ~mask_p, and the sum is divided by the batch size.  No CPU fallback.

Limits (VpcError): obs_dim <= 1024, K (emb_dim) <= 32, latent_dim <= 15.

Reference behaviour that is reproduced, not fixed:
  * inputs of any leading shape are reshaped to [-1, obs_dim] by `forward` and `loss` (VAE.py:97-99, 188-190, 288-289, 343-344):
    MNIST batches may arrive as [B, 28, 28] or [B, 1, 28, 28];
  * `encoder` returns three EMPTY CPU tensors of shape (0, 10) - ten columns whatever latent_dim is - when the mask has no
    rows (VAE.py:66-67, 259-260);
  * Reg_EDDI_mnist.loss needs BOOL masks (`~mask`, `~mask_p`, VAE.py:106, 141) and returns RE_q_imputed = 0 in the train
    stage (VAE.py:148); vanilla_EDDI_mnist.loss takes bool or float masks (`1 - mask * 1.0`, VAE.py:294), has no `stage`
    dependence at all and computes RE_q_imputed on the UNobserved entries in EVERY call (VAE.py:294-295) - it is not
    Reg_EDDI_mnist minus the p pass;
  * vanilla_EDDI_mnist.forward takes no `stage` (VAE.py:342); vanilla_EDDI_mnist.loss has no `alpha_annealing`;
  * an unknown reg_type prints 'Not implemented!' (VAE.py:145-147); here it then raises instead of failing in backward.
`EDDIMnistTrainer` is the training step (train.py:28-117 with data_type == 'mnist') as one fixed launch sequence.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from ._lib import check, lib, ptr, require_cuda, stream_ptr
from .chainfamily import nm_sample, nm_sample_bwd
from .images import mlp_spec
from .linear import ACT_NONE, ACT_RELU, ACT_SIGMOID_HARDTANH, chain, chain_buffers, chain_bwd, chain_fwd, wgrad_now
from .models import MAX_EPOCH, Reg_VAE, vanilla_VAE
from .ops import as_mask_u8
from .trainer import _FlatAdamTrainer, draw_counters

H1, H2, H3 = 500, 500, 200  # VAE.py:32-44 hard-codes the widths: trunk K-500-500-200-2L, decoder L-200-500-500-d
MAX_D, MAX_K, MAX_L = 1024, 32, 15

_TRUNK_NAMES = ("We1", "be1", "We2", "be2", "We3", "be3", "We4", "be4")
_DEC_NAMES = ("Wd1", "bd1", "Wd2", "bd2", "Wd3", "bd3", "Wd4", "bd4")


def eddiw_fold(E, tb, Wp, cp, AC, d, K):
    check(lib().vpc_eddiw_fold(ptr(E), ptr(tb), ptr(Wp), ptr(cp), ptr(AC), d, K, stream_ptr()), "vpc_eddiw_fold")


def eddiw_front_fwd(x, mask_u8, AC, agg, B, d, K, mask2_u8=None):
    """agg [B][K] (or [2B][K] when a second mask is given: the q and p passes of a step stacked)."""
    check(lib().vpc_eddiw_front_fwd(ptr(x), ptr(mask_u8), ptr(mask2_u8), ptr(AC), ptr(agg), B, d, K, stream_ptr()),
          "vpc_eddiw_front_fwd")


def eddiw_front_bwd(x, mask_u8, AC, dagg, E, tb, Wp, gE, gtb, gWp, gcp, B, d, K, accumulate=False, mask2_u8=None,
                    scratch=None):
    rows = B * (2 if mask2_u8 is not None else 1)
    need = int(lib().vpc_eddiw_front_scratch(rows, d, K))
    sc = scratch if scratch is not None and scratch.numel() >= need else torch.empty(need, device=x.device)
    check(lib().vpc_eddiw_front_bwd(ptr(x), ptr(mask_u8), ptr(mask2_u8), ptr(AC), ptr(dagg), ptr(E), ptr(tb), ptr(Wp),
                                    ptr(sc), sc.numel(), ptr(gE), ptr(gtb), ptr(gWp), ptr(gcp), int(accumulate), B, d, K,
                                    stream_ptr()), "vpc_eddiw_front_bwd")


def _chains(trunk, dec):
    """(trunk, decoder) chains on [W1, b1, ..]: pnp_encoder2.{0,2,4,6} = K-500-500-200-2L with ReLU between layers, seq_decoder
    L-200-500-500-d with a Sigmoid on every output (split = d)."""
    return (chain(trunk, (ACT_RELU, ACT_RELU, ACT_RELU, ACT_NONE)),
            chain(dec, (ACT_RELU, ACT_RELU, ACT_RELU, ACT_SIGMOID_HARDTANH), dec[6].shape[0]))


def _fresh_grads(layers, M, device):
    """New (dw, db) per layer as wgrad_now keys, and the flat list [dw1, db1, dw2, ..] an autograd backward returns."""
    keys = [(torch.empty(l[3], l[2], device=device), torch.empty(l[3], device=device), M, l[3], l[2]) for l in layers]
    return keys, [t for k in keys for t in k[:2]]


class EDDIMnistEncoderFn(torch.autograd.Function):
    """(x, mask, eps) -> (z, mean, logvar).  Reference: VAE.py:62-84 / 255-277."""

    @staticmethod
    def forward(ctx, model, x, mask_u8, eps, E, tb, Wp, cp, *trunk):
        require_cuda(x, mask_u8, eps, E, trunk[0])
        d, Ld, K = model.obs_dim, model.latent_dim, model.emb_dim
        B, dev = x.shape[0], x.device
        AC = torch.empty(2, K, d, device=dev)
        eddiw_fold(E, tb, Wp, cp, AC, d, K)
        layers = model._chains()[0]
        acts = chain_buffers(layers, B, dev)
        eddiw_front_fwd(x, mask_u8, AC, acts[0], B, d, K)
        chain_fwd(layers, acts, B)
        heads = acts[-1]
        z = torch.empty(B, Ld, device=dev)
        nm_sample(heads, eps, z, B, 1, Ld)  # z = mean + eps * exp(logvar / 2); eps None -> z = mean
        ctx.model = model
        ctx.has_eps = eps is not None
        ctx.save_for_backward(x, mask_u8, AC, *acts, eps if eps is not None else torch.empty(0, device=dev), E, tb, Wp)
        return z, heads[:, :Ld], heads[:, Ld:]

    @staticmethod
    def backward(ctx, dz, dmean, dlogvar):
        model = ctx.model
        x, mask_u8, AC, agg, h1, h2, h3, heads, eps, E, tb, Wp = ctx.saved_tensors
        eps = eps if ctx.has_eps else None
        d, Ld, K = model.obs_dim, model.latent_dim, model.emb_dim
        B, dev = x.shape[0], x.device
        e = lambda *s: torch.empty(*s, device=dev)
        gh = torch.zeros(B, 2 * Ld, device=dev)
        if dmean is not None:
            gh[:, :Ld] += dmean
        if dlogvar is not None:
            gh[:, Ld:] += dlogvar
        layers = model._chains()[0]
        dacts = chain_buffers(layers, B, dev)
        dzc = ops._f32c(dz) if dz is not None else torch.zeros(B, Ld, device=dev)
        nm_sample_bwd(dzc, eps, heads, gh, dacts[-1], B, 1, Ld)
        keys, grads = _fresh_grads(layers, B, dev)
        chain_bwd(layers, [agg, h1, h2, h3], dacts, B, wgrad_now, keys)  # (agg is a sum of ReLUs, not a ReLU output: no gate)
        gE, gtb, gWp, gcp = e(d, K), e(d, 1), e(K, 2 + K), e(K)
        eddiw_front_bwd(x, mask_u8, AC, dacts[0], E, tb, Wp, gE, gtb, gWp, gcp, B, d, K)
        return (None, None, None, None, gE, gtb, gWp, gcp, *grads)


class EDDIMnistDecoderFn(torch.autograd.Function):
    """(z, 8 decoder tensors) -> xhat = sigmoid(MLP(z)).  VAE.py:86-90."""

    @staticmethod
    def forward(ctx, model, z, *w):
        require_cuda(z, w[0])
        z = ops._f32c(z)
        B = z.shape[0]
        layers = model._chains()[1]
        acts = chain_buffers(layers, B, z.device, first=z)
        chain_fwd(layers, acts, B)
        ctx.model = model
        ctx.save_for_backward(*acts)
        return acts[-1]

    @staticmethod
    def backward(ctx, dxhat):
        z, g1, g2, g3, xhat = ctx.saved_tensors
        B, dev, d = z.shape[0], z.device, xhat.shape[1]
        layers = ctx.model._chains()[1]
        dacts = chain_buffers(layers, B, dev, last=ops._f32c(dxhat))
        keys, grads = _fresh_grads(layers, B, dev)
        chain_bwd(layers, [z, g1, g2, g3], dacts, B, wgrad_now, keys, y_gate=xhat, gate=ACT_SIGMOID_HARDTANH,
                  gate_split=d)  # dpre = dxhat xhat (1 - xhat)
        return (None, dacts[0], *grads)


class _EDDIMnistBase:
    """Shared construction / parameter plumbing; mixed in BEFORE Reg_VAE / vanilla_VAE, whose loss() (the K4 kernel behind
    it) and flat-parameter plumbing are reused unchanged."""
    _wide = False
    _eddi_mnist = True  # active.reward_matrix refuses these classes (d = 784 active learning is not a reference configuration)
    # the 20 trainable tensors in state_dict (= flat) order: front-end (4) | trunk (8) | decoder (8)
    _flat_spec = (("E", "type_pars1", "front"), ("tb", "type_bias1", "front")) + \
        mlp_spec(("Wp", "cp"), "pnp_encoder1", "front") + \
        mlp_spec(_TRUNK_NAMES, "pnp_encoder2", "enc") + mlp_spec(_DEC_NAMES, "seq_decoder", "dec")

    @staticmethod
    def _build_chains(v):
        return _chains([v[k] for k in _TRUNK_NAMES], [v[k] for k in _DEC_NAMES])

    def _build(self, obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, num_samples, num_estimates):
        nn.Module.__init__(self)
        if obs_dim > MAX_D or latent_dim > MAX_L or K > MAX_K:
            raise L.VpcError(f"the gfx950 image-width EDDI kernels support obs_dim <= {MAX_D}, K (emb_dim) <= {MAX_K} and "
                             f"latent_dim <= {MAX_L}")
        self.obs_dim, self.hid_dim, self.emb_dim, self.latent_dim = obs_dim, hid_dim, K, latent_dim
        self.K = K
        self.batch_size = training_parameters["batch_size"]
        self.training_parameters = training_parameters
        self.experiment_type = experiment_type
        self.num_samples, self.num_estimates = num_samples, num_estimates

    def _build_modules(self):
        # containers in the reference's construction order (same seed -> same initial weights), VAE.py:27-56
        K, latent_dim, obs_dim = self.emb_dim, self.latent_dim, self.obs_dim
        self.pnp_encoder1 = nn.Sequential(nn.Linear(2 + K, K), nn.ReLU())
        self.pnp_encoder2 = nn.Sequential(nn.Linear(K, H1), nn.ReLU(), nn.Linear(H1, H2), nn.ReLU(), nn.Linear(H2, H3),
                                          nn.ReLU(), nn.Linear(H3, 2 * latent_dim))
        self.seq_decoder = nn.Sequential(nn.Linear(latent_dim, H3), nn.ReLU(), nn.Linear(H3, H2), nn.ReLU(),
                                         nn.Linear(H2, H1), nn.ReLU(), nn.Linear(H1, obs_dim), nn.Sigmoid())
        xlv = torch.log(torch.square(torch.Tensor([0.1 * np.sqrt(2)])))  # log 0.02, shape (1,)
        self.register_buffer("x_logvar", xlv, persistent=False)
        self._x_logvar_value = float(xlv.item())
        self.type_pars1 = nn.Parameter(torch.zeros(obs_dim, K), requires_grad=True)
        nn.init.xavier_uniform_(self.type_pars1)
        self.type_bias1 = nn.Parameter(torch.zeros(obs_dim, 1), requires_grad=True)
        nn.init.xavier_uniform_(self.type_bias1)
        self.prior_mean = nn.Parameter(torch.zeros(latent_dim), requires_grad=False)
        self.prior_std = nn.Parameter(torch.ones(latent_dim), requires_grad=False)
        self.max_epoch = MAX_EPOCH
        self._layout = None
        self._img = None
        self._part = {}

    def _images(self, key=None):  # no packed weight images: every layer reads the flat parameters
        return None

    def decoder(self, z_int):
        """VAE.py:86-90: returns (x_mean, x_logvar) with x_logvar the shape-(1,) constant log 0.02."""
        L.require_cuda(z_int)
        self.flatten_parameters()
        return EDDIMnistDecoderFn.apply(self, z_int, *self.trainable()[12:]), self.x_logvar

    def encoder(self, x, mask, sample=True):
        """VAE.py:62-84 / 255-277: returns (z, mean, logvar)."""
        L.require_cuda(x)
        if mask.shape[0] == 0:  # VAE.py:66-67
            return torch.empty(0, 10), torch.empty(0, 10), torch.empty(0, 10)
        self.flatten_parameters()
        xf = ops._f32c(x.reshape(-1, self.obs_dim))
        m = as_mask_u8(mask.reshape(-1, self.obs_dim).to(x.device))
        eps = torch.randn(xf.shape[0], self.latent_dim, device=xf.device) if sample else None
        return EDDIMnistEncoderFn.apply(self, xf, m, eps, *self.trainable()[:12])


class Reg_EDDI_mnist(_EDDIMnistBase, Reg_VAE):
    """Reference: src/models/VAE.py:10-201."""

    def __init__(self, obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, reg_type, num_samples=1,
                 num_estimates=1):
        self._build(obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, num_samples, num_estimates)
        self.reg_type = reg_type  # VAE.py:26: set before the modules
        self._build_modules()

    def forward(self, data, mask, mask_p, stage="train"):
        """VAE.py:187-201: q pass, then p pass (both stages alike); the p outputs are returned first."""
        d = self.obs_dim
        data, mask, mask_p = data.reshape(-1, d), mask.reshape(-1, d), mask_p.reshape(-1, d)
        z_q, mean_q, logvar_q = self.encoder(data, mask)
        x_mean_q, x_logvar_q = self.decoder(z_q)
        z_p, mean_p, logvar_p = self.encoder(data, mask_p)
        x_mean_p, x_logvar_p = self.decoder(z_p)
        return mean_p, logvar_p, x_mean_p, x_logvar_p, mean_q, logvar_q, x_mean_q, x_logvar_q

    def loss(self, x, x_recon_p, x_logvar_p, mean_p, logvar_p, x_recon_q, x_logvar_q, mean_q, logvar_q, mask, mask_p,
             epoch, vae_elbo=False, llh_eval=False, MI=False, beta_annealing=False, beta=1.0, alpha=0.5, stage="train",
             alpha_annealing=False):
        """VAE.py:92-162: Reg_VAE.loss on the reshaped inputs, with this class's defaults."""
        d = self.obs_dim
        return Reg_VAE.loss(self, x.reshape(-1, d), x_recon_p, x_logvar_p, mean_p, logvar_p, x_recon_q, x_logvar_q, mean_q,
                            logvar_q, mask.reshape(-1, d), mask_p.reshape(-1, d), epoch, vae_elbo, llh_eval, MI,
                            beta_annealing, beta, alpha, stage, alpha_annealing)


class vanilla_EDDI_mnist(_EDDIMnistBase, vanilla_VAE):
    """Reference: src/models/VAE.py:204-347."""

    def __init__(self, obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, num_samples=1,
                 num_estimates=1):
        self._build(obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, num_samples, num_estimates)
        self._build_modules()

    def forward(self, data, mask):
        """VAE.py:342-347."""
        d = self.obs_dim
        z_q, mean_q, logvar_q = self.encoder(data.reshape(-1, d), mask.reshape(-1, d))
        x_mean_q, x_logvar_q = self.decoder(z_q)
        return mean_q, logvar_q, x_mean_q, x_logvar_q

    def loss(self, x, x_recon_q, x_logvar_q, mean_q, logvar_q, epoch, mask, vae_elbo=False, llh_eval=False, MI=False,
             beta_annealing=False, beta=1.0, alpha=0.5, stage="train"):
        """VAE.py:285-317: vanilla_VAE.loss, except that RE_q_imputed is computed in EVERY call (:294-295) - `stage` is
        accepted and ignored, as in the reference."""
        d = self.obs_dim
        return vanilla_VAE.loss(self, x.reshape(-1, d), x_recon_q, x_logvar_q, mean_q, logvar_q, epoch, mask.reshape(-1, d),
                                vae_elbo, llh_eval, MI, beta_annealing, beta, alpha, True, "evaluate")


# ------------------------------------------------------------------------------------------------ fused step
_TRUNK_WKEYS, _DEC_WKEYS = tuple((None, i) for i in range(4)), tuple((None, 4 + i) for i in range(4))  # (no timer, workspace index)


class EDDIMnistTrainer(_FlatAdamTrainer):
    """The training step of train.py:28-117 for data_type == 'mnist' as a fixed launch sequence without host synchronisation:
    mask_p + eps draws -> fold -> front-end (q and p passes stacked, one launch) -> the four trunk GEMMs on the stacked passes
    -> rsample -> the four decoder GEMMs -> loss with its gradient seeds (K4) -> decoder and trunk backward GEMMs, every
    weight gradient left as partials and summed by ONE launch -> front-end backward -> flat Adam over the one parameter
    buffer (state_dict order).  The reference draws mask_p row by row from numpy's host RNG (train.py:39-45); only its
    distribution mask & Bernoulli(1 - p / 100) is reproducible, and one device draw over the batch has it.
    Single device: world_size > 1 is refused (VpcError); data parallelism for this model is not built yet."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, process_group=None, world_size=1, rank=0):
        if not isinstance(model, _EDDIMnistBase):
            raise TypeError("EDDIMnistTrainer supports Reg_EDDI_mnist and vanilla_EDDI_mnist")
        if world_size != 1:
            raise L.VpcError("EDDIMnistTrainer runs on one device: world_size > 1 is not supported for Reg_EDDI_mnist / "
                             "vanilla_EDDI_mnist")
        super().__init__(model, lr, betas, eps, seed, process_group, world_size, rank, 9)
        self.vanilla = isinstance(model, vanilla_VAE)
        self.out9 = self.tail
        self.loss_part = torch.empty(L.num_cus() * 8, 8, dtype=torch.float64, device=self.dev)
        self.g = [p.grad for p in self._plist]  # gradient views in flat order: front-end (4) | trunk (8) | decoder (8)
        self._B = None

    def _ws(self, B):
        if self._B == B:
            return
        m, dev = self.model, self.dev
        d, Ld, K = m.obs_dim, m.latent_dim, m.emb_dim
        P = 1 if self.vanilla else 2
        R = P * B
        e = lambda *s: torch.empty(*s, device=dev)
        self.AC = e(2, K, d)
        self.enc = [e(R, K), e(R, H1), e(R, H2), e(R, H3), e(R, 2 * Ld)]       # agg, h1, h2, h3, heads
        self.denc = [e(R, K), e(R, H1), e(R, H2), e(R, H3), e(R, 2 * Ld)]      # dagg, dh1, dh2, dh3, dht
        self.dec = [e(R, Ld), e(R, H3), e(R, H2), e(R, H1), e(R, d)]           # z, g1, g2, g3, xhat
        self.ddec = [e(R, Ld), e(R, H3), e(R, H2), e(R, H1), e(R, d)]          # dz, dg1, dg2, dg3, dxhat
        self.lat, self.dlat = e(P, 2, B, Ld), e(P, 2, B, Ld)                   # [pass][mean | logvar][B][L]
        self.gh = e(R, 2 * Ld)
        self.LP = 4 * ((Ld + 3) // 4)
        self.eps_pad = e(3, B, self.LP)                                        # Philox fills whole groups of 4
        self.eps = e(R, Ld)
        self.eps_ml = e(B, Ld)
        self.mask_p_buf = torch.empty(B, d, dtype=torch.uint8, device=dev)
        self.front_scratch = e(int(lib().vpc_eddiw_front_scratch(R, d, K)))
        # the two GEMM chains, and the per-layer partial buffers of their eight weight gradients: summed by ONE launch
        t, g = self._plist, self.g
        self.trunk, self.dec_layers = _chains(t[4:12], t[12:20])
        self._wgrad_workspace([(R, l[3], l[2]) for l in self.trunk + self.dec_layers],
                              [(g[4 + 2 * i], g[5 + 2 * i]) for i in range(8)])
        self._sl = dict(mean=[self.lat[p_, 0] for p_ in range(P)], logvar=[self.lat[p_, 1] for p_ in range(P)],
                        dmean=[self.dlat[p_, 0] for p_ in range(P)], dlogvar=[self.dlat[p_, 1] for p_ in range(P)],
                        heads_src=self.enc[4].view(P, B, 2, Ld).permute(0, 2, 1, 3), gh_dst=self.gh.view(P, B, 2, Ld),
                        dlat_src=self.dlat.permute(0, 2, 1, 3), xhat=[self.dec[4][p_ * B:(p_ + 1) * B] for p_ in range(P)],
                        dxhat=[self.ddec[4][p_ * B:(p_ + 1) * B] for p_ in range(P)],
                        eps_dst=self.eps.view(P, B, Ld), eps_src=self.eps_pad[:P, :, :Ld], eml_src=self.eps_pad[2, :, :Ld])
        self._B = B

    def step(self, x, mask, mask_p=None, eps=None, *, epoch=1, alpha=0.5, beta=1.0, beta_annealing=False,
             p_missingness=30, eps_ml=None):
        """x [B, ...] (reshaped to [B, obs_dim]), mask likewise.  Injectable for parity tests: mask_p [B, obs_dim], eps
        [P, B, L] (the rsample draws of the q and p passes; P = 1 for the vanilla class) and eps_ml [B, L] (ml_reg's third
        draw); left None they are drawn on the device (Philox, seed / counter of this trainer)."""
        m = self.model
        d, Ld, K = m.obs_dim, m.latent_dim, m.emb_dim
        x = ops._f32c(x.reshape(-1, d))
        L.require_cuda(x)
        mask = as_mask_u8(mask.reshape(-1, d))
        L.require_cuda(mask)
        B = x.shape[0]
        self._ws(B)
        co = self.coefficients(epoch, alpha, beta, beta_annealing)
        two = not self.vanilla
        P = 2 if two else 1
        R = P * B
        sl = self._sl
        t = self._plist
        E, tb, Wp, cp = t[:4]
        # ---- draws
        need_ml = two and co.ml_on
        # (always all three planes of eps_pad, whatever the step consumes)
        draw_mask, draw_eps = two and mask_p is None, eps is None or (need_ml and eps_ml is None)
        dr = draw_counters(self.rng_offset, draw_mask, 3 if draw_eps else 0, B, B, 0, self.LP, d)
        self.rng_offset = dr.next_offset
        if draw_mask:
            ops.draw_mask(mask, self.mask_p_buf, 1.0 - p_missingness / 100.0, self.seed, dr.offset_mask, dr.elem_lo)
            mask_p = self.mask_p_buf
        elif two:
            mask_p = as_mask_u8(mask_p.reshape(-1, d))
        if draw_eps:
            ops.fill_normal(self.eps_pad, self.seed, dr.offset_eps, None, dr.eps_shard)
        if eps is None:
            sl["eps_dst"].copy_(sl["eps_src"])
        else:
            sl["eps_dst"].copy_(eps.reshape(P, B, Ld))
        if need_ml:
            self.eps_ml.copy_(sl["eml_src"] if eps_ml is None else eps_ml)
        masks = [mask, mask_p] if two else [mask]
        # ---- encoder: front-end on both passes in one launch, trunk on the stacked passes
        eddiw_fold(E, tb, Wp, cp, self.AC, d, K)
        eddiw_front_fwd(x, masks[0], self.AC, self.enc[0], B, d, K, masks[1] if two else None)
        chain_fwd(self.trunk, self.enc, R)
        heads = self.enc[4]
        nm_sample(heads, self.eps, self.dec[0], R, 1, Ld)
        # ---- decoder
        chain_fwd(self.dec_layers, self.dec, R)
        # ---- loss + seeds (K4 on the materialised xhat; the statistics as [pass][mean | logvar][B][L])
        self.lat.copy_(sl["heads_src"])
        maskB = [mask_p, None] if (two and co.maskB_on) else [None] * P
        nb = ops.loss_fwd_bwd(x, sl["xhat"], masks, maskB, co, sl["mean"], sl["logvar"], self.eps_ml if need_ml else None,
                              1.0 / B, m._x_logvar_value, sl["dxhat"], sl["dmean"], sl["dlogvar"], self.loss_part, d, Ld)
        ops.loss_finalize(self.loss_part, nb, co, B, B, d, self.out9, self.accum)
        # ---- decoder backward (weight gradients stay partials until the one reduce launch)
        chain_bwd(self.dec_layers, self.dec, self.ddec, R, self._wgrad, _DEC_WKEYS, y_gate=self.dec[4],
                  gate=ACT_SIGMOID_HARDTANH, gate_split=d)
        # ---- rsample backward: d heads = K4's seeds + the path through z
        sl["gh_dst"].copy_(sl["dlat_src"])
        nm_sample_bwd(self.ddec[0], self.eps, heads, self.gh, self.denc[4], R, 1, Ld)
        # ---- trunk backward
        chain_bwd(self.trunk, self.enc, self.denc, R, self._wgrad, _TRUNK_WKEYS)
        self._wgrad_reduce()
        g = self.g
        eddiw_front_bwd(x, masks[0], self.AC, self.denc[0], E, tb, Wp, g[0], g[1], g[2], g[3], B, d, K,
                        mask2_u8=masks[1] if two else None, scratch=self.front_scratch)
        self._adam()
