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
`EDDIMnistTrainer` is the training step (train.py:28-117 with data_type == 'mnist') as one fixed launch sequence.  Front-end
wrappers, the Family record of the API path and the constructor prologue are eddi.py's (front_ops("eddiw"), pointnet_family,
_PointNet); this module states the widths, the chains, the limits and the step.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import ops
from ._lib import lib
from .chainfamily import ChainDecoderFn, nm_sample, nm_sample_bwd
from .eddi import _FRONT_SPEC, _PointNet, front_ops, param_chains, pointnet_family
from .images import mlp_spec
from .linear import ACT_NONE, ACT_RELU, ACT_SIGMOID_HARDTANH, chain, chain_bwd, chain_fwd
from .models import Reg_VAE, vanilla_VAE
from .ops import as_mask_u8
from .trainer import _FlatAdamTrainer, draw_counters

H1, H2, H3 = 500, 500, 200  # VAE.py:32-44 hard-codes the widths: trunk K-500-500-200-2L, decoder L-200-500-500-d
MAX_D, MAX_K, MAX_L = 1024, 32, 15

_TRUNK_NAMES = ("We1", "be1", "We2", "be2", "We3", "be3", "We4", "be4")
_DEC_NAMES = ("Wd1", "bd1", "Wd2", "bd2", "Wd3", "bd3", "Wd4", "bd4")

eddiw_fold, eddiw_front_fwd, eddiw_front_bwd = front_ops("eddiw")
# the decoder returns xhat, one [M, d] buffer behind the chain's Sigmoid gate (VAE.py:86-90)
FAMILY = pointnet_family((eddiw_fold, eddiw_front_fwd, eddiw_front_bwd), _TRUNK_NAMES, _DEC_NAMES)


class _EDDIMnistBase(_PointNet):
    """Shared construction / parameter plumbing; mixed in BEFORE Reg_VAE / vanilla_VAE, whose loss() (the K4 kernel behind
    it) and flat-parameter plumbing are reused unchanged."""
    _wide = False
    _eddi_mnist = True  # active.reward_matrix refuses these classes (d = 784 active learning is not a reference configuration)
    family = FAMILY
    _kernels, _limits = "image-width EDDI", (MAX_D, MAX_L, MAX_K)
    _trunk_hidden, _dec_hidden = (H1, H2, H3), (H3, H2, H1)
    # the 20 trainable tensors in state_dict (= flat) order: front-end (4) | trunk (8) | decoder (8)
    _flat_spec = _FRONT_SPEC + mlp_spec(_TRUNK_NAMES, "pnp_encoder2", "enc") + mlp_spec(_DEC_NAMES, "seq_decoder", "dec")

    @staticmethod
    def _build_chains(v):
        """(trunk, decoder) chains on the named views v: pnp_encoder2.{0,2,4,6} = K-500-500-200-2L with ReLU between layers,
        seq_decoder L-200-500-500-d with a Sigmoid on every output (split = d)."""
        return (chain([v[k] for k in _TRUNK_NAMES], (ACT_RELU, ACT_RELU, ACT_RELU, ACT_NONE)),
                chain([v[k] for k in _DEC_NAMES], (ACT_RELU, ACT_RELU, ACT_RELU, ACT_SIGMOID_HARDTANH), v["Wd4"].shape[0]))

    def _images(self, key=None):  # no packed weight images: every layer reads the flat parameters
        return None

    def decoder(self, z_int):
        """VAE.py:86-90: returns (x_mean, x_logvar) with x_logvar the shape-(1,) constant log 0.02."""
        L.require_cuda(z_int)
        return ChainDecoderFn.apply(FAMILY, self, z_int, *self._dec_weights()), self.x_logvar


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
        g = self.g
        self.trunk, self.dec_layers = param_chains(m)
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
