"""PNP / EDDI encoder family: drop-in classes for the reference's

    Reg_EDDI       src/models/VAE.py:670-853
    vanilla_EDDI   src/models/VAE.py:856-992

Same constructor arguments, `encoder` / `decoder` / `forward` / `loss` signatures, return order and state_dict keys
(type_pars1, type_bias1, prior_mean, prior_std, pnp_encoder1.0, pnp_encoder2.{0,2,4}, seq_decoder.{0,2,4}).  Decoder
and loss are those of Reg_VAE / vanilla_VAE (same HIP kernels, inherited); the encoder is the point-net front-end
(csrc/vpc_eddi.hip: folded per-feature affine + ReLU + mask-weighted sum, nothing of size B*d*(2+K) materialised)
followed by pnp_encoder2 as three fp32 MFMA GEMMs (csrc/vpc_gemm.hip).  No CPU fallback.

On the API path the encoder is chainfamily.ChainEncoderFn with the point-net Family record (the front-end is its input op).
Shared with the image-width pair of eddi_mnist.py, and here once: front_ops, pointnet_family and _PointNet.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from ._lib import check, lib, ptr, stream_ptr
from .chainfamily import ChainEncoderFn, Family, gauss_sample, gauss_sample_bwd
from .images import PackedImage, mlp_spec
from .linear import chain_bwd, chain_fwd
from .models import _W6, MAX_EPOCH, Reg_VAE, vanilla_VAE
from .ops import as_mask_u8
from .trainer import _FlatAdamTrainer, draw_counters, pad_cols

H1, H2 = 100, 50  # VAE.py:694-698 hard-codes 100 / 50


# ------------------------------------------------------------------------------------------------ the point-net front-end
def front_ops(prefix):
    """(fold, front_fwd, front_bwd) on the kernels vpc_<prefix>_* of csrc/vpc_eddi.hip: "eddi" the narrow front-end (obs_dim <=
    128), "eddiw" the image-width one.  front_fwd writes agg [B][K], or [2B][K] when a second mask is given: the q and p passes
    of a step stacked."""
    n_fold, n_fwd, n_scratch, n_bwd = (f"vpc_{prefix}_{k}" for k in ("fold", "front_fwd", "front_scratch", "front_bwd"))

    def fold(E, tb, Wp, cp, AC, d, K):
        check(getattr(lib(), n_fold)(ptr(E), ptr(tb), ptr(Wp), ptr(cp), ptr(AC), d, K, stream_ptr()), n_fold)

    def front_fwd(x, mask_u8, AC, agg, B, d, K, mask2_u8=None):
        check(getattr(lib(), n_fwd)(ptr(x), ptr(mask_u8), ptr(mask2_u8), ptr(AC), ptr(agg), B, d, K, stream_ptr()), n_fwd)

    def front_bwd(x, mask_u8, AC, dagg, E, tb, Wp, gE, gtb, gWp, gcp, B, d, K, accumulate=False, mask2_u8=None, scratch=None):
        rows = B * (2 if mask2_u8 is not None else 1)
        need = int(getattr(lib(), n_scratch)(rows, d, K))
        sc = scratch if scratch is not None and scratch.numel() >= need else torch.empty(need, device=x.device)
        check(getattr(lib(), n_bwd)(ptr(x), ptr(mask_u8), ptr(mask2_u8), ptr(AC), ptr(dagg), ptr(E), ptr(tb), ptr(Wp), ptr(sc),
                                    sc.numel(), ptr(gE), ptr(gtb), ptr(gWp), ptr(gcp), int(accumulate), B, d, K, stream_ptr()),
              n_bwd)

    return fold, front_fwd, front_bwd


eddi_fold, eddi_front_fwd, eddi_front_bwd = front_ops("eddi")


def pointnet_family(ops3, enc_names, dec_names):
    """The Family record of a point-net family on `ops3` = front_ops(..): the input op folds the four front-end tensors (E, tb,
    Wp, cp: the last weights of apply()) and writes the aggregate, the trunk's input; its backward takes its gradient to theirs."""
    fold, front_fwd, front_bwd = ops3

    def enc_input(x, mask_u8, agg, B, d, E, tb, Wp, cp):
        K = E.shape[1]
        AC = torch.empty(2, K, d, device=x.device)
        fold(E, tb, Wp, cp, AC, d, K)
        front_fwd(x, mask_u8, AC, agg, B, d, K)
        return x, mask_u8, AC, E, tb, Wp

    def input_bwd(saved, dagg, g, B, d):
        x, mask_u8, AC, E, tb, Wp = saved
        front_bwd(x, mask_u8, AC, dagg, E, tb, Wp, g["E"], g["tb"], g["Wp"], g["cp"], B, d, E.shape[1])

    return Family(enc_names, dec_names, enc_input, gauss_sample, gauss_sample_bwd, 1, input_bwd=input_bwd, n_front=4)


FAMILY = pointnet_family((eddi_fold, eddi_front_fwd, eddi_front_bwd), _W6[:6], _W6[6:])

_FRONT_SPEC = (("E", "type_pars1", "front"), ("tb", "type_bias1", "front")) + mlp_spec(("Wp", "cp"), "pnp_encoder1", "front")


def _mlp(widths, *last):
    """nn.Sequential of Linear layers widths[0] -> widths[1] -> .. with a ReLU between them and `last` behind."""
    mods = [m for a, b in zip(widths, widths[1:]) for m in (nn.Linear(a, b), nn.ReLU())]
    return nn.Sequential(*mods[:-1], *last)


class _PointNet:
    """What the two point-net pairs (_EDDIBase here, eddi_mnist._EDDIMnistBase) share: the constructor prologue and the
    encoder on the chain-family frame.  A pair states `family`, `_kernels` / `_limits` (the VpcError past them) and the hidden
    widths `_trunk_hidden` / `_dec_hidden` of pnp_encoder2 (K -> .. -> 2L) and seq_decoder (L -> .. -> d, Sigmoid)."""

    def _build(self, obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, num_samples, num_estimates):
        nn.Module.__init__(self)
        max_d, max_l, max_k = self._limits
        if obs_dim > max_d or latent_dim > max_l or K > max_k:
            raise L.VpcError(f"the gfx950 {self._kernels} kernels support obs_dim <= {max_d}, latent_dim <= {max_l} and "
                             f"K (emb_dim) <= {max_k}")
        self.obs_dim, self.hid_dim, self.emb_dim, self.latent_dim, self.K = obs_dim, hid_dim, K, latent_dim, K
        self.batch_size = training_parameters["batch_size"]
        self.training_parameters, self.experiment_type = training_parameters, experiment_type
        self.num_samples, self.num_estimates = num_samples, num_estimates

    def _build_modules(self):
        # containers in the reference's construction order (same seed -> same initial weights), VAE.py:687-709 / 27-56
        K, latent_dim, obs_dim = self.emb_dim, self.latent_dim, self.obs_dim
        self.pnp_encoder1 = nn.Sequential(nn.Linear(2 + K, K), nn.ReLU())
        self.pnp_encoder2 = _mlp((K, *self._trunk_hidden, 2 * latent_dim))
        self.seq_decoder = _mlp((latent_dim, *self._dec_hidden, obs_dim), nn.Sigmoid())
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
        self._layout = self._img = None
        self._part = {}

    def encoder(self, x, mask, sample=True):
        """VAE.py:713-741 / 897-925 / 62-84 / 255-277: returns (z, mean, logvar)."""
        return self._encode(x, mask, sample)

    def _encode(self, x, mask, sample=True, eps=None):
        """encoder() with an injectable eps [B, L] (sample and no eps: drawn on the device)."""
        L.require_cuda(x)
        if mask.shape[0] == 0:  # VAE.py:717-718 / 66-67: ten columns whatever latent_dim is
            return torch.empty(0, 10), torch.empty(0, 10), torch.empty(0, 10)
        self._images()
        xf = ops._f32c(x.reshape(-1, self.obs_dim))
        m = as_mask_u8(mask.reshape(-1, self.obs_dim).to(x.device))
        if sample and eps is None:
            eps = torch.randn(xf.shape[0], self.latent_dim, device=xf.device)
        z, heads = ChainEncoderFn.apply(self.family, self, xf, m, ops._f32c(eps) if sample else None, 1, *self._enc_weights(),
                                        *self._segment_params("front"))
        return (z, *heads.chunk(2, dim=1))  # mean first; one split node, whose backward is one cat


class _EDDIBase(_PointNet):
    """Shared construction / parameter plumbing; mixed in BEFORE Reg_VAE / vanilla_VAE, whose decoder(), forward()
    and loss() (and the kernels behind them) are reused unchanged."""
    family = FAMILY
    _kernels, _limits = "EDDI", (128, 15, 32)
    _trunk_hidden, _dec_hidden = (H1, H2), (H2, H1)

    # flat order: [pnp_encoder2 (6) | seq_decoder (6) | type_pars1, type_bias1, pnp_encoder1 (2)] - the decoder sits at
    # indices 6..11 as in the VAE classes, which is what DecoderFn's gradient split assumes
    _flat_spec = mlp_spec(_W6[:6], "pnp_encoder2", "enc") + mlp_spec(_W6[6:], "seq_decoder", "dec") + _FRONT_SPEC

    def _new_image(self, device):
        """Only the DECODER half of the packed image is used (the encoder is the front-end + GEMM trunk)."""
        lay = self._lay()
        pidx = lay.device_tables(device)[0][lay.n_enc:]
        lo = sum(p.numel() for p in self.trainable()[:6])
        hi = lo + lay.n_params - lay.n_enc
        return PackedImage(torch.from_numpy(lay.img_template).to(device),
                           lambda flat, buf: ops.pack_weights(flat[lo:hi], pidx, buf))

    def decoder(self, z_int):
        """VAE.py:743-747: the Reg_VAE decoder kernels on this class's seq_decoder (trainable()[6:12])."""
        L.require_cuda(z_int)
        self._lay()
        self._images()
        return ops.DecoderFn.apply(self, z_int, *self.trainable()[6:12]), self.x_logvar


class Reg_EDDI(_EDDIBase, Reg_VAE):
    """Reference: src/models/VAE.py:670-853."""

    def __init__(self, obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, reg_type, num_samples=1,
                 num_estimates=1):
        self._build(obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, num_samples, num_estimates)
        self._build_modules()
        self.reg_type = reg_type

    def forward(self, data, mask, mask_p, stage="train"):
        return Reg_VAE.forward(self, data, mask, mask_p, stage)

    def loss(self, x, x_recon_p, x_logvar_p, mean_p, logvar_p, x_recon_q, x_logvar_q, mean_q, logvar_q, mask, mask_p,
             epoch, vae_elbo=False, llh_eval=False, MI=False, beta_annealing=False, beta=1.0, alpha=0.5, stage="train",
             alpha_annealing=False):
        """VAE.py:749-813: Reg_VAE.loss with this class's defaults (alpha = 0.5)."""
        return Reg_VAE.loss(self, x, x_recon_p, x_logvar_p, mean_p, logvar_p, x_recon_q, x_logvar_q, mean_q, logvar_q,
                            mask, mask_p, epoch, vae_elbo, llh_eval, MI, beta_annealing, beta, alpha, stage,
                            alpha_annealing)


class vanilla_EDDI(_EDDIBase, vanilla_VAE):
    """Reference: src/models/VAE.py:856-992."""

    def __init__(self, obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, num_samples=1,
                 num_estimates=1):
        self._build(obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, num_samples, num_estimates)
        self._build_modules()

    def loss(self, x, x_recon_q, x_logvar_q, mean_q, logvar_q, epoch, mask, vae_elbo=False, llh_eval=False, MI=False,
             beta_annealing=False, beta=1.0, alpha=0.5, stage="train"):
        """VAE.py:933-964: vanilla_VAE.loss, except that RE_q_imputed is computed in EVERY stage (:938-939)."""
        return vanilla_VAE.loss(self, x, x_recon_q, x_logvar_q, mean_q, logvar_q, epoch, mask, vae_elbo, llh_eval, MI,
                                beta_annealing, beta, alpha, True, "evaluate")


# ------------------------------------------------------------------------------------------------ fused step
LP = 16  # row pitch of the padded latent workspaces of the fused decoder kernel


def small_step_route(d, K, B, world_size, max_rows):
    """Whether EDDITrainer.step takes the small-batch one-kernel step (csrc/vpc_small.hip: step_small_eddi_kernel): a single
    rank, 0 < B <= max_rows (ops.step_small_max_rows(): 16 x CUs by default, 0 with VPC_STEP_SMALL=0) and a shape with an
    instantiation (K <= 32, obs_dim <= 64).  Data-parallel steps, larger batches and wider tables keep the launch chain."""
    return world_size == 1 and 0 < B <= max_rows and ops.small_eddi_tiles(d, K) is not None


class _SmallStep:
    """What the small-batch step of one EDDITrainer owns: the point-net layout's tables, the packed images of trunk and decoder
    and the per-tile buffers the chain has no use for."""

    def __init__(self, tr):
        m, dev = tr.model, tr.dev
        d, Ld, K = m.obs_dim, m.latent_dim, m.emb_dim
        lay = self.lay = L.pointnet_layout(d, K, Ld)
        n = lay.n_params
        self.pidx, _ = lay.device_tables(dev)
        self.inv = lay.inverse_maps(dev)
        pidx = self.pidx
        self.img = PackedImage(torch.from_numpy(lay.img_template).to(dev), lambda flat, buf: ops.pack_weights(flat[:n], pidx, buf))
        self.enc_img, self.dec_img = self.img.buf[:lay.enc_img], self.img.buf[lay.enc_img:]
        self.dk = ops.small_aug_pitch(d)
        nb = L.max_blocks()
        self.partE = torch.empty(nb * lay.enc_part, device=dev)
        self.partF = torch.empty(nb * 2 * K * self.dk, device=dev)
        self.snap = torch.empty(lay.n_front, device=dev)
        self.pads = {}
        self.B = None


_TRUNK_WKEYS = ((None, 2), (None, 1), (None, 0))  # (no timer, workspace index) of the trunk's layers 0, 1, 2


def param_chains(model):
    """(trunk, decoder) chains of a point-net model for its step trainer: the class's _build_chains on the Parameters
    themselves, which follow every re-assignment of p.data (the API path's model._chains() holds views of one flat buffer)."""
    return model._build_chains(dict(zip(*model._flat_table()[:2])))


class EDDITrainer(_FlatAdamTrainer):
    """The EDDI training step (train.py:28-117 for 'reg_EDDI*' / 'vanilla_EDDI*') as a fixed launch sequence without
    host synchronisation: [decoder image re-pack] -> mask_p + eps draws -> fold -> front-end (both passes) ->
    pnp_encoder2 GEMMs on the stacked passes -> the SAME fused decoder + loss + decoder-backward kernel as the VAE step
    (nothing of size B x d is materialised) -> trunk backward GEMMs -> front-end backward -> [one all-reduce of
    [grads | loss terms]] -> flat Adam.

    Small batches on one rank (small_step_route: B <= ops.step_small_max_rows(), K <= 32, obs_dim <= 64) run the whole step as
    TWO launches instead: step_small_eddi_kernel (draws, front-end, trunk, decoder, loss and every backward pass of a 16-row
    tile per workgroup) and one tail (fixed-order reductions, the front-end's chain rule, Adam, image re-pack).  The kernel
    takes x, mask and mask_p at 4 * ceil(obs_dim / 4) columns (mask 0 in the padding).  The draws keep the chain's counters,
    trainer.draw_counters at the pitch obs_dim, so the device-drawn mask_p and eps of a seed are bit for bit the chain's at
    every width: for obs_dim % 4 == 0 the kernel makes them itself; for obs_dim % 4 != 0 the chain's draw launch makes them on
    the unpadded rows and mask_p is padded afterwards (one launch and one copy more) - NOT the padded-pitch stream of the dense
    small-batch step, because tests/test_draw_rule_gpu.py pins this trainer's stream at obs_dim 14 to the unpadded pitch.
    VPC_STEP_SMALL=0 in the environment keeps the chain.  `last_path` names what the last step ran: "small" or "chain"."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, process_group=None, world_size=1, rank=0):
        if not isinstance(model, _EDDIBase):
            raise TypeError("EDDITrainer supports Reg_EDDI and vanilla_EDDI")
        super().__init__(model, lr, betas, eps, seed, process_group, world_size, rank, 9)
        self.vanilla = isinstance(model, vanilla_VAE)
        self.lay = model._lay()
        self.out9 = self.tail
        ncu = L.max_blocks()  # partial blocks any kernel may write
        self.partD = torch.empty(ncu * self.lay.dec_part, device=self.dev)
        self.loss_part = torch.empty(ncu, 8, dtype=torch.float64, device=self.dev)
        _, self.gidx = self.lay.device_tables(self.dev)
        self.g = [p.grad for p in self._plist]  # gradient views in flat order: trunk (6) | decoder (6) | front-end (4)
        self.n_trunk = sum(p.numel() for p in self._plist[:6])
        self.n_dec = self.lay.n_params - self.lay.n_enc
        self._B = None
        self._small = None  # the small-batch step's tables and buffers: made on its first use
        # (what of small_step_route is fixed per trainer: the row limit is asked for only where it can matter)
        self._small_shape = world_size == 1 and ops.small_eddi_tiles(model.obs_dim, model.emb_dim) is not None
        self.last_path = None

    def _draws(self, mask, mask_p, eps_in, co, keep_prob, B, Bg, row_lo, in_kernel_ok=False):
        """THE inject-or-draw rule of the step, for both paths, on self.eps_buf [3][B][LP] and self.mask_p_buf.  eps_in =
        (eps_q, eps_p, eps_ml); the planes the step consumes are q, then p (regularised), then ml_reg's third.  eps is drawn
        together with mask_p whenever mask_p is absent (injected planes are copied over it), else unless eps_q is injected.
        in_kernel_ok (the small path at obs_dim % 4 == 0) and every draw made on the device: no launch here, the step's kernel
        makes them.  Returns (mask_p as uint8 or None, whether the third plane is read, the in-kernel arguments or None)."""
        d, Ld = self.model.obs_dim, self.model.latent_dim
        two = not self.vanilla
        need_ml = two and co.ml_on
        planes = 3 if need_ml else 2 if two else 1
        eps_view, eps_in = self.eps_buf[:planes], eps_in[:planes]
        draw_mask = two and mask_p is None
        draw_eps = draw_mask or eps_in[0] is None
        dr = draw_counters(self.rng_offset, draw_mask, planes if draw_eps else 0, B, Bg, row_lo, LP, d)  # GLOBAL row
        self.rng_offset = dr.next_offset
        in_kernel = None
        if in_kernel_ok and draw_mask == two and all(e is None for e in eps_in):
            in_kernel = (mask if two else None, keep_prob, eps_view, self.seed, dr.offset_mask, dr.offset_eps, None, dr.elem_lo,
                         dr.eps_shard)
        elif draw_mask:
            ops.draw_step(mask, self.mask_p_buf, keep_prob, eps_view, self.seed, dr.offset_mask, dr.offset_eps, None, dr.elem_lo,
                          dr.eps_shard)
        elif draw_eps:
            ops.fill_normal(eps_view, self.seed, dr.offset_eps, None, dr.eps_shard)
        if draw_mask:
            mask_p = self.mask_p_buf
        elif two:
            mask_p = as_mask_u8(mask_p.reshape(-1, d))
        for plane, e in enumerate(eps_in):
            if e is not None:
                self.eps_buf[plane, :, :Ld].copy_(e)
        return mask_p, need_ml, in_kernel

    def _ws(self, B):
        if self._B == B:
            return
        m, dev = self.model, self.dev
        d, Ld, K = m.obs_dim, m.latent_dim, m.emb_dim
        P = 1 if self.vanilla else 2
        e = lambda *s: torch.empty(*s, device=dev)
        self.AC = e(2, K, d)
        self.trunk = param_chains(m)[0]
        self.enc = [e(P * B, K), e(P * B, H1), e(P * B, H2), e(P * B, 2 * Ld)]    # agg, h1, h2, heads
        self.denc = [e(P * B, K), e(P * B, H1), e(P * B, H2), e(P * B, 2 * Ld)]   # dagg, dh1, dh2, dheads
        self.lat = torch.zeros(P, 2, B, LP, device=dev)    # [pass][mean | logvar][B][16]
        self.dlat = torch.zeros(P, 2, B, LP, device=dev)
        self.eps_buf = e(3, B, LP)
        self.mask_p_buf = torch.empty(B, d, dtype=torch.uint8, device=dev)
        self.front_scratch = e(int(lib().vpc_eddi_front_scratch(P * B, d, K)))
        # per-layer partial buffers of the trunk's three weight gradients, last layer first (_TRUNK_WKEYS): summed by ONE launch
        # (vpc_linear_wgrad_reduce)
        R, g = P * B, self.g
        self._wgrad_workspace([(R, 2 * Ld, H2), (R, H2, H1), (R, H1, K)], [(g[4], g[5]), (g[2], g[3]), (g[0], g[1])])
        # the slices the step passes to its launches, made once per batch size (1-3 us of host time each; the step is host-paced)
        self._sl = dict(mean=[self.lat[p_, 0] for p_ in range(P)], logvar=[self.lat[p_, 1] for p_ in range(P)],
                        dmean=[self.dlat[p_, 0] for p_ in range(P)], dlogvar=[self.dlat[p_, 1] for p_ in range(P)],
                        eps=[self.eps_buf[p_] for p_ in range(3)], lat_dst=self.lat[..., :Ld],
                        heads_src=self.enc[3].view(P, B, 2, Ld).permute(0, 2, 1, 3), dheads_dst=self.denc[3].view(P, B, 2, Ld),
                        dlat_src=self.dlat[..., :Ld].permute(0, 2, 1, 3),
                        gdec=self.grad[self.n_trunk:self.n_trunk + self.n_dec], gidx_dec=self.gidx[self.lay.n_enc:])
        self._B = B
        if self._small is not None:
            self._small.B = None  # (eps_buf and mask_p_buf are the chain's now)

    def step(self, x, mask, mask_p=None, eps_q=None, eps_p=None, eps_ml=None, *, epoch=1, alpha=0.5, beta=1.0,
             beta_annealing=False, p_missingness=30, global_batch=None, row_lo=None):
        m, lay = self.model, self.lay
        d, Ld, K = m.obs_dim, m.latent_dim, m.emb_dim
        x = ops._f32c(x.reshape(-1, d))
        L.require_cuda(x)
        mask = as_mask_u8(mask.reshape(-1, d))
        B = x.shape[0]
        if self._small_shape and small_step_route(d, K, B, self.world_size, ops.step_small_max_rows()):
            return self._step_small(x, mask, mask_p, (eps_q, eps_p, eps_ml), self.coefficients(epoch, alpha, beta, beta_annealing),
                                    1.0 - p_missingness / 100.0, global_batch, row_lo)
        self.last_path = "chain"
        self._ws(B)
        Bg, row_lo = self._batch_rows(B, global_batch, row_lo)
        co = self.coefficients(epoch, alpha, beta, beta_annealing)
        two = not self.vanilla
        P = 2 if two else 1
        t = self._plist
        E, tb, Wp, cp = t[12:]
        dec_img = m._images(m._param_key(t))[lay.enc_img:]  # re-packed after the previous step's Adam
        mask_p, need_ml, _ = self._draws(mask, mask_p, (eps_q, eps_p, eps_ml), co, 1.0 - p_missingness / 100.0, B, Bg, row_lo)
        masks = [mask, mask_p] if two else [mask]
        # ---- encoder: front-end per pass, trunk on the stacked passes
        eddi_fold(E, tb, Wp, cp, self.AC, d, K)
        eddi_front_fwd(x, masks[0], self.AC, self.enc[0], B, d, K, masks[1] if two else None)  # both passes, one launch
        R = P * B
        chain_fwd(self.trunk, self.enc, R)
        sl = self._sl
        sl["lat_dst"].copy_(sl["heads_src"])
        mean, logvar, dmean, dlogvar = sl["mean"], sl["logvar"], sl["dmean"], sl["dlogvar"]
        epss = sl["eps"][:P]
        eml = sl["eps"][2] if need_ml else None
        # ---- fused decoder + loss + decoder backward (the VAE step's kernel)
        maskB = [mask_p, None] if (two and co.maskB_on) else [None] * P
        nbD = ops.decoder_fused(x, dec_img, masks, maskB, co, mean, logvar, epss, eml, 1.0 / Bg, m._x_logvar_value, dmean,
                                dlogvar, self.partD, self.loss_part, d, Ld, LP)
        ops.reduce_partials(self.partD, nbD, lay.dec_part, sl["gidx_dec"], sl["gdec"])
        ops.loss_finalize(self.loss_part, nbD, co, B, Bg, d, self.out9, self.accum if self.world_size == 1 else None)
        # ---- encoder backward
        sl["dheads_dst"].copy_(sl["dlat_src"])
        g = self.g
        # (the three weight gradients leave their GEMMs as partials and are summed by ONE launch: two launches less per step;
        # the aggregate is a sum of ReLUs, not a ReLU output: its dgrad has no gate)
        chain_bwd(self.trunk, self.enc, self.denc, R, self._wgrad, _TRUNK_WKEYS)
        self._wgrad_reduce()
        eddi_front_bwd(x, masks[0], self.AC, self.denc[0], E, tb, Wp, g[12], g[13], g[14], g[15], B, d, K,
                       mask2_u8=masks[1] if two else None, scratch=self.front_scratch)
        if self.world_size > 1:
            self._allreduce()
        dp = self.world_size > 1  # the Adam launch also adds the all-reduced loss to the epoch accumulator
        self._adam(None, self.out9 if dp else None, self.accum if dp else None)

    def _step_small(self, x, mask, mask_p, eps_in, co, keep_prob, global_batch, row_lo):
        """The step as step_small_eddi_kernel + one tail launch (class docstring).  x [B][d] fp32, mask [B][d] uint8."""
        m, dev = self.model, self.dev
        d, Ld, K = m.obs_dim, m.latent_dim, m.emb_dim
        s = self._small
        if s is None:
            s = self._small = _SmallStep(self)
        lay, dk, B = s.lay, s.dk, x.shape[0]
        two = not self.vanilla
        if s.B != B:
            self.eps_buf = torch.empty(3, B, LP, device=dev)
            self.mask_p_buf = torch.empty(B, d, dtype=torch.uint8, device=dev)
            s.eps = [self.eps_buf[p_] for p_ in range(3)]
            s.B, self._B = B, None  # (the chain makes its own workspaces again)
        Bg, row_lo = self._batch_rows(B, global_batch, row_lo)
        key = m._param_key(self._plist)
        img = s.img.get(key, m._flat)
        # ---- draws (_draws).  obs_dim % 4 == 0 and every draw made on the device: the kernel makes them; else the chain's
        # launches, on the unpadded rows
        mask_p, need_ml, in_kernel = self._draws(mask, mask_p, eps_in, co, keep_prob, B, Bg, row_lo, in_kernel_ok=dk == d)
        if dk != d:  # the kernel's rows: 4 * ceil(d / 4) columns, mask 0 in the padding
            x, mask = pad_cols(s.pads, x, dk, 0, dev), pad_cols(s.pads, mask, dk, 1, dev)
            if two:
                mask_p = pad_cols(s.pads, mask_p, dk, 2, dev)
        # ---- the step, then the tail
        masks = [mask, mask_p] if two else [mask]
        maskB = [mask_p, None] if (two and co.maskB_on) else [None] * len(masks)
        args = (x, s.enc_img, s.dec_img, masks, maskB, co, s.eps[:len(masks)], s.eps[2] if need_ml else None, 1.0 / Bg,
                m._x_logvar_value, s.partE, self.partD, self.loss_part, dk, d, Ld, K, m._flat[lay.n_params:], s.partF, s.snap)
        if in_kernel is not None:
            nb = self._timed("step_small", ops.step_small_eddi_draw_f32, *args, *in_kernel)
        else:
            nb = self._timed("step_small", ops.step_small_eddi_f32, *args)
        self.step_count += 1
        self._timed("reduce_step", ops.reduce_step_adam_eddi, s.partE, self.partD, nb, lay.enc_part, lay.dec_part, s.inv,
                    self.grad, lay.n_params, self.loss_part, co, B, Bg, d, self.out9, self.accum, m._flat, self.exp_avg,
                    self.exp_avg_sq, self.lr, self.betas[0], self.betas[1], self.adam_eps, self.step_count, s.pidx, img, s.partF,
                    s.snap, K, dk)
        self._flat_written(key, s.img)
        self.last_path = "small"
