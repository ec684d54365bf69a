"""Fused training step: the build's counterpart of the reference's step body
src/experiment_main/train.py:53-117 for Reg_VAE / vanilla_VAE:

    mask_p draw -> forward (2 x encoder, 2 x decoder) -> loss -> zero_grad -> backward -> Adam -> loss accumulate

as 5 kernel launches (6 under data parallelism) and no B x d intermediate - 4 (5) on the fp32 row-tiled path at batches
that give every CU a 128-row tile, where the two draws are made by the kernels that consume them
(vpc_encoder_fwd_draw_f32 draws mask_p for the mask words it holds, vpc_decoder_fused_draw_f32 the eps of the lane that
forms z; FusedTrainer._draw_fused says when):

    vpc_draw_step            mask_p = mask & Bernoulli(1 - p_missingness/100) and eps_q, eps_p (, eps_ml), Philox
                             counters keyed by the GLOBAL row                        (train.py:53-55, VAE.py:389-392)
    vpc_encoder_fwd          both passes, writes h1/h2 workspaces + mean/logvar      (VAE.py:387-395)
    vpc_decoder_fused        reparameterise + decoder + loss + seeds + decoder bwd   (VAE.py:397-467)
    vpc_encoder_bwd          encoder backward of both passes                         (train.py:115)
    vpc_reduce_step_adam     per-workgroup partial blocks -> flat gradient (fixed order) + loss scalar + epoch
                             accumulator + flat Adam + re-pack of the weight images  (train.py:114-117, no host sync)
      data parallel / graph replay: vpc_reduce_step -> [ONE all-reduce of the flat bucket: grads + loss terms]
                             -> vpc_adam_step
    precision "bf16", obs_dim in (64, 128], throughput shape: encoder_fwd + decoder_fused + encoder_bwd are ONE launch,
    vpc_step_fused_bf16 (csrc/vpc_step.hip) - h1 / h2 / latent statistics never leave the chip
    fp32 with the draws in the kernels and two passes, from 128 rows x CUs on: the same three are the three PHASES of one
    launch, vpc_step_f32 (csrc/vpc_step_f32.hip) - the kernels' code and bytes, two kernel boundaries less
    (FusedTrainer._step_f32 says when; 2 launches per step)

Gradients are those of the GLOBAL mean loss: seeds carry 1/B_global, so summing the flat bucket over ranks is
exactly `train_loss = loss / x.shape[0]` (VAE.py:452) on the concatenated batch.
"""
from __future__ import annotations

import os

import torch

from . import _lib as L
from . import dist as dp_mod
from . import ops
from .images import PackedImage
from .models import Reg_VAE, loss_coefficients, vanilla_VAE  # noqa: F401  (also reached as fused.loss_coefficients)
from .ops import H1P, H2P, as_mask_u8
from .trainer import _FlatAdamTrainer, draw_counters, pad_cols, padded_width

LP = 16  # row pitch of the padded latent workspaces


class FusedTrainer(_FlatAdamTrainer):
    timer_every = 8  # an event pair costs ~5 us of GPU idle time per kernel: bench.py brackets every 8th step only

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, process_group=None, world_size=1, rank=0,
                 precision="f32", collective=None):
        """precision: "f32" (v_mfma_f32_16x16x4_f32, the parity path), "bf16x3" (split-bf16 products on
        v_mfma_f32_16x16x32_bf16: fp32-class accuracy) or "bf16" (plain bf16 inputs, fp32 accumulation and loss math);
        the bf16 forms exist for Reg_VAE / vanilla_VAE with obs_dim % 4 == 0, both workgroup shapes (csrc/vpc_bf16.h).
        `precision` bounds the rounding a step may use; it does not choose the kernel: small batches run the fp32
        N-split kernel in every precision.
        Mask-augmented models (Reg_VAE_mask / vanilla_VAE_mask) take the N-split kernel too at small batches.  There
        x, mask and mask_p are padded to 4 * ceil(obs_dim / 4) columns (mask 0 in the padding) and the draw counters are
        trainer.draw_counters at THAT pitch: for obs_dim % 4 == 0 the draws are bit for bit those of the row-tiled path
        (VPC_STEP_SMALL=0, or a larger batch); for obs_dim % 4 != 0 the mask_p stream of a seed is the plain models'
        stream at the padded pitch, not the unpadded one the row-tiled path draws.
        collective: carrier of the per-step bucket under data parallelism (dist.FlatAllReduce = ncclAllReduce on the
        compute stream); None = chosen on the first multi-rank step by dist.make_collective (RCCL when the process group
        is NCCL, torch.distributed.all_reduce otherwise)."""
        if not isinstance(model, (Reg_VAE, vanilla_VAE)):
            raise TypeError("FusedTrainer supports Reg_VAE and vanilla_VAE")
        if getattr(model, "_wide", False):
            raise L.VpcError("FusedTrainer covers encoder inputs <= 128 wide and latent_dim <= 15; use wide.WideTrainer "
                             "(harness.train does) for wider models")
        if precision not in ops.PRECISIONS:
            raise ValueError(f"precision {precision!r}: expected one of {sorted(ops.PRECISIONS)}")
        # data parallel: this rank's rows are [rank * B, (rank + 1) * B) of the global batch by default
        super().__init__(model, lr, betas, eps, seed, process_group, world_size, rank, 9, collective)
        self.vanilla = isinstance(model, vanilla_VAE)
        # the data-parallel tail (reduce_step -> all-reduce -> adam_step) instead of the single fused launch
        self.dp = world_size > 1 or collective is not None
        self.lay = model._lay()
        self.precision = precision
        self.prec = ops.PRECISIONS[precision]
        if self.prec:
            lay = self.lay
            if lay.mask_augm or lay.d % 4:
                raise L.VpcError("the bf16 / bf16x3 kernels cover the plain encoder with obs_dim % 4 == 0 (<= 128)")
            pidx_bf, tmpl, self.enc_img_bf = lay.bf16_tables(self.dev)
            # bf16 images, packed lazily from the flat parameters under the model's parameter key (images.py)
            self._pair = PackedImage(torch.from_numpy(tmpl).to(self.dev),
                                     lambda flat, buf: ops.pack_weights_bf16(flat, pidx_bf, buf))
            # plain bf16, obs_dim in (64, 128]: the whole-step kernel (csrc/vpc_step.hip) with its own compact image
            self._step_ok = self.prec == 2 and 64 < lay.d <= 128
            if self._step_ok:
                pidx_c, tmpl_c = lay.step_tables(self.dev)
                self.pidx_c = pidx_c  # (the pack functions hold no reference to the trainer: no cycle, freed by refcount)
                self._whole = PackedImage(torch.from_numpy(tmpl_c).to(self.dev),
                                          lambda flat, buf: ops.step_pack_weights_bf16(flat, pidx_c, buf))
        self.out9 = self.tail  # the loss terms of the step
        ncu = L.max_blocks()  # partial blocks any kernel may write (2 x CUs: small-batch shape)
        self._draw_fused_rows = 64 * ncu  # 128 rows x CUs: from here on the row-tiled fp32 step draws in its kernels (_draw_fused)
        self.partE = torch.empty(ncu * self.lay.enc_part, device=self.dev)
        self.partD = torch.empty(ncu * self.lay.dec_part, device=self.dev)
        self.loss_part = torch.empty(ncu, 8, dtype=torch.float64, device=self.dev)
        self.pidx, self.gidx = self.lay.device_tables(self.dev)
        self.inv = self.lay.inverse_maps(self.dev)  # caller-owned maps for the layout-order gradient reduction
        self._ws_B = None
        self._pads = {}

    def invalidate_image(self):
        """Alias of model.invalidate_images(): after writing parameters behind torch's version counters."""
        self.model.invalidate_images()

    # ------------------------------------------------------------------
    def _workspaces(self, B, d):
        if self._ws_B == (B, d):
            return
        dev, Ld = self.dev, self.lay.L
        np_ = 1 if self.vanilla else 2
        self.h1 = [torch.empty(B, H1P, device=dev) for _ in range(np_)]
        self.h2 = [torch.empty(B, H2P, device=dev) for _ in range(np_)]
        # latent statistics live in padded [B][16] workspaces (16-byte vector access in the kernels)
        self.mean = [torch.empty(B, LP, device=dev) for _ in range(np_)]
        self.logvar = [torch.empty(B, LP, device=dev) for _ in range(np_)]
        self.dmean = [torch.empty(B, LP, device=dev) for _ in range(np_)]
        self.dlogvar = [torch.empty(B, LP, device=dev) for _ in range(np_)]
        self.eps_buf = torch.empty(3, B, LP, device=dev)
        self.mask_p_buf = torch.empty(B, d, dtype=torch.uint8, device=dev)
        self._ws_B = (B, d)

    def _step_ws(self, B):
        """Workspace of the whole-step kernel (the packed seeds between its two sweeps)."""
        n = ops.step_workspace_floats(B)
        if getattr(self, "_ws_step", None) is None or self._ws_step.numel() < n:
            self._ws_step = torch.empty(n, device=self.dev)
        return self._ws_step

    def dominant_launch(self):
        """Name (as in `timers`) of the launch that carries most of the step's FLOPs in the shape last stepped."""
        if getattr(self, "_used_step_small", False):
            return "step_small"
        if getattr(self, "_used_step_fused", False) or getattr(self, "_used_step_f32", False):
            return "step_fused"
        return "decoder_fused"

    # ------------------------------------------------------------------
    def step(self, x, mask, mask_p=None, eps_q=None, eps_p=None, eps_ml=None, *, epoch=1, alpha=1.0, beta=1.0,
             beta_annealing=False, p_missingness=30, global_batch=None, row_lo=None, update=True, _state=None):
        """One training step on the local rows `x` [B, d] (fp32, GPU), `mask` [B, d] (bool / uint8 / float).
        mask_p / eps_* are drawn on the device unless injected (parity tests).  Returns nothing: the loss of
        this step is in `self.out9[0]` (device), the running total in `self.accum` (train.py:117).
        Data parallel: `global_batch` rows in all (default B * world_size) of which this rank holds
        [row_lo, row_lo + B) (default rank * B).  The Philox counters of the draws are those of the GLOBAL row
        (SURVEY.md section 8e): with one shared seed every row gets the mask_p / eps it would get in the single-process
        step on the concatenated batch, whatever the world size."""
        L.require_cuda(x)
        self._timer_tick += 1
        lay, m = self.lay, self.model
        B, d, Ld = x.shape[0], lay.d, lay.L
        # Small batches run the fp32 N-split kernel (csrc/vpc_small.hip) in EVERY precision: `precision` bounds the rounding a step may
        # use, and at these sizes the fp32 kernel is both the most accurate and the fastest form (B = 64: 41 us against 62 us for the
        # bf16 engine's small-shape kernels).  VPC_STEP_SMALL=0 in the environment keeps the requested engine (tests of its kernels).
        use_small = B <= ops.step_small_max_rows()  # (<= 16 x CUs rows)
        # ---- inputs and padding
        x = ops._f32c(x)
        mask = as_mask_u8(mask)
        # Row pitch of the kernels' x / mask arrays.  obs_dim % 4 != 0 would take the scalar-load kernel variants (the ones
        # that spill, profiles/r01_kernel_resources.txt): instead the inputs are copied into arrays padded to a multiple of
        # 4 columns with mask 0 in the padding - never observed, so it adds nothing to any sum or gradient, and the weight
        # images already hold zeros for the columns / rows past obs_dim - and the 16-byte-vector variants run on those.
        # The mask-augmented classes: unpadded rows for the row-tiled kernels, that padding rule for the N-split kernel.
        dk = ops.small_aug_pitch(d) if (use_small and lay.mask_augm) else padded_width(d, lay.mask_augm)
        if dk != d:
            x, mask = pad_cols(self._pads, x, dk, 0, self.dev), pad_cols(self._pads, mask, dk, 1, self.dev)
            if mask_p is not None:
                mask_p = pad_cols(self._pads, as_mask_u8(mask_p), dk, 2, self.dev)
        self._workspaces(B, dk)
        Bg, row_lo = self._batch_rows(B, global_batch, row_lo)
        co = self.coefficients(epoch, alpha, beta, beta_annealing)
        two = not self.vanilla
        self._used_step_small = use_small
        use_step = (not use_small) and bool(self.prec) and self._step_ok and ops.step_fused_applicable(B, dk, Ld, 2 if two else 1)
        self._used_step_fused = use_step
        # every image is checked against ONE parameter key per step (images.py).  The model's fp32 images are what the fp32
        # kernels read and the Adam launches re-pack; the whole-step bf16 kernel has its own image and leaves them stale
        key = m._param_key(self._plist)
        img = None if use_step else m._images(key)
        if use_step:
            imgs = (self._whole.get(key, m._flat),)
        elif self.prec and not use_small:
            img_bf = self._pair.get(key, m._flat)
            imgs = (img_bf[:self.enc_img_bf], img_bf[self.enc_img_bf:])
        else:
            imgs = (img[:lay.enc_img], img[lay.enc_img:])
        rng0 = self.rng_offset
        # ---- random draws
        mask_p, in_kernel = self._draws(co, mask, mask_p, (eps_q, eps_p, eps_ml), B, Bg, row_lo, dk, use_small,
                                        1.0 - p_missingness / 100.0, _state)
        # ---- forward, loss and backward: the launches of this batch size and precision
        nbE, nbD = self.last_blocks = self._launches(co, x, mask, mask_p, in_kernel, imgs, B, Bg, dk, use_small, use_step)
        # ---- flat gradient + loss terms, Adam
        self._tail(co, key, img, imgs[0] if use_step else None, nbE, nbD, B, Bg, update, _state, self.rng_offset - rng0)

    def _draw_fused(self, B, dk, planes, all_drawn):
        """Whether the row-tiled step makes its draws inside encoder_fwd / decoder_fused (one launch less, the mask read once
        less): fp32, the 8-wave kernels (plain encoder, dk in (64, 128], VPC_DEC8 / VPC_TILE not selecting the other shape),
        no Philox group straddling a row (dk % 8 == 0), padded latent rows, every draw made on the device, at most two eps
        planes (the ml_reg sample is a third), and a batch that gives every CU a 128-row tile - below it the separate launch
        stays.  VPC_DRAW_FUSED=0 keeps the separate launch, =1 takes the in-kernel draws at any batch size (tests, A/B runs)."""
        env = os.environ.get("VPC_DRAW_FUSED", "")
        if env == "0" or self.prec or self.lay.mask_augm or not (64 < dk <= 128) or dk % 8 or LP != 16:
            return False
        if not all_drawn or planes > 2 or os.environ.get("VPC_DEC8") == "0" or os.environ.get("VPC_TILE") == "64":
            return False
        return env == "1" or B >= self._draw_fused_rows

    def _step_f32(self, B):
        """Whether a step whose draws are made in its kernels (_draw_fused) and that has two passes runs encoder_fwd,
        decoder_fused and encoder_bwd as the three phases of ONE launch (ops.step_f32, csrc/vpc_step_f32.hip; timed as
        `step_fused`): from 128 rows x CUs on, where the three kernels run one common grid, unless a switch selects another
        form of one of them.  VPC_STEP_F32=0 keeps the three launches, =1 takes the one launch at any batch size with
        encoder_bwd in the throughput shape (tests, A/B runs)."""
        env = os.environ.get("VPC_STEP_F32", "")
        if env == "0" or self.vanilla or "VPC_TILE" in os.environ:
            return False
        if any(os.environ.get(k) == "0" for k in ("VPC_ENC_SWEEP", "VPC_DRAW_FUSED", "VPC_DEC8")):
            return False
        return env == "1" or B >= self._draw_fused_rows

    def _draws(self, co, mask, mask_p, eps_in, B, Bg, row_lo, dk, use_small, keep_prob, _state):
        """The step's draws - mask_p into mask_p_buf, eps into eps_buf - on the device unless injected, at the counters of
        trainer.draw_counters (mask_p and eps in ONE launch when both are drawn).  All planes are drawn if any consumed
        plane is missing; injected ones are copied over them.  Returns (mask_p, the arguments of the in-kernel draw or None)."""
        two = not self.vanilla
        planes = 3 if (two and co.ml_on) else 2 if two else 1  # only the draws this step consumes
        eps_view, eps_in = self.eps_buf[:planes], eps_in[:planes]
        draw_mask = two and mask_p is None
        draw_eps = any(e is None for e in eps_in)
        dr = draw_counters(self.rng_offset, draw_mask, planes if draw_eps else 0, B, Bg, row_lo, LP, dk)
        self.rng_offset = dr.next_offset
        # (`_state`: under graph replay the offset lives on the device - a frozen host offset would replay one eps)
        in_kernel = None
        if use_small and draw_mask == two and all(e is None for e in eps_in) and LP == 16:
            # small batches: the N-split kernel makes the step's draws itself (same counters, one launch less) when ALL of
            # them are drawn on the device
            in_kernel = (mask if two else None, keep_prob, eps_view, self.seed, dr.offset_mask, dr.offset_eps, _state,
                         dr.elem_lo, dr.eps_shard)
        elif not use_small and self._draw_fused(B, dk, planes, draw_mask == two and all(e is None for e in eps_in)):
            # row-tiled fp32 step: encoder_fwd draws mask_p, decoder_fused draws eps (same counters; _launches)
            in_kernel = (mask if two else None, keep_prob, eps_view, self.seed, dr.offset_mask, dr.offset_eps, _state,
                         dr.elem_lo, dr.eps_shard)
        elif draw_mask and draw_eps:
            self._timed("draw_step", ops.draw_step, mask, self.mask_p_buf, keep_prob, eps_view, self.seed, dr.offset_mask,
                        dr.offset_eps, _state, dr.elem_lo, dr.eps_shard)
        elif draw_mask:
            ops.draw_mask(mask, self.mask_p_buf, keep_prob, self.seed, dr.offset_mask, dr.elem_lo)
        elif draw_eps:
            ops.fill_normal(eps_view, self.seed, dr.offset_eps, _state, dr.eps_shard)
        if draw_mask:
            mask_p = self.mask_p_buf
        elif two:
            mask_p = as_mask_u8(mask_p)
        for plane, e in enumerate(eps_in):  # injected draws (parity tests) arrive dense [B][L]; pad entries are ignored
            if e is not None:
                self.eps_buf[plane, :, :self.lay.L].copy_(e)
        return mask_p, in_kernel

    def _launches(self, co, x, mask, mask_p, in_kernel, imgs, B, Bg, dk, use_small, use_step):
        """Forward, loss and backward into the partial blocks; returns how many (encoder, decoder) blocks were written."""
        lay, two = self.lay, not self.vanilla
        Ld, inv_B, xlv = lay.L, 1.0 / Bg, self.model._x_logvar_value
        masks = [mask, mask_p] if two else [mask]
        epss = [self.eps_buf[0], self.eps_buf[1]] if two else [self.eps_buf[0]]
        eml = self.eps_buf[2] if (two and co.ml_on) else None
        maskB = [mask_p, None] if (two and co.maskB_on) else [None] * len(masks)
        if use_small:
            # small batch (fp32 arithmetic in every precision): the whole step in ONE launch, 16-row tiles with the feature
            # tiles split over the waves; the mask-augmented classes through the entries whose input stage builds [x*mask | mask]
            args = (x, *imgs, masks, maskB, co, epss, eml, inv_B, xlv, self.partE, self.partD, self.loss_part, dk)
            args += (lay.d, Ld) if lay.mask_augm else (Ld,)
            fn, fn_draw = ((ops.step_small_aug_f32, ops.step_small_aug_draw_f32) if lay.mask_augm else
                           (ops.step_small_f32, ops.step_small_draw_f32))
            if in_kernel is not None:
                nb = self._timed("step_small", fn_draw, *args, *in_kernel)
            else:
                nb = self._timed("step_small", fn, *args)
            return nb, nb
        if use_step:
            # plain bf16, throughput shape: encoder forward + decoder + loss + all backward in ONE launch
            nb = self._timed("step_fused", ops.step_fused_bf16, x, imgs[0], masks, maskB, co, epss, eml, inv_B, xlv,
                             self.partE, self.partD, self.loss_part, self._step_ws(B), dk, Ld)
            return nb, nb
        # forward (encoder), fused decoder + loss + decoder backward, encoder backward
        enc_img, dec_img = imgs
        self._used_step_f32 = False
        if in_kernel is not None and self._step_f32(B):
            # the three MFMA kernels as phases of one launch (same bytes everywhere); None: they would not share a grid
            mask_in, keep_prob, _, seed, off_mask, off_eps, state, elem_lo, eps_shard = in_kernel
            nb = self._timed("step_fused", ops.step_f32, x, enc_img, dec_img, mask_in, self.mask_p_buf, maskB, co, self.h1,
                             self.h2, self.mean, self.logvar, epss, inv_B, xlv, self.dmean, self.dlogvar, self.partE,
                             self.partD, self.loss_part, dk, Ld, keep_prob, seed, off_mask, off_eps, state, elem_lo, eps_shard,
                             os.environ.get("VPC_STEP_F32") == "1")
            if nb is not None:
                self._used_step_f32 = True
                return nb
        if in_kernel is not None:
            # the draws inside the two kernels that consume them (_draw_fused); vanilla_VAE has no mask_p: plain encoder_fwd
            mask_in, keep_prob, _, seed, off_mask, off_eps, state, elem_lo, eps_shard = in_kernel
            if two:
                self._timed("encoder_fwd", ops.encoder_fwd_draw_f32, x, enc_img, mask_in, self.mask_p_buf, self.h1, self.h2,
                            self.mean, self.logvar, dk, Ld, keep_prob, seed, off_mask, state, elem_lo)
            else:
                self._timed("encoder_fwd", ops.encoder_fwd, x, enc_img, masks, None, self.h1, self.h2, self.mean,
                            self.logvar, None, dk, Ld, LP, lay.mask_augm, self.prec)
            nbD = self._timed("decoder_fused", ops.decoder_fused_draw_f32, x, dec_img, masks, maskB, co, self.mean,
                              self.logvar, epss, inv_B, xlv, self.dmean, self.dlogvar, self.partD, self.loss_part, dk, Ld,
                              seed, off_eps, state, eps_shard)
        else:
            self._timed("encoder_fwd", ops.encoder_fwd, x, enc_img, masks, None, self.h1, self.h2, self.mean, self.logvar,
                        None, dk, Ld, LP, lay.mask_augm, self.prec)
            nbD = self._timed("decoder_fused", ops.decoder_fused, x, dec_img, masks, maskB, co, self.mean, self.logvar, epss,
                              eml, inv_B, xlv, self.dmean, self.dlogvar, self.partD, self.loss_part, dk, Ld, LP, self.prec)
        nbE = self._timed("encoder_bwd", ops.encoder_bwd, x, enc_img, masks, self.h1, self.h2, self.dmean,
                          self.dlogvar, self.partE, dk, Ld, LP, lay.mask_augm, self.prec)
        return nbE, nbD

    def _tail(self, co, key, img, img_c, nbE, nbD, B, Bg, update, _state, rng_inc):
        """Partial blocks -> flat gradient + loss terms (+ Adam when nothing has to happen between them: one launch).
        img_c: the compact bf16 image when the whole-step kernel ran (else None), img: the model's fp32 images."""
        lay, m, use_step = self.lay, self.model, img_c is not None
        blocks = (self.partE, nbE, lay.enc_part, self.partD, nbD, lay.dec_part, self.gidx, self.grad, lay.n_enc,
                  self.loss_part, nbD, co, B, Bg, lay.d, self.out9)
        if update and not self.dp and _state is None:
            self.step_count += 1
            # the fused Adam re-packs the image the step read: the whole-step kernel's compact bf16 image, else the model's
            # fp32 images (the pair-slot bf16 image goes stale and is re-packed by whoever needs it next)
            self._timed("reduce_step", ops.reduce_step_adam, *blocks, self.accum, m._flat, self.exp_avg, self.exp_avg_sq,
                        self.lr, self.betas[0], self.betas[1], self.adam_eps, self.step_count,
                        self.pidx_c if use_step else self.pidx, img_c if use_step else img, self.inv, use_step)
            self._flat_written(key, self._whole if use_step else m._img)
            return
        ops.reduce_step(*blocks, None if self.dp else self.accum, _state, rng_inc if _state is not None else 0, self.inv)
        if self.dp:
            self._allreduce()
        if update:
            self.step_count += 1
            # under data parallelism the Adam launch also adds the all-reduced loss to the epoch accumulator
            ops.adam_step(m._flat, self.grad, self.exp_avg, self.exp_avg_sq, self.step_count,
                        self.lr, self.betas[0], self.betas[1], self.adam_eps, None if use_step else self.pidx, img,
                        None if _state is None else _state[0:1],
                        loss_in=self.out9 if self.dp else None, accum=self.accum if self.dp else None)
            if not use_step:
                self._flat_written(key, m._img)
            elif _state is not None:
                # graph capture: the lazy re-pack at the start of the next eager step is not part of a replay - the compact
                # image of the whole-step kernel is re-packed here, inside the captured sequence
                self._whole.pack(m._flat, img_c)
                self._flat_written(key, self._whole)
            else:
                self._flat_written(key)
        elif self.dp:
            self.accum += self.out9[0]

    # ------------------------------------------------------------------ HIP-graph replay of the step
    def step_graph(self, x, mask, *, epoch=1, alpha=1.0, beta=1.0, beta_annealing=False, p_missingness=30):
        """Same step, replayed from a captured HIP graph (torch.cuda.CUDAGraph): one host call per step instead
        of six kernel launches - what matters at the reference's own batch sizes (64 / 128), where the step is
        launch-bound.  Step count and Philox offsets live on the device (`state`), since kernel arguments are
        frozen in a graph.  Draws are always on the device; the first call with a new (shape, coefficients) runs
        one eager step and captures.  Under data parallelism the graph holds reduce_step -> ncclAllReduce -> adam_step
        when the bucket travels through dist.FlatAllReduce (RCCL on the compute stream); with a torch.distributed
        carrier (gloo) it falls back to step()."""
        if self.dp and not isinstance(self._collective(), dp_mod.FlatAllReduce):
            return self.step(x, mask, epoch=epoch, alpha=alpha, beta=beta, beta_annealing=beta_annealing,
                             p_missingness=p_missingness)
        L.require_cuda(x)
        x = ops._f32c(x)
        mask = as_mask_u8(mask)
        co = self.coefficients(epoch, alpha, beta, beta_annealing)
        key = (tuple(x.shape), p_missingness, bytes(co))
        kw = dict(epoch=epoch, alpha=alpha, beta=beta, beta_annealing=beta_annealing, p_missingness=p_missingness)
        self._graph_step(key, (x, mask), lambda *a, **k: self.step(*a, **kw, **k))
