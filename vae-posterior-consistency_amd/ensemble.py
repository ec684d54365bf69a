"""G independent models of one architecture stepped by ONE pair of launches.

The reference is a list of many small runs: every line of Data/imputation_args.json is batch 64 on a ~12-column table, and the
drivers wrap each line in `for missing in [...]: for alpha in [...]:` (src/experiment_main/imputation.py:21-39) around the step
loop of src/experiment_main/train.py:28-117.  The small-batch step (csrc/vpc_small.hip) gives one workgroup to each 16-row tile,
so one such model occupies 4 of the chip's compute units.  Here the members of a sweep share the launch instead:

    vpc_step_small_multi_f32     grid = tiles per member x G workgroups; workgroup (t, g) runs the tile body of the single-model
                                 kernel on member g's buffers (own parameters, data, seed, coefficients: the member table)
    vpc_reduce_step_adam_multi   the gradient reduction + loss terms + Adam + image re-pack with blockIdx.y = member

A member computes bit for bit what a stand-alone FusedTrainer with its parameters, seed, learning rate and hyperparameters
computes on its data: same tile body, same summation order, same Philox counters.

    stack_models(models)         one [G, n] buffer under the members' parameters; every model stays an ordinary module
    MemberTable                  the per-member records (loss coefficients, keep probability, lr, seed) on the host
    EnsembleTrainer              the step, the read-outs and per-member views of the stacked state
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ops
from .fused import LP
from .images import PackedImage, flat_written
from .models import Reg_VAE, loss_coefficients, vanilla_VAE
from .ops import as_mask_u8
from .trainer import draw_counters, pad_cols

# VpcMember of include/vpc.h (64 bytes): the first 32 are its VpcLossCoef, spelled flat
MEMBER_DTYPE = np.dtype([("cA", "<f4", 2), ("cE", "<f4", 2), ("bq", "<f4"), ("bp", "<f4"), ("cr", "<f4"), ("wml", "<f4"),
                         ("keep_prob", "<f4"), ("lr", "<f4"), ("seed", "<u8"), ("use_maskB", "<i4"), ("reserved", "<i4", 3)])
assert MEMBER_DTYPE.itemsize == 64
MAX_BLOCKS = 8192  # VPC_MULTI_MAX_BLOCKS of include/vpc.h: workgroups (G x tiles per member) of one ensemble launch
ROW_ALIGN = 64  # floats: every row of a stack starts on a 256-byte boundary, as a stand-alone flat buffer does


def _per_member(v, G, name):
    """Scalar or length-G sequence -> tuple of G values."""
    if isinstance(v, (int, float)):
        return (v,) * G
    v = tuple(v.tolist() if hasattr(v, "tolist") else v)
    if len(v) != G:
        raise L.VpcError(f"{name}: {len(v)} values for {G} members (a scalar or one value per member)")
    return v


def _pitch(n):
    return (n + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN


def stackable(model):
    """Can `model` be one row of a stack?  THE predicate of stack_models, EnsembleTrainer and harness.train_sweep: exactly
    Reg_VAE or vanilla_VAE (no subclass: not mask-augmented, not EDDI) on the small layouts (not wide)."""
    return type(model) in (Reg_VAE, vanilla_VAE) and not model._wide


def _require_stackable(m):
    if not stackable(m):
        if getattr(m, "mask_augm", False) or getattr(m, "_wide", False):
            raise L.VpcError("ensemble members are plain (not mask-augmented) models with obs_dim <= 128 and latent_dim <= 15")
        raise TypeError(f"EnsembleTrainer supports Reg_VAE and vanilla_VAE members, got {type(m).__name__}")


def validate_members(models, world_size=1):
    """What one ensemble can hold: stackable members of ONE class, shape and reg_type, on one process.  Raises before
    anything touches the device."""
    if world_size > 1:
        raise L.VpcError("EnsembleTrainer is single-process: data parallelism is not part of the ensemble step")
    if len(models) == 0:
        raise L.VpcError("an ensemble needs at least one member")
    for m in models:
        _require_stackable(m)
    m0 = models[0]
    for m in models[1:]:
        if type(m) is not type(m0):
            raise TypeError(f"members of one ensemble share a class: {type(m0).__name__} and {type(m).__name__}")
        a = (m.obs_dim, m.latent_dim, getattr(m, "reg_type", None))
        b = (m0.obs_dim, m0.latent_dim, getattr(m0, "reg_type", None))
        if a != b:
            raise L.VpcError(f"members of one ensemble share (obs_dim, latent_dim, reg_type): {b} and {a}")


def stack_models(models):
    """Put the trainable tensors of `models` (same parameter count, already on their device) into ONE [G, n] fp32 buffer:
    model g's tensors become views of row g in table order, so that model.flatten_parameters() returns row g through its
    fast path.  state_dict / in-place load_state_dict / the API path keep working; `.to(device)` afterwards un-stacks a
    model (stack again).  Idempotent for the same list.  Returns the [G, n] buffer (rows 256-byte aligned)."""
    models = list(models)
    if len(models) == 0:
        raise L.VpcError("an ensemble needs at least one member")
    for m in models:
        _require_stackable(m)
    first = models[0].__dict__.get("_stack")
    if first is not None and len(first[1]) == len(models) and all(a is b for a, b in zip(first[1], models)) and \
            all(m.flatten_parameters().data_ptr() == first[0][g].data_ptr() for g, m in enumerate(models)):
        return first[0]
    flats = [m.flatten_parameters() for m in models]
    n, dev = flats[0].numel(), flats[0].device
    for f in flats:
        if f.numel() != n or f.device != dev:
            raise L.VpcError("stack_models: members must have the same parameter count and sit on one device")
    stack = torch.zeros(len(models), _pitch(n), device=dev)[:, :n]
    for g, (m, f) in enumerate(zip(models, flats)):
        row = stack[g]
        row.copy_(f)
        off = 0
        for p in m.trainable():
            p.data = row[off:off + p.numel()].view_as(p)
            off += p.numel()
        m._flat = row
        m.__dict__["_view_cache"] = None
        m.__dict__["_stack"] = (stack, models)
        m.invalidate_images()
    return stack


class MemberTable:
    """Host side of the device-resident member table: one VpcMember record per member.  `update` rebuilds the rows only when
    one of its inputs changed, and reports whether any row did (then, and only then, the trainer uploads it)."""

    def __init__(self, models, lr=1e-3, seeds=None):
        self.models = list(models)
        G = len(self.models)
        self.rows = np.zeros(G, MEMBER_DTYPE)
        self.rows["lr"] = _per_member(lr, G, "lr")
        self.rows["seed"] = _per_member(range(G) if seeds is None else seeds, G, "seeds")
        self.two = not isinstance(self.models[0], vanilla_VAE)
        self.need_ml = False
        self.builds = 0  # times the rows were rebuilt
        self.version = 0  # bumped whenever a row's bytes changed
        self._inputs = None

    def update(self, epoch=1, alpha=1.0, beta=1.0, beta_annealing=False, p_missingness=30):
        G = len(self.models)
        inputs = (epoch, _per_member(alpha, G, "alpha"), _per_member(beta, G, "beta"), bool(beta_annealing),
                  _per_member(p_missingness, G, "p_missingness"))
        if inputs == self._inputs:
            return False
        _, alphas, betas_, _, pms = inputs
        rows = self.rows.copy()
        heads = rows.view(np.uint8).reshape(G, MEMBER_DTYPE.itemsize)[:, :C.sizeof(L.VpcLossCoef)]
        for g in range(G):
            co = loss_coefficients(self.models[g], epoch, alphas[g], betas_[g], beta_annealing)
            heads[g] = np.frombuffer(co, np.uint8)  # the record is the head of the row
            rows[g]["keep_prob"] = 1.0 - pms[g] / 100.0
            rows[g]["use_maskB"] = int(self.two and co.maskB_on)
        ml = rows["wml"] != 0.0
        if self.two and ml.any() != ml.all():
            # a member with wml == 0 draws two eps planes, one with wml != 0 three: they would not consume the same counters
            raise L.VpcError("members of one ensemble step must agree on whether the ml_reg term is on (wml != 0)")
        self.need_ml = bool(self.two and ml.any())
        self._inputs = inputs
        self.builds += 1
        changed = rows.tobytes() != self.rows.tobytes()
        self.rows = rows
        if changed:
            self.version += 1
        return changed


class MemberView:
    """Read access to one member's slice of the stacked state, named as a stand-alone trainer names it."""

    def __init__(self, ens, g):
        self.model = ens.models[g]
        self.grad, self.exp_avg, self.exp_avg_sq = ens.grad[g], ens.exp_avg[g], ens.exp_avg_sq[g]
        self.out9, self.accum = ens.out9[g], ens.accum[g:g + 1]


class EnsembleTrainer:
    def __init__(self, models, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seeds=None, world_size=1):
        """models: G plain Reg_VAE or G plain vanilla_VAE of one (obs_dim, latent_dim, reg_type), on the GPU.  lr and seeds:
        scalars or one value per member (seeds=None: member g draws with seed g).  The step count (Adam's bias corrections)
        and the Philox offsets are shared: every member steps in every call."""
        models = list(models)
        validate_members(models, world_size)
        self.table = MemberTable(models, lr, seeds)
        self.models = models
        self.betas, self.adam_eps = betas, eps
        self.rng_offset, self.step_count = 0, 0
        # ---- device state from here on
        self.params = stack_models(models)
        L.require_cuda(self.params)
        G, n = self.params.shape
        self.G, self.dev = G, self.params.device
        self.vanilla = isinstance(models[0], vanilla_VAE)
        self.lay = lay = models[0]._lay()
        zeros = lambda w: torch.zeros(G, _pitch(w), device=self.dev)[:, :w]
        self.grad, self.exp_avg, self.exp_avg_sq = zeros(n), zeros(n), zeros(n)
        self.row_pitch = self.params.stride(0)
        self.out9 = torch.zeros(G, 9, device=self.dev)
        self.accum = torch.zeros(G, device=self.dev)
        self.pidx, self.gidx = lay.device_tables(self.dev)
        self.inv = lay.inverse_maps(self.dev)
        # the members' fp32 weight images are rows of one stack: each stays the model's own image (images.py), so the API
        # path reads what the ensemble step re-packs
        n_img = lay.enc_img + lay.dec_img
        self.img = torch.from_numpy(lay.img_template).to(self.dev).repeat(G, 1)
        if n_img % 4:
            raise L.VpcError("weight image rows must be 16-byte multiples")
        pidx = self.pidx
        self._plists, self._row_ptr = [], []
        for g, m in enumerate(models):
            m._img = PackedImage(self.img[g], lambda flat, buf: ops.pack_weights(flat, pidx, buf))
            pl = m.trainable()
            self._plists.append(pl)
            self._row_ptr.append(self.params[g].data_ptr())
            off = 0
            for p in pl:  # .grad are views of the stacked gradient, as under a stand-alone trainer
                p.grad = self.grad[g, off:off + p.numel()].view_as(p)
                off += p.numel()
        self.table_dev = torch.zeros(G * MEMBER_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self._table_version = -1
        self.trainers = [MemberView(self, g) for g in range(G)]
        # workgroup order of the step launch (include/vpc.h): 1 = all tiles of a member on one XCD, 0 = member-major.  Same bits;
        # 1 is 3-5 % faster where the GPU is the limit and never slower from 8 members on; below 8 members its grid has
        # surplus workgroups that cost 0.3-0.8 us (profiles/ensemble_notes.md)
        self.order = 1 if G >= 8 else 0
        self._ws = None
        self._pads = {}

    # ------------------------------------------------------------------
    def _workspaces(self, B, dk):
        tiles = (B + 15) // 16
        if self._ws == (B, dk):
            return tiles
        G, lay, dev = self.G, self.lay, self.dev
        self.eps_buf = torch.empty(G, 3, B, LP, device=dev)
        self.mask_p_buf = torch.zeros(G, B, dk, dtype=torch.uint8, device=dev)
        if getattr(self, "_tiles_cap", 0) < tiles:
            self.partE = torch.empty(G, tiles * lay.enc_part, device=dev)
            self.partD = torch.empty(G, tiles * lay.dec_part, device=dev)
            self.loss_part = torch.empty(G, tiles * 8, dtype=torch.float64, device=dev)
            self._tiles_cap = tiles
        self._ws = (B, dk)
        return tiles

    def _upload_table(self):
        if self._table_version != self.table.version:
            self.table_dev.copy_(torch.from_numpy(self.table.rows.view(np.uint8).reshape(-1)))
            self._table_version = self.table.version

    # ------------------------------------------------------------------
    def step(self, x, mask, mask_p=None, eps_q=None, eps_p=None, eps_ml=None, *, epoch=1, alpha=1.0, beta=1.0,
             beta_annealing=False, p_missingness=30):
        """One training step of every member.  x, mask: [B, d] (one batch shared by all members) or [G, B, d]; alpha, beta,
        p_missingness: scalars or one value per member.  mask_p / eps_* are drawn on the device - member g with its own seed,
        in its own element space, exactly as its stand-alone trainer would - unless ALL the step's draws are injected
        ([G, ...] or shared).  No host sync: losses are in `out9[:, 0]`, the running totals in `accum`."""
        L.require_cuda(x)
        G, lay = self.G, self.lay
        d, Ld = lay.d, lay.L
        for t, name in ((x, "x"), (mask, "mask")):
            if t.dim() not in (2, 3) or t.shape[-1] != d or (t.dim() == 3 and t.shape[0] != G):
                raise L.VpcError(f"{name}: expected [B, {d}] or [{G}, B, {d}], got {tuple(t.shape)}")
        B = x.shape[-2]
        if mask.shape[-2] != B:
            raise L.VpcError("x and mask differ in their batch size")
        if B > ops.step_small_max_rows():
            raise L.VpcError(f"batch {B}: the ensemble step covers batches up to {ops.step_small_max_rows()} rows "
                             "(larger ones fill the chip on their own: FusedTrainer)")
        tiles = (B + 15) // 16
        if G * tiles > MAX_BLOCKS:
            raise L.VpcError(f"{G} members x {tiles} tiles = {G * tiles} workgroups: one ensemble launch holds {MAX_BLOCKS}")
        two = not self.vanilla
        changed = self.table.update(epoch, alpha, beta, beta_annealing, p_missingness)
        need_ml = self.table.need_ml
        given = [mask_p is not None] * two + [eps_q is not None] + [eps_p is not None] * two + [eps_ml is not None] * need_ml
        if any(given) != all(given):
            raise L.VpcError("inject all of the step's draws (mask_p, eps_q, eps_p, eps_ml as the model uses them) or none")
        draw = not any(given)
        x = ops._f32c(x)
        mask = as_mask_u8(mask)
        dk = d if d % 4 == 0 else 4 * ((d + 3) // 4)  # (the padding rule of FusedTrainer.step)
        if dk != d:
            x, mask = pad_cols(self._pads, x, dk, 0, self.dev), pad_cols(self._pads, mask, dk, 1, self.dev)
        self._workspaces(B, dk)
        if changed or self._table_version != self.table.version:
            self._upload_table()
        # every member's image is checked against its parameter key (images.py); a stale one is re-packed from its row
        keys = []
        for g, m in enumerate(self.models):
            key = m._param_key(self._plists[g])
            if key[1] != self._row_ptr[g]:
                raise L.VpcError(f"member {g} no longer sits in the ensemble's parameter stack (moved or re-flattened)")
            if m._img.key != key:
                m._images(key)
            keys.append(key)
        nplanes = 3 if need_ml else 2 if two else 1
        off_m = off_e = 0
        if draw:  # every member is an unsharded batch of B rows
            off_m, off_e, self.rng_offset, _, _ = draw_counters(self.rng_offset, two, nplanes, B, B, 0, LP, dk)
        else:
            if two:
                self.mask_p_buf[:, :, :d].copy_(as_mask_u8(mask_p))
            self.eps_buf[:, 0, :, :Ld].copy_(eps_q)
            if two:
                self.eps_buf[:, 1, :, :Ld].copy_(eps_p)
            if need_ml:
                self.eps_buf[:, 2, :, :Ld].copy_(eps_ml)
        m0 = self.models[0]
        strides = (x.stride(0) if x.dim() == 3 else 0, mask.stride(0) if mask.dim() == 3 else 0, self.mask_p_buf.stride(0),
                   self.eps_buf.stride(0), self.img.stride(0), self.partE.stride(0), self.partD.stride(0),
                   self.loss_part.stride(0), self.row_pitch)
        ops.step_small_multi_f32(x, mask, self.mask_p_buf if two else None, self.eps_buf, self.img[0, :lay.enc_img],
                                 self.img[0, lay.enc_img:], self.table_dev, G, 2 if two else 1, nplanes, draw, off_m, off_e,
                                 1.0 / B, m0._x_logvar_value, self.partE, self.partD, self.loss_part, strides, B, dk, Ld,
                                 self.order)
        self.step_count += 1
        ops.reduce_step_adam_multi(self.partE, self.partD, self.loss_part, tiles, lay.enc_part, lay.dec_part, strides,
                                   self.inv, self.table_dev, G, self.grad, B, d, self.out9, self.accum, self.params,
                                   self.exp_avg, self.exp_avg_sq, self.betas[0], self.betas[1], self.adam_eps,
                                   self.step_count, self.pidx, self.img)
        for g, m in enumerate(self.models):
            flat_written(m, self._plists[g], keys[g], (m._img,))

    # ------------------------------------------------------------------
    def loss_values(self):
        """Losses of the last step, one per member (host sync)."""
        return self.out9[:, 0].tolist()

    def epoch_total(self, reset=True):
        """Per member, the sum of train_loss over the steps since the last reset (train.py:117-118; one host sync)."""
        v = self.accum.tolist()
        if reset:
            self.accum.zero_()
        return v
