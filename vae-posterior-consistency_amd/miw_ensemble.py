"""G MIWAE or G Reg_MIWAE models of one shape stepped by ONE launch set: the ensemble form of MIWTrainer's small-batch step.

The reference's run list (Data/imputation_args.json) opens with reg_MIWAE1..3 and vanilla_MIWAE1..3, each batch 64 on a
12-column table under the drivers' loops `for missing: for alpha:` (src/experiment_main/imputation.py:21-39).  One such step
is seven launches that occupy at most half of the chip and are paced by the host (miwae.MIWTrainer._step_small).  Here the
members of a sweep share those seven launches, whatever G:

    vpc_miw_multi_prep          mask_p draw + stacked encoder input + every eps plane, member g with seed_g, keep_prob_g
    vpc_miw_small_fwd_multi     grid = ceil(R / rb) x G workgroups, workgroup (u, g) = the stand-alone body on member g
    vpc_miw_loss_multi          the loss's three launches with a member axis, alpha_g
    vpc_miw_small_bwd_multi     blocks_per_member workgroups per member, each walking that member's row blocks
    vpc_miw_small_tail_multi    a member's partial blocks summed in block order, flat Adam with lr_g

A member computes bit for bit what a stand-alone MIWTrainer(seed=seed_g, lr=lr_g) on the small path with small_rb = rb
computes whenever blocks_per_member >= ceil(R / rb) <= compute units (same body, same partial blocks, same order); with
fewer blocks per member only the summation order of the weight gradients differs.  fp32, no host synchronisation, no float
atomics, bit-reproducible.

    default_blocks(G, R, n_cu)   the (rb, blocks_per_member) rule, from measurement (profiles/miw_ensemble_notes.md)
    partial_floats(G, blocks, n) the size rule of the partial buffer
    MIWEnsembleTrainer           the step, the read-outs and per-member views of the stacked state
    sweep_key                    how harness.train_sweep groups MIWAE-path members
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._lib import VpcError, check, lib, ptr, stream_ptr
from .ensemble import _per_member, _pitch, _shared_or_per_member, stack_models
from .linear import _f32c
from .miwae import (HID, PAIR_REFERENCE, SMALL_MAX_D, SMALL_MAX_L, MIWAE, Reg_MIWAE, small_max_rows,
                    small_step_route)
from .trainer import chain_draw_increment

# VpcMiwMember of include/vpc.h (24 bytes)
MEMBER_DTYPE = np.dtype([("seed", "<u8"), ("alpha", "<f4"), ("keep_prob", "<f4"), ("lr", "<f4"), ("reserved", "<i4")])
assert MEMBER_DTYPE.itemsize == 24
MAX_BLOCKS = 65536  # VPC_MIW_MULTI_MAX_BLOCKS: workgroups of the forward or of the backward launch
MAX_MEMBERS = 4096  # VPC_MIW_MULTI_MAX_MEMBERS
MAX_RB = 4  # rows of the stacked passes per workgroup (csrc/vpc_miw_chain.h)
# The limit of the partial buffer [G][blocks_per_member][n_params], in floats (1 GiB).  It is written once and read once
# per step, so long before this limit it is the step's largest memory stream: G = 64 at the wine shape (n = 43 320) is
# 355 MB with 32 blocks per member and 44 MB with 4.
PART_MAX_FLOATS = 1 << 28
LAUNCHES = ("vpc_miw_multi_prep", "vpc_miw_small_fwd_multi", "vpc_miw_loss_multi", "vpc_miw_small_bwd_multi",
            "vpc_miw_small_tail_multi")


def n_params(d, Ld):
    """Floats of the flat parameter buffer (MiwOff of csrc/vpc_miw_chain.h): 43 320 at d = 12, L = 10."""
    return (d * HID + HID) + (HID * HID + HID) + (HID * 2 * Ld + 2 * Ld) + (Ld * HID + HID) + (HID * HID + HID) + \
        (HID * 3 * d + 3 * d)


def partial_floats(G, blocks_per_member, n):
    """Floats of the partial buffer: one block of all n parameters per (member, workgroup of the backward kernel)."""
    return int(G) * int(blocks_per_member) * int(n)


def default_blocks(G, R, n_cu, rb=None):
    """(rb, blocks_per_member) of an ensemble of G members with R rows of the stacked passes each, on n_cu compute units (rb
    given: the blocks for that rb).
    Measured, not derived (profiles/miw_ensemble_notes.md, the wine shape B = 64, S = 20, d = 12, L = 10, 256 compute units):

      * rb: as the stand-alone step chooses it from ALL the rows in the launch - the smallest of 1, 2, 4 that leaves at
        most one workgroup per compute unit over G * R rows, 4 beyond;
      * blocks_per_member: the backward kernel's workgroups fill the chip once - ceil(n_cu / G), at most the member's row
        blocks and the compute units.  Every further block is one more copy of all parameters written by the backward and
        read by the tail."""
    G, R, n_cu = max(int(G), 1), max(int(R), 1), max(int(n_cu), 1)
    rows = G * R
    if rb is None:
        rb = 1 if rows <= n_cu else 2 if rows <= 2 * n_cu else 4
    units = -(-R // rb)
    return rb, max(1, min(-(-n_cu // G), units, n_cu))


def _require_miw(m):
    if type(m) not in (MIWAE, Reg_MIWAE):
        raise TypeError(f"MIWEnsembleTrainer supports MIWAE and Reg_MIWAE members, got {type(m).__name__}")
    if not (0 < m.obs_dim <= SMALL_MAX_D and 0 < m.latent_dim <= SMALL_MAX_L):
        raise VpcError(f"MIWAE ensemble members have obs_dim <= {SMALL_MAX_D} and latent_dim <= {SMALL_MAX_L} (the small-batch "
                       f"step's limits): got {m.obs_dim}, {m.latent_dim}")


def validate_members(models, world_size=1):
    """What one ensemble can hold: MIWAE or Reg_MIWAE members of ONE class and (obs_dim, latent_dim, num_samples) within the
    small-batch step's widths, on one process.  Raises before anything touches the device."""
    if world_size != 1:
        raise VpcError("MIWEnsembleTrainer is single-process: the reference's row/sample pairing couples rows across the "
                       "global batch (no data-parallel form without an all-gather)")
    if len(models) == 0:
        raise VpcError("an ensemble needs at least one member")
    if len(models) > MAX_MEMBERS:
        raise VpcError(f"{len(models)} members: one ensemble holds {MAX_MEMBERS}")
    for m in models:
        _require_miw(m)
    m0 = models[0]
    shape = lambda m: (m.obs_dim, m.latent_dim, m.num_samples)
    for m in models[1:]:
        if type(m) is not type(m0):
            raise TypeError(f"members of one ensemble share a class: {type(m0).__name__} and {type(m).__name__}")
        if shape(m) != shape(m0):
            raise VpcError(f"members of one ensemble share (obs_dim, latent_dim, num_samples): {shape(m0)} and {shape(m)}")


def sweep_key(model, vae_type, loader, obs_dim, max_rows=None):
    """The group of harness.train_sweep that `model` steps in - ("miw", class, obs_dim, latent_dim, num_samples) - or None:
    a 'with_drop' run (train()'s loop thins its mask with a drop mask of its own at every step), not a MIWAE-path model, a
    width past the small-batch step, or a first batch that small_step_route does not take at max_rows decoder rows (None:
    small_max_rows(), VPC_MIW_SMALL in the environment).  With the small step switched off (unset, or 0) nothing is routed
    and the loader is not touched."""
    max_rows = small_max_rows() if max_rows is None else max_rows
    if max_rows <= 0 or "with_drop" in vae_type:
        return None
    try:
        _require_miw(model)
    except (TypeError, VpcError):
        return None
    first = next(iter(loader), None)
    if first is None:
        return None
    B = first[0].reshape(-1, obs_dim).shape[0]
    P = 2 if model.regularised else 1
    if not small_step_route(model.obs_dim, model.latent_dim, B, model.num_samples, P, max_rows):
        return None
    return ("miw", type(model), model.obs_dim, model.latent_dim, model.num_samples)


class MIWMemberView:
    """Read access to one member's slice of the stacked state, named as a stand-alone MIWTrainer names it."""

    def __init__(self, ens, g):
        self._ens, self._g = ens, g
        self.model = ens.models[g]
        self.grad, self.exp_avg, self.exp_avg_sq = ens.grad[g], ens.exp_avg[g], ens.exp_avg_sq[g]
        self.out8, self.accum, self.tail = ens.out8[g], ens.accum[g:g + 1], ens.loss_f32[g:g + 1]

    # the workspaces are rebuilt when the batch size changes: read through the ensemble
    mask_p = property(lambda self: self._ens.mask_p[self._g])
    eps = property(lambda self: self._ens.eps[self._g])
    rng_offset = property(lambda self: self._ens.rng_offset)
    step_count = property(lambda self: self._ens.step_count)

    def loss_value(self):
        return float(self.tail[0].item())


class MIWEnsembleTrainer:
    def __init__(self, models, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seeds=None, rb=None, blocks_per_member=None,
                 world_size=1):
        """models: G MIWAE or G Reg_MIWAE of one (obs_dim <= 32, latent_dim <= 16, num_samples), on the GPU.  lr and seeds:
        scalars or one value per member (seeds=None: member g draws with seed g).  The step count (Adam's bias corrections)
        and the Philox offsets are shared: every member steps in every call.
        rb (1, 2 or 4): rows of the stacked passes per workgroup; blocks_per_member: the most workgroups of the backward
        kernel per member (a step uses min(blocks_per_member, ceil(R / rb), compute units)).  None: default_blocks, per
        batch size.  `rb` and `blocks_per_member` hold what the last step used.  The partial buffer has
        G x blocks_per_member x n_params floats (partial_floats); beyond PART_MAX_FLOATS the step raises VpcError before
        it launches anything."""
        models = list(models)
        validate_members(models, world_size)
        if rb is not None and rb not in (1, 2, 4):
            raise VpcError(f"rb = {rb}: a workgroup owns 1, 2 or 4 rows of the stacked passes")
        if blocks_per_member is not None and blocks_per_member < 1:
            raise VpcError(f"blocks_per_member = {blocks_per_member} < 1")
        G = len(models)
        lrs, seeds = _per_member(lr, G, "lr"), _per_member(range(G) if seeds is None else seeds, G, "seeds")
        self.rows = np.zeros(G, MEMBER_DTYPE)
        self.rows["lr"], self.rows["seed"] = lrs, seeds
        self.models, self.G = models, G
        self.reg = models[0].regularised
        self.betas, self.adam_eps = betas, eps
        self.rng_offset = self.step_count = 0
        self._rb, self._bpm = rb, blocks_per_member
        self.rb = self.blocks_per_member = None
        self.last_launches = ()
        # ---- device state from here on
        self.params = stack_models(models, _require_miw)
        L.require_cuda(self.params)
        self.dev = self.params.device
        n = self.n = self.params.shape[1]
        zeros = lambda w: torch.zeros(G, _pitch(w), device=self.dev)[:, :w]
        self.grad, self.exp_avg, self.exp_avg_sq = zeros(n), zeros(n), zeros(n)
        self.row_pitch = self.params.stride(0)
        self.out8 = torch.zeros(G, 8, dtype=torch.float64, device=self.dev)
        self.loss_f32 = torch.zeros(G, device=self.dev)
        self.accum = torch.zeros(G, device=self.dev)
        self.table_dev = torch.zeros(G * MEMBER_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self._table_bytes = None
        self._plists = [m.trainable() for m in models]
        self._row_ptr = [self.params[g].data_ptr() for g in range(G)]
        for g, pl in enumerate(self._plists):
            off = 0
            for p in pl:  # .grad are views of the stacked gradient, as under a stand-alone trainer
                p.grad = self.grad[g, off:off + p.numel()].view_as(p)
                off += p.numel()
        self.n_cu = L.max_blocks() // 2
        # workgroup order of the forward and backward launches (include/vpc.h): 1 = all workgroups of a member on one XCD,
        # 0 = member-major.  Same bits; the choice is measured (profiles/miw_ensemble_notes.md)
        self.order = 1 if G >= 8 else 0
        self._part = None
        self._B = None
        self.trainers = [MIWMemberView(self, g) for g in range(G)]

    # ------------------------------------------------------------------
    def _workspaces(self, B):
        """Every member's stand-alone workspace as one dense [G][..] stack; rebuilt when B changes (an epoch's last batch)."""
        if self._B == B:
            return
        m, G, dev = self.models[0], self.G, self.dev
        d, Ld, S = m.obs_dim, m.latent_dim, m.num_samples
        P = 2 if self.reg else 1
        R, M = P * B, P * B * S
        e = lambda *s: torch.empty(G, *s, device=dev)
        self.xin, self.mask_p = e(R, d), (e(B, d) if self.reg else None)
        self.h1, self.h2, self.heads, self.hact = e(R, HID), e(R, HID), e(R, 2 * Ld), e(R, 2 * Ld)
        self.eps = e(2 * P, B, S, Ld)  # per member: the sampling draws of the P passes, then the loss-time draws
        self.z, self.g1, self.g2, self.Y = e(M, Ld), e(M, HID), e(M, HID), e(M, 3 * d)
        self.Gy, self.gh, self.dht = e(M, 3 * d), e(R, 2 * Ld), e(R, 2 * Ld)
        one = (int(lib().vpc_miw_loss_scratch(B, S)) + 7) // 8  # doubles of one member's scratch (a multiple of 64 bytes)
        self.scratch = torch.empty(G * one, dtype=torch.float64, device=dev)
        self._B = B

    def _blocks(self, R):
        """(rb, blocks per member) of a step on R rows of the stacked passes per member."""
        rb, bpm = default_blocks(self.G, R, self.n_cu, self._rb)
        if self._bpm is not None:
            bpm = self._bpm
        return rb, max(1, min(bpm, -(-R // rb), self.n_cu))

    def _sync_table(self, alpha, p_missingness):
        G = self.G
        self.rows["alpha"] = _per_member(alpha, G, "alpha")
        self.rows["keep_prob"] = [1.0 - p / 100.0 for p in _per_member(p_missingness, G, "p_missingness")]
        b = self.rows.tobytes()
        if b != self._table_bytes:  # THE upload of the member table: whenever a row changed since the last one
            self.table_dev.copy_(torch.from_numpy(self.rows.view(np.uint8).reshape(-1)))
            self._table_bytes = b

    def step(self, x, mask, mask_p=None, eps=None, *, alpha=1.0, p_missingness=30):
        """One optimiser step of every member.  x, mask: [B, d] (one batch shared by all members) or [G, B, d]; alpha and
        p_missingness: scalars or one value per member.  mask_p ([B, d] or [G, B, d]; Reg_MIWAE) and eps ([2 P, B, S, L] or
        [G, 2 P, B, S, L]: forward q, forward p, loss q, loss p for Reg_MIWAE; forward, loss for MIWAE) are drawn on the
        device - member g with its own seed, exactly as its stand-alone trainer would - unless ALL of them are injected.
        No host sync: losses are in `loss_f32` / `out8[:, 0]`, the running totals in `accum`."""
        L.require_cuda(x, mask, mask_p, eps)
        m0, G = self.models[0], self.G
        d, Ld, S = m0.obs_dim, m0.latent_dim, m0.num_samples
        sx = _shared_or_per_member(x, "x", G, (None, d))
        B = x.shape[-2]
        sm = _shared_or_per_member(mask, "mask", G, (B, d), " (x and mask agree in their rows)")
        reg = self.reg
        P = 2 if reg else 1
        R = P * B
        given = [mask_p is not None] * reg + [eps is not None]
        if any(given) != all(given) or (not reg and mask_p is not None):
            raise VpcError("inject all of the step's draws (mask_p for Reg_MIWAE, and eps) or none")
        draw = not any(given)
        if not draw:
            if reg:
                _shared_or_per_member(mask_p, "mask_p", G, (B, d))
            _shared_or_per_member(eps, "eps", G, (2 * P, B, S, Ld))
        if R * S > (1 << 24):
            raise VpcError(f"{R * S} decoder rows per member: the small-batch step holds {1 << 24}")
        rb, bpm = self._blocks(R)
        units = -(-R // rb)
        if units * G > MAX_BLOCKS:
            raise VpcError(f"{G} members x {units} row blocks = {units * G} workgroups: one ensemble launch holds {MAX_BLOCKS}")
        need = partial_floats(G, bpm, self.n)
        if need > PART_MAX_FLOATS:
            raise VpcError(f"partial buffer of {G} members x {bpm} blocks x {self.n} parameters = {need} floats: the limit is "
                           f"{PART_MAX_FLOATS} (lower blocks_per_member)")
        for g, mdl in enumerate(self.models):
            if mdl.flatten_parameters().data_ptr() != self._row_ptr[g]:
                raise VpcError(f"member {g} no longer sits in the ensemble's parameter stack (moved or re-flattened)")
        xf, mf = _f32c(x), _f32c(mask)
        self._workspaces(B)
        if self._part is None or self._part.numel() < need:
            self._part = torch.empty(need, device=self.dev)
        self._sync_table(alpha, p_missingness)
        self.rb, self.blocks_per_member = rb, bpm
        if not draw:
            if reg:
                self.mask_p.copy_(mask_p)
            self.eps.copy_(eps)
        st, mem, lb = stream_ptr(), ptr(self.table_dev), lib()
        mp = ptr(self.mask_p)
        called = []

        def run(name, *args):  # one library entry: called, checked, recorded
            check(getattr(lb, name)(*args), name)
            called.append(name)

        run("vpc_miw_multi_prep", ptr(xf), sx, ptr(mf), sm, mp, ptr(self.xin), ptr(self.eps), mem, G, int(draw), B, S, d, Ld,
            self.rng_offset, self.rng_offset + (1 << 40), st)
        self.rng_offset += chain_draw_increment(2 * P * B * S * Ld, B, d)
        prm, order = ptr(self.params), self.order
        run("vpc_miw_small_fwd_multi", prm, self.row_pitch, ptr(self.xin), ptr(self.eps), ptr(self.h1), ptr(self.h2),
            ptr(self.heads), ptr(self.hact), ptr(self.z), ptr(self.g1), ptr(self.g2), ptr(self.Y), G, R, S, d, Ld, rb, order, st)
        run("vpc_miw_loss_multi", ptr(xf), sx, ptr(mf), sm, mp, ptr(self.Y), ptr(self.hact), ptr(self.eps), ptr(self.Gy),
            ptr(self.gh), ptr(self.scratch), self.scratch.numel() * 8, ptr(self.out8), ptr(self.loss_f32), ptr(self.accum), mem,
            G, B, S, d, Ld, PAIR_REFERENCE, st)
        run("vpc_miw_small_bwd_multi", prm, self.row_pitch, ptr(self.xin), ptr(self.eps), ptr(self.h1), ptr(self.h2),
            ptr(self.heads), ptr(self.z), ptr(self.g1), ptr(self.g2), ptr(self.Gy), ptr(self.gh), ptr(self.dht), ptr(self._part),
            self._part.numel(), G, bpm, R, S, d, Ld, rb, order, st)
        self.step_count += 1
        run("vpc_miw_small_tail_multi", ptr(self._part), self._part.numel(), G, bpm, d, Ld, ptr(self.grad), prm,
            ptr(self.exp_avg), ptr(self.exp_avg_sq), self.row_pitch, mem, self.betas[0], self.betas[1], self.adam_eps,
            self.step_count, st)
        self.last_launches = tuple(called)  # the library entries this step called, in order
        for mdl in self.models:  # the launch wrote the flat parameters behind torch's back (images.py)
            mdl.invalidate_images()

    # ------------------------------------------------------------------
    def loss_values(self):
        """Losses of the last step, one per member (host sync)."""
        return self.loss_f32.tolist()

    def epoch_total(self, reset=True):
        """Per member, the sum of train_loss over the steps since the last reset (train.py:117-118; one host sync)."""
        v = self.accum.tolist()
        if reset:
            self.accum.zero_()
        return v
