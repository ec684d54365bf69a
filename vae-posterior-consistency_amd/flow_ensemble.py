"""G VAEFlow or G REG_VAEFlow models of one shape stepped by ONE launch set: the ensemble form of FlowTrainer's few-row step.

The reference's run list (Data/imputation_args.json:7-12) holds vanilla_flow1..3 and reg_flow1..3, each batch 64 on a 12-column
table under the drivers' loops `for missing: for alpha:` (src/experiment_main/imputation.py:21-39).  One such step is 22
dependent launches of at most 128 workgroups each (flow.FlowTrainer._step_small; profiles/flow_small_notes.md): it is paced
by launch latency and leaves half of the chip idle.  Here the members of a sweep share those 22 launches, whatever G:

    vpc_flow_multi_prep     mask_p draw + stacked encoder input + eps, member g with seed_g and keep_prob_g
    vpc_rows_fwd_multi      3 encoder layers, the flow (vpc_flow_fwd_multi) and 5 decoder layers: grid = one member's x G
    vpc_flow_loss_multi     the loss's two launches with a member axis, alpha_g and beta_g
    vpc_rows_bwd_multi      5 decoder layers, the flow backward (vpc_flow_bwd_multi) and 3 encoder layers; every launch writes
                            the members' complete weight gradients into the stacked flat gradient
    vpc_adam_step_multi     flat Adam over [G][n] with lr_g

Every kernel runs the stand-alone kernel's body on member g's arrays, so member g computes bit for bit what a stand-alone
FlowTrainer(model_g, lr=lr_g, seed=seed_g) on the small path (VPC_FLOW_SMALL=128) computes - loss, gradients, Adam state,
parameters, draws and epoch total, at every step and whatever G.  fp32, no host synchronisation, no atomics.

    workspace_floats(G, R, B, d, hid, reg)   the size rule of the activation workspaces
    FlowEnsembleTrainer                      the step, the read-outs and per-member views of the stacked state
    sweep_key                                how harness.train_sweep groups flow members
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from ._lib import VpcError, check, lib, ptr, stream_ptr
from .ensemble import _per_member, _pitch, _shared_or_per_member, stack_models
from .flow import (CTX, FLOW_L, REG_VAEFlow, SMALL_MAX_ROWS, SMALL_MAX_WIDTH, STAGE_EVAL, STAGE_TRAIN, VAEFlow, small_max_rows,
                   small_step_route)
from .linear import ACT_NONE, _f32c
from .trainer import chain_draw_increment

# VpcFlowMember of include/vpc.h (32 bytes)
MEMBER_DTYPE = np.dtype([("seed", "<u8"), ("alpha", "<f4"), ("beta", "<f4"), ("keep_prob", "<f4"), ("lr", "<f4"),
                         ("reserved", "<i4", (2,))])
assert MEMBER_DTYPE.itemsize == 32
MAX_MEMBERS = 4096  # VPC_FLOW_MULTI_MAX_MEMBERS
# The limit of the activation workspaces of one ensemble, in floats (1 GiB): a member holds about 3 MB at hid 500, R = 128, so
# 64 members hold 207 MB and the member limit of 4096 would hold 13 GB.
WORKSPACE_MAX_FLOATS = 1 << 28
# The entries of one step, in order: 21 calls, 22 launches (the loss is two), whatever G
LAUNCHES = ("vpc_flow_multi_prep",) + ("vpc_rows_fwd_multi",) * 3 + ("vpc_flow_fwd_multi",) + ("vpc_rows_fwd_multi",) * 5 + \
    ("vpc_flow_loss_multi",) + ("vpc_rows_bwd_multi",) * 5 + ("vpc_flow_bwd_multi",) + ("vpc_rows_bwd_multi",) * 3 + \
    ("vpc_adam_step_multi",)
# The smallest group harness.train_sweep steps through FlowEnsembleTrainer: a group of two already beat two stand-alone steps
# back to back (profiles/flow_ensemble_notes.md, G = 2 at the wine shape, REG and vanilla)
MIN_GROUP = 2


def _pad4(n):
    """A member slice rounded up to a multiple of 4 floats: the stride rule of vpc_rows_*_multi (include/vpc.h)."""
    return (int(n) + 3) // 4 * 4


def _row_widths(d, hid):
    """Widths of a member's arrays on the R stacked rows: xin; eps, z, zlp, gz, gzlp, dzd; t, dt; h1, h2, dh1, dh2 and the
    four decoder activations and their gradients; Y, G."""
    return (2 * d,) + (FLOW_L,) * 6 + (CTX,) * 2 + (hid,) * 12 + (d,) * 2


def workspace_floats(G, R, B, d, hid, reg):
    """Floats of the activation workspaces of G members with R = P * B stacked rows each: every array of FlowTrainer's
    workspace as a dense [G][..] stack whose member slices are padded to a multiple of 4 floats, and mask_p [B][d] for
    REG_VAEFlow.  (The loss partials - 64 bytes per 4 data rows and member - are not counted.)"""
    per = sum(_pad4(R * w) for w in _row_widths(d, hid)) + (_pad4(B * d) if reg else 0)
    return int(G) * per


def _require_flow(m):
    if type(m) not in (VAEFlow, REG_VAEFlow):
        raise TypeError(f"FlowEnsembleTrainer supports VAEFlow and REG_VAEFlow members, got {type(m).__name__}")
    if not (0 < 2 * m.obs_dim <= SMALL_MAX_WIDTH and 0 < m.hid_dim <= SMALL_MAX_WIDTH):
        raise VpcError(f"flow ensemble members have 2 * obs_dim <= {SMALL_MAX_WIDTH} and hid_dim <= {SMALL_MAX_WIDTH} (the "
                       f"few-row layer ops' limits): got obs_dim {m.obs_dim}, hid_dim {m.hid_dim}")


def validate_members(models, world_size=1):
    """What one ensemble can hold: VAEFlow or REG_VAEFlow members of ONE class and (obs_dim, hid_dim) within the few-row layer
    ops' widths, on one process.  Raises before anything touches the device."""
    if world_size != 1:
        raise VpcError("FlowEnsembleTrainer is single-process: the flow's torch.any(inside) is a predicate over the whole batch "
                       "(no data-parallel form without a cross-rank vote)")
    if len(models) == 0:
        raise VpcError("an ensemble needs at least one member")
    if len(models) > MAX_MEMBERS:
        raise VpcError(f"{len(models)} members: one ensemble holds {MAX_MEMBERS}")
    for m in models:
        _require_flow(m)
    m0 = models[0]
    shape = lambda m: (m.obs_dim, m.hid_dim)
    for m in models[1:]:
        if type(m) is not type(m0):
            raise TypeError(f"members of one ensemble share a class: {type(m0).__name__} and {type(m).__name__}")
        if shape(m) != shape(m0):
            raise VpcError(f"members of one ensemble share (obs_dim, hid_dim): {shape(m0)} and {shape(m)}")


def sweep_key(model, vae_type, loader, obs_dim, max_rows=None):
    """The group of harness.train_sweep that `model` steps in - ("flow", class, obs_dim, hid_dim) - or None: the few-row step is
    switched off (max_rows None: flow.small_max_rows(), VPC_FLOW_SMALL in the environment; unset or 0 - then the loader is
    not touched), a 'with_drop' run (train()'s loop thins its mask with a drop mask of its own at every step), not a flow
    model, or a first batch that flow.small_step_route does not take at max_rows stacked rows."""
    max_rows = small_max_rows() if max_rows is None else max_rows
    if max_rows <= 0 or "with_drop" in vae_type:
        return None
    try:
        _require_flow(model)
    except (TypeError, VpcError):
        return None
    first = next(iter(loader), None)
    if first is None:
        return None
    B = first[0].reshape(-1, obs_dim).shape[0]
    if not small_step_route((2 if model.regularised else 1) * B, model.obs_dim, model.hid_dim, max_rows):
        return None
    return ("flow", type(model), model.obs_dim, model.hid_dim)


class FlowMemberView:
    """Read access to one member's slice of the stacked state, named as a stand-alone FlowTrainer names it."""

    def __init__(self, ens, g):
        self._ens, self._g = ens, g
        self.model = ens.models[g]
        self.grad, self.exp_avg, self.exp_avg_sq = ens.grad[g], ens.exp_avg[g], ens.exp_avg_sq[g]
        self.out8, self.accum, self.tail = ens.out8[g], ens.accum[g:g + 1], ens.loss_f32[g:g + 1]

    # the workspaces are rebuilt when the batch size changes: read through the ensemble
    mask_p = property(lambda self: self._ens.mask_p[self._g])
    eps = property(lambda self: self._ens.eps[self._g])
    z = property(lambda self: self._ens.z[self._g])
    zlp = property(lambda self: self._ens.zlp[self._g])
    rng_offset = property(lambda self: self._ens.rng_offset)
    step_count = property(lambda self: self._ens.step_count)

    def loss_value(self):
        return float(self.tail[0].item())


class FlowEnsembleTrainer:
    def __init__(self, models, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seeds=None, order=None, world_size=1):
        """models: G VAEFlow or G REG_VAEFlow of one (obs_dim, hid_dim), 2 * obs_dim and hid_dim <= 1024, on the GPU.  lr and
        seeds: scalars or one value per member (seeds=None: member g draws with seed g).  The step count (Adam's bias
        corrections) and the Philox offsets are shared: every member steps in every call.
        order: the workgroup order of the layer launches (include/vpc.h, vpc_rows_fwd_multi: 0 member-major, 1 a member on one
        XCD; same bits); None: the measured default (profiles/flow_ensemble_notes.md)."""
        models = list(models)
        validate_members(models, world_size)
        if order not in (None, 0, 1):
            raise VpcError(f"order = {order}: 0 (member-major) or 1 (a member's workgroups on one XCD)")
        G = len(models)
        lrs, seeds = _per_member(lr, G, "lr"), _per_member(range(G) if seeds is None else seeds, G, "seeds")
        self.rows = np.zeros(G, MEMBER_DTYPE)
        self.rows["lr"], self.rows["seed"] = lrs, seeds
        self.models, self.G = models, G
        self.reg = models[0].regularised
        self.betas, self.adam_eps = betas, eps
        self.rng_offset = self.step_count = 0
        self.last_launches = ()
        # ---- device state from here on
        self.params = stack_models(models, _require_flow)
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
        # member 0's layers and gradient views: every member's lie row_pitch floats further per member
        m0 = models[0]
        self.enc_layers, self.dec_layers = m0._chains()
        g0 = m0._named_views(self.grad[0])
        pairs = lambda names: [(g0[w], g0[b]) for w, b in zip(names[0::2], names[1::2])]
        self._enc_grads, self._dec_grads = pairs(m0._ENC_NAMES), pairs(m0._DEC_NAMES)
        # 1 = all workgroups of a member on one XCD (its weights re-read through one L2): measured faster from G = 8 on
        self.order = (1 if G >= 8 else 0) if order is None else order
        self._B = None
        self.trainers = [FlowMemberView(self, g) for g in range(G)]

    # ------------------------------------------------------------------
    def _workspaces(self, B):
        """Every member's stand-alone workspace (FlowTrainer._buffers) as one [G][rows][width] stack whose member slices are
        padded to a multiple of 4 floats; rebuilt when B changes (an epoch's last batch)."""
        if self._B == B:
            return
        m, G, dev = self.models[0], self.G, self.dev
        d, H = m.obs_dim, m.hid_dim
        R = (2 if self.reg else 1) * B

        def e(rows, w):  # .stride(0) is the member stride the kernels take
            return torch.empty(G, _pad4(rows * w), device=dev)[:, :rows * w].view(G, rows, w)

        self.xin, self.mask_p, self.eps = e(R, 2 * d), (e(B, d) if self.reg else None), e(R, FLOW_L)
        self.h1, self.h2, self.t = e(R, H), e(R, H), e(R, CTX)
        self.z, self.zlp = e(R, FLOW_L), e(R, FLOW_L)
        self.gd = [e(R, H) for _ in range(4)]
        self.Y, self.Gy = e(R, d), e(R, d)
        self.gz, self.gzlp, self.dzd = e(R, FLOW_L), e(R, FLOW_L), e(R, FLOW_L)
        self.dgd = [e(R, H) for _ in range(4)]
        self.dt, self.dh2, self.dh1 = e(R, CTX), e(R, H), e(R, H)
        self.scratch = torch.empty((int(lib().vpc_flow_loss_multi_scratch(G, B)) + 7) // 8, dtype=torch.float64, device=dev)
        self.enc_acts, self.enc_dacts = [self.xin, self.h1, self.h2, self.t], [None, self.dh1, self.dh2, self.dt]
        self.dec_acts, self.dec_dacts = [self.z, *self.gd, self.Y], [self.dzd, *self.dgd, self.Gy]
        self._B = B

    def _sync_table(self, alpha, beta, p_missingness):
        G = self.G
        self.rows["alpha"], self.rows["beta"] = _per_member(alpha, G, "alpha"), _per_member(beta, G, "beta")
        self.rows["keep_prob"] = [1.0 - p / 100.0 for p in _per_member(p_missingness, G, "p_missingness")]
        b = self.rows.tobytes()
        if b != self._table_bytes:  # THE upload of the member table: whenever a row changed since the last one
            self.table_dev.copy_(torch.from_numpy(self.rows.view(np.uint8).reshape(-1)))
            self._table_bytes = b

    def step(self, x, mask, mask_p=None, eps=None, *, alpha=1.0, beta=1.0, p_missingness=30, stage="train"):
        """One optimiser step of every member.  x, mask: [B, d] (one batch shared by all members) or [G, B, d]; alpha, beta and
        p_missingness: scalars or one value per member.  mask_p ([B, d] or [G, B, d]; REG_VAEFlow) and eps ([P, B, 10] or
        [G, P, B, 10]: the q pass, then the p pass) are drawn on the device - member g with its own seed, exactly as its
        stand-alone trainer would - unless ALL of them are injected.  R = P * B <= 128 stacked rows.  No host sync: losses are
        in `loss_f32` / `out8[:, 0]`, the running totals in `accum`."""
        L.require_cuda(x, mask, mask_p, eps)
        m0, G = self.models[0], self.G
        d, H = m0.obs_dim, m0.hid_dim
        sx = _shared_or_per_member(x, "x", G, (None, d))
        B = x.shape[-2]
        sm = _shared_or_per_member(mask, "mask", G, (B, d), " (x and mask agree in their rows)")
        reg = self.reg
        P = 2 if reg else 1
        R = P * B
        given = [mask_p is not None] * reg + [eps is not None]
        if any(given) != all(given) or (not reg and mask_p is not None):
            raise VpcError("inject all of the step's draws (mask_p for REG_VAEFlow, and eps) or none")
        draw = not any(given)
        if not draw:
            if reg:
                _shared_or_per_member(mask_p, "mask_p", G, (B, d))
            se = _shared_or_per_member(eps, "eps", G, (P, B, FLOW_L))
        if not small_step_route(R, d, H, SMALL_MAX_ROWS):
            raise VpcError(f"{R} stacked rows per member: the few-row step holds {SMALL_MAX_ROWS} (R = P * B)")
        if stage not in ("train", "evaluate"):
            raise VpcError(f"stage = {stage!r}: 'train' or 'evaluate'")
        need = workspace_floats(G, R, B, d, H, reg)
        if need > WORKSPACE_MAX_FLOATS:
            raise VpcError(f"workspaces of {G} members x {R} rows = {need} floats: the limit is {WORKSPACE_MAX_FLOATS}")
        for g, mdl in enumerate(self.models):
            if mdl.flatten_parameters().data_ptr() != self._row_ptr[g]:
                raise VpcError(f"member {g} no longer sits in the ensemble's parameter stack (moved or re-flattened)")
        xf, mf = _f32c(x), _f32c(mask)
        self._workspaces(B)
        self._sync_table(alpha, beta, p_missingness)
        if not draw:
            if reg:
                self.mask_p.copy_(mask_p)
            self.eps.copy_(eps.reshape(G, R, FLOW_L) if se else eps.reshape(R, FLOW_L))
        st, mem, lb, order = stream_ptr(), ptr(self.table_dev), lib(), self.order
        pitch, s10 = self.row_pitch, self.eps.stride(0)
        called = []

        def run(name, *args):  # one library entry: called, checked, recorded
            check(getattr(lb, name)(*args), name)
            called.append(name)

        def fwd(layers, acts):  # linear.chain_fwd_rows with a member axis
            for i, (w, b, K, N, act, split) in enumerate(layers):
                xa, ya = acts[i], acts[i + 1]
                run("vpc_rows_fwd_multi", ptr(xa), K, xa.stride(0), ptr(w), ptr(b), pitch, ptr(ya), N, ya.stride(0), G, R, N, K,
                    act, split, order, st)

        def bwd(layers, acts, dacts, grads, input_grad):  # linear.chain_bwd_rows with a member axis (no output gate)
            for i in range(len(layers) - 1, -1, -1):
                w, _, K, N, _, _ = layers[i]
                dw, db = grads[i]
                dy, xa = dacts[i + 1], acts[i]
                dx = dacts[i] if (i > 0 or input_grad) else None
                x_out, act_prev = (xa, layers[i - 1][4]) if i > 0 else (None, ACT_NONE)
                run("vpc_rows_bwd_multi", ptr(dy), N, dy.stride(0), None, N, 0, ACT_NONE, 0, ptr(w), ptr(xa), K, xa.stride(0),
                    ptr(x_out), K, xa.stride(0) if x_out is not None else 0, act_prev, ptr(dx), K,
                    dx.stride(0) if dx is not None else 0, ptr(dw), ptr(db), pitch, G, R, N, K, 0, order, st)

        mp = ptr(self.mask_p)
        smp = self.mask_p.stride(0) if reg else 0
        run("vpc_flow_multi_prep", ptr(xf), sx, ptr(mf), sm, mp, smp, ptr(self.xin), self.xin.stride(0), ptr(self.eps), s10, mem,
            G, int(draw), R, B, d, self.rng_offset, self.rng_offset + (1 << 40), st)
        self.rng_offset += chain_draw_increment(R * FLOW_L, B, d)
        fwd(self.enc_layers, self.enc_acts)
        run("vpc_flow_fwd_multi", ptr(self.t), CTX, self.t.stride(0), ptr(self.eps), ptr(self.z), ptr(self.zlp), s10, G, R, B, st)
        fwd(self.dec_layers, self.dec_acts)
        # the p rows of a member's arrays follow its q rows
        pq = lambda a: (ptr(a), ptr(a[:, B:]) if reg else None)
        run("vpc_flow_loss_multi", ptr(xf), sx, ptr(mf), sm, mp, smp, *pq(self.Y), d, self.Y.stride(0), *pq(self.z),
            *pq(self.zlp), *pq(self.Gy), d, self.Gy.stride(0), *pq(self.gz), *pq(self.gzlp), s10, ptr(self.scratch),
            self.scratch.numel() * 8, ptr(self.out8), ptr(self.loss_f32), ptr(self.accum), mem, G, B, d,
            STAGE_TRAIN if stage == "train" else STAGE_EVAL, 1.0 / B, 1, st)
        # (Gy already holds the gradient of decoder_mean's pre-activation: no gate pass over Y)
        bwd(self.dec_layers, self.dec_acts, self.dec_dacts, self._dec_grads, True)
        run("vpc_flow_bwd_multi", ptr(self.t), CTX, self.t.stride(0), ptr(self.eps), ptr(self.dzd), ptr(self.gz), ptr(self.gzlp),
            s10, ptr(self.dt), CTX, self.dt.stride(0), G, R, B, st)
        bwd(self.enc_layers, self.enc_acts, self.enc_dacts, self._enc_grads, False)
        self.step_count += 1
        run("vpc_adam_step_multi", ptr(self.params), ptr(self.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), pitch, self.n, mem,
            G, self.betas[0], self.betas[1], self.adam_eps, self.step_count, st)
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
