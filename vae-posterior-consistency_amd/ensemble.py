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
    _MemberSet                   what the three classes hold of their members: stacks, device member table, fresh images, inputs
    EnsembleTrainer              the step, the read-outs and per-member views of the stacked state
    MaskEnsembleTrainer          the same for G Reg_VAE_mask / vanilla_VAE_mask members (vpc_step_small_multi_aug_f32)
    EDDIEnsembleTrainer          ... and for G Reg_EDDI / vanilla_EDDI members (vpc_step_small_multi_eddi_f32 +
                                 vpc_reduce_step_adam_eddi_multi); Family says what the three differ in

The sweep's evaluation (eval_vae, evaluate.py:136-297) and its active variable selection (active_learning_func,
evaluate.py:300-511) share their launches the same way: EnsembleEvaluator over build_eval_tables, EnsembleAcquirer over
acquire_plan / acquire_draw_offsets (the shapes and Philox offsets of a run, on the host alone).

    MaskEnsembleEvaluator        EnsembleEvaluator for G Reg_VAE_mask / vanilla_VAE_mask members (vpc_eval_small_multi_aug_f32)
    EDDIEnsembleEvaluator        ... and for G Reg_EDDI / vanilla_EDDI members (vpc_eval_small_multi_eddi_f32: the front-end is read
                                 from the parameter stack); both share vpc_eval_reduce_multi, and X.for_trainer(trainer) reads the
                                 image stack a family trainer's tail re-packs.
    MaskEnsembleAcquirer         EnsembleAcquirer for the same two families: the family evaluator's members and images, the loop of
    EDDIEnsembleAcquirer         EnsembleAcquirer around vpc_impute_small_multi_aug_f32 / _eddi_f32 and vpc_reward_matrix_multi_ex
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from .fused import LP
from .images import PackedImage, flat_written
from .eddi import Reg_EDDI, vanilla_EDDI
from .models import Reg_VAE, Reg_VAE_mask, loss_coefficients, vanilla_VAE, vanilla_VAE_mask
from .ops import as_mask_u8, stride_vector
from .trainer import draw_counters, eval_draw_counters, pad_cols, padded_width

# VpcMember of include/vpc.h (64 bytes): the first 32 are its VpcLossCoef, spelled flat
MEMBER_DTYPE = np.dtype([("cA", "<f4", 2), ("cE", "<f4", 2), ("bq", "<f4"), ("bp", "<f4"), ("cr", "<f4"), ("wml", "<f4"),
                         ("keep_prob", "<f4"), ("lr", "<f4"), ("seed", "<u8"), ("use_maskB", "<i4"), ("reserved", "<i4", 3)])
assert MEMBER_DTYPE.itemsize == 64
MAX_BLOCKS = 8192  # VPC_MULTI_MAX_BLOCKS of include/vpc.h: workgroups (G x tiles per member) of one ensemble launch
EVAL_MAX_BLOCKS = 65536  # VPC_EVAL_MAX_BLOCKS: workgroups of one evaluation launch (the entry walks the tile table in chunks)
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


def steps_in_ensemble(model, vae_type, loader, obs_dim):
    """Does train_sweep step `model` in an ensemble?  Stackable, no 'with_drop' run, a first batch within the small-batch step."""
    first = next(iter(loader), None) if stackable(model) and "with_drop" not in vae_type else None
    return first is not None and first[0].reshape(-1, obs_dim).shape[0] <= ops.step_small_max_rows()


def _shared_or_per_member(t, name, G, tail, note=""):
    """Check that `t` (a tensor, or a shape alone) is [*tail], one array shared by all members, or [G, *tail]; tail[0] = None
    admits any number of rows.  -> the member stride in elements of a DENSE array of that shape, 0 when shared: the shape alone
    decides (an expanded view still has its member axis), and a caller takes the stride of the array it hands to a kernel."""
    shape = tuple(getattr(t, "shape", t))
    k = len(shape) - len(tail)
    if (k == 0 or k == 1 and shape[0] == G) and shape[k + 1:] == tail[1:] and tail[0] in (None, shape[k]):
        return math.prod(shape[1:]) if k else 0
    want = ", ".join("rows" if a is None else str(a) for a in tail)
    raise L.VpcError(f"{name}: expected [{want}] or [{G}, {want}]{note}, got {shape}")


def forward_launches(T, G, max_blocks=0):
    """Launches of one forward call over T tiles x G members at max_blocks workgroups per launch (0: the library's limit)."""
    per = max(1, (max_blocks or EVAL_MAX_BLOCKS) // G)
    return (T + per - 1) // per


def _require_stackable(m):
    if not stackable(m):
        if getattr(m, "mask_augm", False) or getattr(m, "_wide", False):
            raise L.VpcError("ensemble members are plain (not mask-augmented) models with obs_dim <= 128 and latent_dim <= 15")
        raise TypeError(f"EnsembleTrainer supports Reg_VAE and vanilla_VAE members, got {type(m).__name__}")


class Family(NamedTuple):
    """What the member families of the ensemble step differ in on the host: who may be a member, what the members of one
    ensemble share, the layout of their weight images and the row pitch of x / mask / mask_p in the kernels."""
    require: Callable  # model -> None, or raises (TypeError: not this family's class; VpcError: a shape past its kernels)
    shared: Callable  # model -> the tuple the members of one ensemble agree in
    shared_names: str
    layout: Callable  # model -> _lib.Layout of the images the step reads and the tail re-packs
    pitch: Callable  # obs_dim -> row pitch


def _require_mask(m):
    if type(m) not in (Reg_VAE_mask, vanilla_VAE_mask):
        raise TypeError(f"MaskEnsembleTrainer supports Reg_VAE_mask and vanilla_VAE_mask members, got {type(m).__name__}")
    if m._wide:
        raise L.VpcError("mask-augmented ensemble members have 2 * obs_dim <= 128 and latent_dim <= 15")


def _require_eddi(m):
    if type(m) not in (Reg_EDDI, vanilla_EDDI):
        raise TypeError(f"EDDIEnsembleTrainer supports Reg_EDDI and vanilla_EDDI members, got {type(m).__name__}")
    if ops.small_eddi_tiles(m.obs_dim, m.emb_dim) is None:
        raise L.VpcError("point-net ensemble members have obs_dim <= 64 and emb_dim <= 32 (the small-batch step's instantiations)")


_dense_shared = lambda m: (m.obs_dim, m.latent_dim, getattr(m, "reg_type", None))
PLAIN = Family(_require_stackable, _dense_shared, "(obs_dim, latent_dim, reg_type)", lambda m: m._lay(), padded_width)
MASK = Family(_require_mask, _dense_shared, "(obs_dim, latent_dim, reg_type)", lambda m: m._lay(), ops.small_aug_pitch)
EDDI = Family(_require_eddi, lambda m: (m.obs_dim, m.emb_dim, m.latent_dim, getattr(m, "reg_type", None)),
              "(obs_dim, emb_dim, latent_dim, reg_type)",
              lambda m: L.pointnet_layout(m.obs_dim, m.emb_dim, m.latent_dim), ops.small_aug_pitch)


def validate_members(models, world_size=1, family=PLAIN):
    """What one ensemble can hold: stackable members of ONE class, shape and reg_type, on one process (`family`: the same
    rule for the mask-augmented and the point-net members).  Raises before anything touches the device."""
    if world_size > 1:
        raise L.VpcError("EnsembleTrainer is single-process: data parallelism is not part of the ensemble step")
    if len(models) == 0:
        raise L.VpcError("an ensemble needs at least one member")
    for m in models:
        family.require(m)
    m0 = models[0]
    for m in models[1:]:
        if type(m) is not type(m0):
            raise TypeError(f"members of one ensemble share a class: {type(m0).__name__} and {type(m).__name__}")
        a, b = family.shared(m), family.shared(m0)
        if a != b:
            raise L.VpcError(f"members of one ensemble share {family.shared_names}: {b} and {a}")


def stack_models(models, require=_require_stackable):
    """Put the trainable tensors of `models` (same parameter count, already on their device) into ONE [G, n] fp32 buffer:
    model g's tensors become views of row g in table order, so that model.flatten_parameters() returns row g through its
    fast path.  state_dict / in-place load_state_dict / the API path keep working; `.to(device)` afterwards un-stacks a
    model (stack again).  Idempotent for the same list.  Returns the [G, n] buffer (rows 256-byte aligned).
    require: the membership rule of the caller's family (Family.require)."""
    models = list(models)
    if len(models) == 0:
        raise L.VpcError("an ensemble needs at least one member")
    for m in models:
        require(m)
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


def install_image_stack(models, lay, dev):
    """The members' fp32 weight images [enc | dec] as rows of ONE new stack: row g becomes model g's own image (images.py), so
    the API path, the ensemble step's re-pack and the ensemble evaluation read and stamp the same buffer.  Returns the stack."""
    if (lay.enc_img + lay.dec_img) % 4:
        raise L.VpcError("weight image rows must be 16-byte multiples")
    img = torch.from_numpy(lay.img_template).to(dev).repeat(len(models), 1)
    pidx = lay.device_tables(dev)[0]
    for g, m in enumerate(models):
        m._img = PackedImage(img[g], lambda flat, buf: ops.pack_weights(flat, pidx, buf))
    return img


def image_stack_of(models, n_img, dev):
    """(member 0's image, row stride in floats) when the members' images are rows of one stack on `dev`, else None."""
    bufs = [getattr(m._img, "buf", None) for m in models]
    if any(b is None or b.device != dev or b.numel() != n_img or b.dtype != torch.float32 for b in bufs):
        return None
    p0 = bufs[0].data_ptr()
    step = bufs[1].data_ptr() - p0 if len(bufs) > 1 else 4 * n_img
    if step < 4 * n_img or step % 16 or any(b.data_ptr() != p0 + g * step for g, b in enumerate(bufs)):
        return None
    return bufs[0], step // 4


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


class _MemberSet:
    """What EnsembleTrainer, EnsembleEvaluator and EnsembleAcquirer hold of their members, stated once: validation (raised
    before anything touches the device), member table, parameter and image stack, image freshness, inputs at the row pitch."""

    def __init__(self, models, lr, seeds, world_size, family=PLAIN):
        models = list(models)
        validate_members(models, world_size, family)
        self.table = MemberTable(models, lr, seeds)
        self.models = models
        self.rng_offset = 0
        # ---- device state from here on
        self.params = stack_models(models, family.require)
        L.require_cuda(self.params)
        self.G, self.dev = len(models), self.params.device
        self.lay = lay = family.layout(models[0])
        self.n_img, self.dk = lay.enc_img + lay.dec_img, family.pitch(lay.d)  # (dk: row pitch of x / mask in the kernels)
        self._plists = [m.trainable() for m in models]
        self._pads = {}  # pad_cols buffers of this object: slot 0 = x, slot 1 = mask

    def _image_stack_and_table(self, new_image_stack):
        """The members' images as rows of ONE stack (a trainer installs a new one, an evaluator only when they sit in none) and
        the device member table; the trainer allocates them after its own state."""
        adopt = not new_image_stack and image_stack_of(self.models, self.n_img, self.dev) is not None
        self.img = None if adopt else install_image_stack(self.models, self.lay, self.dev)
        self.table_dev = torch.zeros(self.G * MEMBER_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self._table_version = -1

    def _sync_table(self):  # THE upload of the member table: whenever the host rows changed since the last one
        if self._table_version != self.table.version:
            self.table_dev.copy_(torch.from_numpy(self.table.rows.view(np.uint8).reshape(-1)))
            self._table_version = self.table.version

    def _member_image(self, g):
        """The PackedImage of member g that the launches read: the model's own (a row of the image stack)."""
        return self.models[g]._img

    def _repack(self, g, key):
        self.models[g]._images(key)

    def _fresh_images(self, row_ptr=None):
        """Re-pack every image whose parameter key is stale (images.py) -> the keys.  row_ptr: the trainer's rows of the stack."""
        keys = []
        for g, m in enumerate(self.models):
            key = m._param_key(self._plists[g])
            if row_ptr is not None and key[1] != row_ptr[g]:
                raise L.VpcError(f"member {g} no longer sits in the ensemble's parameter stack (moved or re-flattened)")
            if self._member_image(g).key != key:
                self._repack(g, key)
            keys.append(key)
        return keys

    def _check_inputs(self, x, mask):
        """x, mask: each [rows, d] (shared by all members) or [G, rows, d] -> (rows, whether x has the member axis, whether mask)."""
        per_x = _shared_or_per_member(x, "x", self.G, (None, self.lay.d))
        rows = x.shape[-2]
        return rows, per_x, _shared_or_per_member(mask, "mask", self.G, (rows, self.lay.d), " (x and mask agree in their rows)")

    def _padded_inputs(self, x, mask, per_x, per_mask):
        """-> (x fp32, mask 0 / 1 bytes, both dense in rows of dk columns, and the member strides of these two arrays)."""
        x, mask = ops._f32c(x), as_mask_u8(mask)
        if self.dk != self.lay.d:
            x, mask = pad_cols(self._pads, x, self.dk, 0, self.dev), pad_cols(self._pads, mask, self.dk, 1, self.dev)
        return x, mask, x.stride(0) if per_x else 0, mask.stride(0) if per_mask else 0


class EnsembleTrainer(_MemberSet):
    family = PLAIN  # (MaskEnsembleTrainer and EDDIEnsembleTrainer below: the same frame around their families' launches)

    def __init__(self, models, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seeds=None, world_size=1):
        """models: G plain Reg_VAE or G plain vanilla_VAE of one (obs_dim, latent_dim, reg_type), on the GPU.  lr and seeds:
        scalars or one value per member (seeds=None: member g draws with seed g).  The step count (Adam's bias corrections)
        and the Philox offsets are shared: every member steps in every call."""
        super().__init__(models, lr, seeds, world_size, self.family)
        self.betas, self.adam_eps = betas, eps
        self.step_count = 0
        G, n = self.params.shape
        self.vanilla = isinstance(self.models[0], vanilla_VAE)
        zeros = lambda w: torch.zeros(G, _pitch(w), device=self.dev)[:, :w]
        self.grad, self.exp_avg, self.exp_avg_sq = zeros(n), zeros(n), zeros(n)
        self.row_pitch = self.params.stride(0)
        self.out9 = torch.zeros(G, 9, device=self.dev)
        self.accum = torch.zeros(G, device=self.dev)
        self.pidx, self.gidx = self.lay.device_tables(self.dev)
        self.inv = self.lay.inverse_maps(self.dev)
        self._image_stack_and_table(new_image_stack=True)
        self._row_ptr = [self.params[g].data_ptr() for g in range(G)]
        for g, pl in enumerate(self._plists):
            off = 0
            for p in pl:  # .grad are views of the stacked gradient, as under a stand-alone trainer
                p.grad = self.grad[g, off:off + p.numel()].view_as(p)
                off += p.numel()
        self.trainers = [MemberView(self, g) for g in range(G)]
        # workgroup order of the step launch (include/vpc.h): 1 = all tiles of a member on one XCD, 0 = member-major.  Same bits;
        # 1 is 3-5 % faster where the GPU is the limit and never slower from 8 members on; below 8 members its grid has
        # surplus workgroups that cost 0.3-0.8 us (profiles/ensemble_notes.md)
        self.order = 1 if G >= 8 else 0
        self._ws = None

    # ------------------------------------------------------------------
    def _workspaces(self, B, dk):
        if self._ws == (B, dk):
            return
        G, lay, dev, tiles = self.G, self.lay, self.dev, (B + 15) // 16
        self.eps_buf = torch.empty(G, 3, B, LP, device=dev)
        self.mask_p_buf = torch.zeros(G, B, dk, dtype=torch.uint8, device=dev)
        if getattr(self, "_tiles_cap", 0) < tiles:
            self.partE = torch.empty(G, tiles * lay.enc_part, device=dev)
            self.partD = torch.empty(G, tiles * lay.dec_part, device=dev)
            self.loss_part = torch.empty(G, tiles * 8, dtype=torch.float64, device=dev)
            self._tiles_cap = tiles
        own = {  # the strides of what the trainer owns; a step fills in those of its x and mask
            ops.MS_MASK_P: self.mask_p_buf.stride(0), ops.MS_EPS: self.eps_buf.stride(0), ops.MS_IMG: self.img.stride(0),
            ops.MS_PARTE: self.partE.stride(0), ops.MS_PARTD: self.partD.stride(0), ops.MS_LOSS: self.loss_part.stride(0),
            ops.MS_PARAM: self.row_pitch, **self._family_workspaces(tiles)}
        self._strides = stride_vector(max(own) + 1 if max(own) >= ops.MS_COUNT else ops.MS_COUNT, own)
        self._ws = (B, dk)

    def _family_workspaces(self, tiles):
        """Per-tile buffers a family's launches take besides -> {stride slot: member stride}."""
        return {}

    def _check_draws(self, draw):
        """Whether this family can make the step's draws in the launch (raises before anything is launched or counted)."""

    def _launch_step(self, x, mask, two, nplanes, draw, off_m, off_e, strides, B):
        lay = self.lay
        ops.step_small_multi_f32(x, mask, self.mask_p_buf if two else None, self.eps_buf, self.img[0, :lay.enc_img],
                                 self.img[0, lay.enc_img:], self.table_dev, self.G, 2 if two else 1, nplanes, draw, off_m, off_e,
                                 1.0 / B, self.models[0]._x_logvar_value, self.partE, self.partD, self.loss_part, strides, B,
                                 self.dk, lay.L, self.order)

    def _launch_tail(self, tiles, strides, B):
        lay = self.lay
        ops.reduce_step_adam_multi(self.partE, self.partD, self.loss_part, tiles, lay.enc_part, lay.dec_part, strides,
                                   self.inv, self.table_dev, self.G, self.grad, B, lay.d, self.out9, self.accum, self.params,
                                   self.exp_avg, self.exp_avg_sq, self.betas[0], self.betas[1], self.adam_eps,
                                   self.step_count, self.pidx, self.img)

    def step(self, x, mask, mask_p=None, eps_q=None, eps_p=None, eps_ml=None, *, epoch=1, alpha=1.0, beta=1.0,
             beta_annealing=False, p_missingness=30):
        """One training step of every member.  x, mask: [B, d] (one batch shared by all members) or [G, B, d]; alpha, beta,
        p_missingness: scalars or one value per member.  mask_p / eps_* are drawn on the device - member g with its own seed,
        in its own element space, exactly as its stand-alone trainer would - unless ALL the step's draws are injected
        ([G, ...] or shared).  No host sync: losses are in `out9[:, 0]`, the running totals in `accum`."""
        L.require_cuda(x)
        G, lay, d, Ld, dk = self.G, self.lay, self.lay.d, self.lay.L, self.dk
        B, per_x, per_mask = self._check_inputs(x, mask)
        tiles = (B + 15) // 16
        if B > ops.step_small_max_rows():
            raise L.VpcError(f"batch {B}: the ensemble step covers batches up to {ops.step_small_max_rows()} rows "
                             "(larger ones fill the chip on their own: FusedTrainer)")
        if G * tiles > MAX_BLOCKS:
            raise L.VpcError(f"{G} members x {tiles} tiles = {G * tiles} workgroups: one ensemble launch holds {MAX_BLOCKS}")
        two = not self.vanilla
        self.table.update(epoch, alpha, beta, beta_annealing, p_missingness)
        need_ml = self.table.need_ml
        given = [mask_p is not None] * two + [eps_q is not None] + [eps_p is not None] * two + [eps_ml is not None] * need_ml
        if any(given) != all(given):
            raise L.VpcError("inject all of the step's draws (mask_p, eps_q, eps_p, eps_ml as the model uses them) or none")
        draw = not any(given)
        self._check_draws(draw)
        x, mask, sx, smask = self._padded_inputs(x, mask, per_x, per_mask)
        self._workspaces(B, dk)
        self._sync_table()
        keys = self._fresh_images(self._row_ptr)
        nplanes = 3 if need_ml else 2 if two else 1
        off_m = off_e = 0
        if draw:  # every member is an unsharded batch of B rows
            off_m, off_e, self.rng_offset, _, _ = draw_counters(self.rng_offset, two, nplanes, B, B, 0, LP, dk)
        else:
            if two:
                self.mask_p_buf[:, :, :d].copy_(as_mask_u8(mask_p))
            for k, e in enumerate((eps_q, eps_p, eps_ml)[:nplanes]):
                self.eps_buf[:, k, :, :Ld].copy_(e)
        strides = self._strides
        strides[ops.MS_X], strides[ops.MS_MASK] = sx, smask
        self._launch_step(x, mask, two, nplanes, draw, off_m, off_e, strides, B)
        self.step_count += 1
        self._launch_tail(tiles, strides, B)
        for g, m in enumerate(self.models):
            flat_written(m, self._plists[g], keys[g], (self._member_image(g),))

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

    def evaluator(self):
        """An EnsembleEvaluator on this trainer's members, with their seeds: it reads the image stack the step re-packs."""
        return EnsembleEvaluator(self.models, seeds=self.table.rows["seed"].tolist())


class _FamilyTrainer(EnsembleTrainer):
    def evaluator(self):
        raise L.VpcError("EnsembleEvaluator and EnsembleAcquirer cover the plain Reg_VAE / vanilla_VAE members only: evaluate "
                         "mask-augmented and point-net members with MaskEnsembleEvaluator.for_trainer(trainer) / "
                         "EDDIEnsembleEvaluator.for_trainer(trainer), and run their acquisition with "
                         "MaskEnsembleAcquirer.for_trainer(trainer) / EDDIEnsembleAcquirer.for_trainer(trainer)")


class _PointNetImages:
    """The images a point-net member set hands to its launches: those of L.pointnet_layout (trunk and decoder of a row
    [trunk | decoder | front-end]), kept by the set as PackedImage rows of ONE stack under the parameter-key freshness rule of
    images.py.  The models' own images (model._lay()'s) stay theirs.  images_from: another set of the same members whose stack and
    PackedImage rows this one shares (an evaluator on a trainer's members reads what the trainer's tail re-packs and stamps)."""
    _images_from = None

    def _image_stack_and_table(self, new_image_stack):
        lay, n, src = self.lay, self.lay.n_params, self._images_from
        if src is not None:
            self.img, self._images_pn = src.img, src._images_pn
        else:
            self.img = torch.from_numpy(lay.img_template).to(self.dev).repeat(self.G, 1)
            pidx = lay.device_tables(self.dev)[0]
            self._images_pn = [PackedImage(self.img[g], lambda flat, buf: ops.pack_weights(flat[:n], pidx, buf))
                               for g in range(self.G)]
        self.table_dev = torch.zeros(self.G * MEMBER_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self._table_version = -1

    def _member_image(self, g):
        return self._images_pn[g]

    def _repack(self, g, key):
        self._images_pn[g].get(key, self.models[g]._flat)


class MaskEnsembleTrainer(_FamilyTrainer):
    """EnsembleTrainer for G Reg_VAE_mask or G vanilla_VAE_mask of one (obs_dim, latent_dim, reg_type): step(), loss_values(),
    epoch_total() and trainers[g] as there.  Rows of x, mask and mask_p go at ops.small_aug_pitch(obs_dim) columns (mask 0 in
    the padding) and the device draws are made in the launch at that pitch - the counters of FusedTrainer's small-batch path,
    so member g computes bit for bit what its stand-alone FusedTrainer computes there."""
    family = MASK

    def _launch_step(self, x, mask, two, nplanes, draw, off_m, off_e, strides, B):
        lay = self.lay
        ops.step_small_multi_aug_f32(x, mask, self.mask_p_buf if two else None, self.eps_buf, self.img[0, :lay.enc_img],
                                     self.img[0, lay.enc_img:], self.table_dev, self.G, 2 if two else 1, nplanes, draw, off_m,
                                     off_e, 1.0 / B, self.models[0]._x_logvar_value, self.partE, self.partD, self.loss_part,
                                     strides, B, self.dk, lay.d, lay.L, self.order)


class EDDIEnsembleTrainer(_PointNetImages, _FamilyTrainer):
    """EnsembleTrainer for G Reg_EDDI or G vanilla_EDDI of one (obs_dim, emb_dim, latent_dim, reg_type).  A row of the
    parameter stack is [trunk | decoder | front-end] as under EDDITrainer; the image stack holds the point-net layout's
    images of trunk and decoder (the one EDDITrainer's small-batch step packs, not model._lay()'s: the models' own images
    stay theirs).  Draws follow EDDITrainer's small-batch rule: counters at the pitch obs_dim, so the launch can make them
    only where obs_dim % 4 == 0 (the kernel's rows have 4 * ceil(obs_dim / 4) columns); for other widths step() takes the
    step's draws injected - all of them, at every obs_dim <= 64 - and refuses to draw: the stand-alone stream is pinned to the
    unpadded pitch, and one draw launch per member would undo the point of the ensemble."""
    family = EDDI

    def _family_workspaces(self, tiles):
        K, n_front = self.lay.K, self.lay.n_front
        if getattr(self, "_front_cap", 0) < tiles:
            self.partF = torch.empty(self.G, tiles * 2 * K * self.dk, device=self.dev)
            self.snap = torch.empty(self.G, _pitch(n_front), device=self.dev)
            self._front_cap = tiles
        return {ops.MS_PARTF: self.partF.stride(0), ops.MS_SNAP: self.snap.stride(0)}

    def _check_draws(self, draw):
        if draw and self.dk != self.lay.d:
            raise L.VpcError(f"obs_dim {self.lay.d} is not a multiple of 4: the ensemble step cannot make a point-net member's "
                             "draws in its launch (the stand-alone stream is drawn at the unpadded pitch, the kernel's rows "
                             f"have {self.dk} columns); inject mask_p and the eps planes")

    def _launch_step(self, x, mask, two, nplanes, draw, off_m, off_e, strides, B):
        lay = self.lay
        ops.step_small_multi_eddi_f32(x, mask, self.mask_p_buf if two else None, self.eps_buf, self.img[0, :lay.enc_img],
                                      self.img[0, lay.enc_img:], self.table_dev, self.G, 2 if two else 1, nplanes, draw, off_m,
                                      off_e, 1.0 / B, self.models[0]._x_logvar_value, self.partE, self.partD, self.loss_part,
                                      strides, B, self.dk, lay.d, lay.L, lay.K, self.params[0, lay.n_params:], self.partF,
                                      self.snap, self.order)

    def _launch_tail(self, tiles, strides, B):
        lay = self.lay
        ops.reduce_step_adam_eddi_multi(self.partE, self.partD, self.loss_part, tiles, lay.enc_part, lay.dec_part, strides,
                                        self.inv, self.table_dev, self.G, self.grad, lay.n_params, B, lay.d, self.out9,
                                        self.accum, self.params, self.exp_avg, self.exp_avg_sq, self.betas[0], self.betas[1],
                                        self.adam_eps, self.step_count, self.pidx, self.img, self.partF, self.snap, lay.K, self.dk)


def sweep_family(model, vae_type, loader, obs_dim):
    """"mask" / "eddi": train_sweep may step the mask-augmented / point-net `model` with others of its kind
    (MaskEnsembleTrainer / EDDIEnsembleTrainer); None: it may not.  No 'with_drop' run, a shape the family's step kernels are
    instantiated for, a first batch within the small-batch step and, for the point-net classes, obs_dim % 4 == 0
    (EDDIEnsembleTrainer draws in its launch only there)."""
    for name, family in (("mask", MASK), ("eddi", EDDI)):
        try:
            family.require(model)
        except (TypeError, L.VpcError):
            continue
        if "with_drop" in vae_type or (family is EDDI and model.obs_dim % 4):
            return None
        first = next(iter(loader), None)
        return name if first is not None and first[0].reshape(-1, obs_dim).shape[0] <= ops.step_small_max_rows() else None
    return None


# ------------------------------------------------------------------------------------------------ evaluation
class EvalTables(NamedTuple):
    """Host form of the tables of include/vpc.h (ensemble evaluation), int64."""
    tiles: np.ndarray  # [T, 4]: data row of the first row, valid rows 1..16, draw row of the first row, batch index
    batches: np.ndarray  # [NB, 4]: rows, MC pass, first tile, tiles
    passes: np.ndarray  # [M, 2]: first batch, batches
    R: int  # draw rows: every row of every batch of every pass


def eval_layout_key(N, batch_size=None, M=1, batches=None):
    """What the tables depend on, hashable: (N, batch layout, M)."""
    if (batch_size is None) == (batches is None):
        raise L.VpcError("give either batch_size or batches (one list of (row_lo, row_hi) ranges per MC pass)")
    if batches is None:
        return int(N), ("batch_size", int(batch_size)), int(M)
    return int(N), tuple(tuple((int(lo), int(hi)) for lo, hi in p) for p in batches), int(M)


def build_eval_tables(N, batch_size=None, M=1, batches=None):
    """The tile, batch and pass tables of one evaluation over N data rows.  batch_size: every pass walks the rows in
    consecutive ranges of batch_size (the last one short); batches: M lists of (row_lo, row_hi) ranges, one list per pass.
    A batch is cut into tiles of 16 rows (the last one ragged), so no tile straddles two batches.  Draw rows count on from pass
    to pass, batch to batch, row to row: under batch_size, row n of pass p draws as row p * N + n."""
    N, layout, M = eval_layout_key(N, batch_size, M, batches)
    if N < 1 or M < 1:
        raise L.VpcError("evaluation needs at least one data row and one MC pass")
    if batches is None:
        if batch_size < 1:
            raise L.VpcError(f"batch_size {batch_size}")
        batches = [[(lo, min(lo + batch_size, N)) for lo in range(0, N, batch_size)]] * M
    else:
        batches = layout
        if len(batches) != M:
            raise L.VpcError(f"{len(batches)} batch lists for {M} MC passes")
    tiles, brows, prows, r = [], [], [], 0
    for p, ranges in enumerate(batches):
        if len(ranges) == 0:
            raise L.VpcError(f"MC pass {p} has no batch")
        prows.append((len(brows), len(ranges)))
        for lo, hi in ranges:
            if not 0 <= lo < hi <= N:
                raise L.VpcError(f"batch rows [{lo}, {hi}) outside the {N} data rows (or empty)")
            t0 = len(tiles)
            for s in range(lo, hi, 16):
                tiles.append((s, min(16, hi - s), r + s - lo, len(brows)))
            r += hi - lo
            brows.append((hi - lo, p, t0, len(tiles) - t0))
    return EvalTables(np.array(tiles, np.int64), np.array(brows, np.int64), np.array(prows, np.int64), r)


class EnsembleEvaluator(_MemberSet):
    """eval_vae's numbers (evaluate.py:136-297) for G stackable members over all batches and MC passes in one pair of launches:
    vpc_eval_small_multi_f32 (forward of every member x pass x batch x 16-row tile -> five sums per tile) and
    vpc_eval_reduce_multi (tiles -> batches -> passes -> [G, 4]).  Only the q pass is computed: VAE.py:410-420 reads nothing else."""
    TABLE_CACHE = 8  # distinct (N, batch layout, M) kept on the device
    family = PLAIN  # (MaskEnsembleEvaluator and EDDIEnsembleEvaluator below: the same frame around their families' forward launch)

    def __init__(self, models, seeds=None, world_size=1):
        """models: as EnsembleTrainer (validate_members), on the GPU.  seeds: one Philox seed per member (None: member g draws
        with seed g).  The evaluator owns a Philox offset: a call advances it by the groups it consumed (eval_draw_counters)."""
        super().__init__(models, 0.0, seeds, world_size, self.family)
        self._image_stack_and_table(new_image_stack=False)
        self._tables, self._part = {}, None
        self.launches = 0  # kernel launches of the last call (the forward entry walks the tile table in chunks)

    def tables(self, N, batch_size=None, M=1, batches=None):
        """(EvalTables, device tiles, device batches, device passes) of a layout: built and uploaded once, then cached."""
        key = eval_layout_key(N, batch_size, M, batches)
        hit = self._tables.get(key)
        if hit is None:
            tb = build_eval_tables(N, batch_size, M, batches)
            if len(self._tables) >= self.TABLE_CACHE:
                self._tables.pop(next(iter(self._tables)))
            hit = self._tables[key] = (tb,) + tuple(torch.from_numpy(a).to(self.dev) for a in (tb.tiles, tb.batches, tb.passes))
        return hit

    def _images(self):
        """(member 0's image, row stride) of the stack the members' images sit in NOW, every image fresh (_fresh_images)."""
        if image_stack_of(self.models, self.n_img, self.dev) is None:  # (a model's image was replaced: .to(), a stand-alone trainer)
            self.img = install_image_stack(self.models, self.lay, self.dev)
        self._fresh_images()
        return image_stack_of(self.models, self.n_img, self.dev)

    def _family_strides(self):
        """Member strides a family's forward launch reads besides -> {stride slot: member stride}."""
        return {}

    def _launch_forward(self, x, mask, eps_plane, img0, tiles_dev, T, N, R, draw, offset, strides, max_blocks):
        """THE forward launch of evaluate(): what a family's evaluator overrides."""
        lay = self.lay
        ops.eval_small_multi_f32(x, mask, eps_plane, img0[:lay.enc_img], img0[lay.enc_img:], self.table_dev, self.G, tiles_dev, T,
                                 N, R, draw, offset, self.models[0]._x_logvar_value, self._part, strides, self.dk, lay.d, lay.L,
                                 max_blocks)

    def evaluate(self, x, mask, batch_size=None, M=1, *, batches=None, epoch, beta=1.0, beta_annealing=False, eps=None,
                 max_blocks=0):
        """x, mask: [N, d] (one data set shared by all members) or [G, N, d].  Batches: consecutive ranges of batch_size rows in
        every one of the M passes, or `batches` = M lists of (row_lo, row_hi).  beta: scalar or one per member; epoch and
        beta_annealing as model.loss takes them.  eps: [R, L] or [G, R, L] normals, R = the rows of all batches of all passes in
        order (M * N under batch_size), or None: drawn on the device from member g's Philox stream (eval_draw_counters).
        Returns [G, 4] on the device = (rmse on ~mask, elbo, negll, negll_imp) as eval_vae averages them; no host sync.
        max_blocks: workgroups per launch (0: the library's limit)."""
        L.require_cuda(x)
        G, lay, d, Ld, dk = self.G, self.lay, self.lay.d, self.lay.L, self.dk
        N, per_x, per_mask = self._check_inputs(x, mask)
        x, mask, sx, smask = self._padded_inputs(x, mask, per_x, per_mask)
        tb, tiles_dev, batches_dev, passes_dev = self.tables(N, batch_size, M, batches)
        T, R = tb.tiles.shape[0], tb.R
        if eps is not None:
            _shared_or_per_member(eps, "eps", G, (R, Ld))
        # the evaluate stage is the q pass's ELBO (VAE.py:410-420): at alpha = 0 every loss record's bq is its KL weight
        self.table.update(epoch, 0.0, beta, beta_annealing, 0)
        self._sync_table()
        img0, simg = self._images()
        [(offset, eps_plane)], seps = self._draws(None if eps is None else eps.unsqueeze(-3), R)
        if self._part is None or self._part.shape[1] < T * 5:
            self._part = torch.empty(G, T * 5, dtype=torch.float64, device=self.dev)
        out = torch.empty(G, 4, device=self.dev)
        strides = stride_vector(ops.MS_COUNT, {ops.MS_X: sx, ops.MS_MASK: smask, ops.MS_EPS: seps, ops.MS_IMG: simg,
                                               ops.MS_PART: self._part.stride(0), **self._family_strides()})
        self._launch_forward(x, mask, eps_plane, img0, tiles_dev, T, N, R, eps is None, offset, strides, max_blocks)
        ops.eval_reduce_multi(self._part, batches_dev, tb.batches.shape[0], passes_dev, M, self.table_dev, G,
                              self._part.stride(0), T, d, out)
        self.launches = forward_launches(T, G, max_blocks) + 1
        return out

    def _draws(self, eps, R, calls=1):
        """-> ([(Philox offset, member 0's eps plane) of `calls` forward calls in issue order], the planes' member stride).
        eps None: drawn on the device at successive eval_draw_counters offsets; else [calls, R, L] (shared by the members) or
        [G, calls, R, L], checked by the caller, which uses no counter."""
        if eps is None:
            offs, self.rng_offset = forward_draw_offsets(self.rng_offset, R, calls)
            return [(off, None) for off in offs], 0
        buf = torch.zeros(*eps.shape[:-1], LP, device=self.dev)  # THE padding of injected normals: rows of LP floats
        Ld = self.lay.L
        buf[..., :Ld].copy_(eps)
        if eps.dim() == 3:
            return [(0, buf[c]) for c in range(calls)], 0
        return [(0, buf[0, c]) for c in range(calls)], buf.stride(0)  # (the stride of the copy: eps may be an expanded view)


class _FamilyEvaluator(EnsembleEvaluator):
    """EnsembleEvaluator for a member family of the ensemble step other than the plain one: evaluate(), tables(), `launches` and
    the Philox offset as there; a subclass says which forward launch runs and what its images are."""

    def __init__(self, models, seeds=None, world_size=1, *, images_from=None):
        """models, seeds: as EnsembleEvaluator, members of this class's family.  images_from: a family trainer on the same
        members (for_trainer) whose image rows are read; the mask-augmented evaluator needs no more than that the trainer exists:
        its members' own images ARE the trainer's rows, and it adopts them as the plain evaluator does."""
        self._images_from = images_from
        super().__init__(models, seeds, world_size)

    @classmethod
    def for_trainer(cls, trainer):
        """An evaluator on a family trainer's members, with their seeds, that reads the image stack the trainer's tail re-packs:
        an evaluation between steps sees the current weights without a re-pack."""
        if getattr(trainer, "family", None) is not cls.family:
            raise TypeError(f"{cls.__name__}.for_trainer takes the trainer of its own family, got {type(trainer).__name__}")
        return cls(trainer.models, seeds=trainer.table.rows["seed"].tolist(), images_from=trainer)


class MaskEnsembleEvaluator(_FamilyEvaluator):
    """EnsembleEvaluator for G Reg_VAE_mask or G vanilla_VAE_mask of one (obs_dim, latent_dim, reg_type): the evaluate stage of
    VAE.py:570-580 / :1053-1060 through vpc_eval_small_multi_aug_f32 + vpc_eval_reduce_multi.  The images are the models' own
    (mask-augmented layout), adopted or installed as a stack exactly as the plain evaluator does - MaskEnsembleTrainer re-packs
    these very rows -; rows of x and mask go at ops.small_aug_pitch(obs_dim) columns."""
    family = MASK

    def _launch_forward(self, x, mask, eps_plane, img0, tiles_dev, T, N, R, draw, offset, strides, max_blocks):
        lay = self.lay
        ops.eval_small_multi_aug_f32(x, mask, eps_plane, img0[:lay.enc_img], img0[lay.enc_img:], self.table_dev, self.G,
                                     tiles_dev, T, N, R, draw, offset, self.models[0]._x_logvar_value, self._part, strides,
                                     self.dk, lay.d, lay.L, max_blocks)


class EDDIEnsembleEvaluator(_PointNetImages, _FamilyEvaluator):
    """EnsembleEvaluator for G Reg_EDDI or G vanilla_EDDI of one (obs_dim, emb_dim, latent_dim, reg_type): the evaluate stage of
    VAE.py:757-767 / :935-950 through vpc_eval_small_multi_eddi_f32 + vpc_eval_reduce_multi.  The images are those of the
    point-net layout, the evaluator's own PackedImage rows (or the trainer's: for_trainer); the front-end is read from the members'
    rows of the parameter stack, so every member has to sit in its row still.  The eps draw does not depend on the pitch of x:
    unlike EDDIEnsembleTrainer.step, evaluate() draws on the device at every obs_dim."""
    family = EDDI

    def __init__(self, models, seeds=None, world_size=1, *, images_from=None):
        super().__init__(models, seeds, world_size, images_from=images_from)
        self._row_ptr = [self.params[g].data_ptr() for g in range(self.G)]

    def _images(self):
        self._fresh_images(self._row_ptr)  # (raises for a member that left its row: the front-end is read from the stack)
        return self.img[0], self.img.stride(0)

    def _family_strides(self):
        return {ops.MS_PARAM: self.params.stride(0)}

    def _launch_forward(self, x, mask, eps_plane, img0, tiles_dev, T, N, R, draw, offset, strides, max_blocks):
        lay = self.lay
        ops.eval_small_multi_eddi_f32(x, mask, eps_plane, img0[:lay.enc_img], img0[lay.enc_img:], self.table_dev, self.G,
                                      tiles_dev, T, N, R, draw, offset, self.models[0]._x_logvar_value, self._part, strides,
                                      self.dk, lay.d, lay.L, lay.K, self.params[0, lay.n_params:], max_blocks)


# ------------------------------------------------------------------------------------------------ acquisition
REWARD_WS_FLOATS = 64 << 20  # default bound of the reward workspaces of one member chunk (256 MB), as active.FLOW_REWARD_WS_FLOATS


def acquire_plan(G, d, Ld, x_shape, M, repeats=1, max_steps=None, eps_shape=None):
    """Shapes of one EnsembleAcquirer.run, checked on the host alone: -> (n, steps, forward calls of the run, draw rows per
    call).  A repeat is 1 + 2 * steps forward calls: the curve's start, then per acquisition step the imputation and the
    curve's next point."""
    _shared_or_per_member(x_shape, "x", G, (None, d))
    n = x_shape[-2]
    if n < 1 or M < 1 or repeats < 1 or d < 2:
        raise L.VpcError(f"run: n = {n}, M = {M}, repeats = {repeats}, obs_dim = {d}: each at least 1 (obs_dim 2)")
    if max_steps is not None and max_steps < 0:
        raise L.VpcError(f"max_steps {max_steps}")
    steps = d - 1 if max_steps is None else min(int(max_steps), d - 1)
    calls, R = repeats * (1 + 2 * steps), M * n
    if eps_shape is not None:
        _shared_or_per_member(eps_shape, "eps", G, (calls, R, Ld),
                              f" ({calls} forward calls = {repeats} repeats x (1 + 2 x {steps} steps))")
    return n, steps, calls, R


def forward_draw_offsets(rng_offset, draw_rows, calls):
    """The Philox offsets of `calls` forward calls in issue order - successive eval_draw_counters(., draw_rows, LP), no rule of
    its own - and the rng_offset after them."""
    offs = []
    for _ in range(calls):
        off, rng_offset = eval_draw_counters(rng_offset, draw_rows, LP)
        offs.append(off)
    return offs, rng_offset


def acquire_draw_offsets(rng_offset, draw_rows, steps, repeats=1):
    """forward_draw_offsets of a run: a repeat is 1 + 2 * steps forward calls (acquire_plan)."""
    return forward_draw_offsets(rng_offset, draw_rows, repeats * (1 + 2 * steps))


def reward_member_chunk(G, n, d, M, budget_floats=REWARD_WS_FLOATS, sizes=None):
    """Members per pass through the reward workspaces so that they stay within `budget_floats` (at least one member)."""
    per = sum(sizes if sizes is not None else ops.reward_scratch_multi(n, d, M))
    return max(1, min(G, int(budget_floats) // per))


class _AcquireCall(NamedTuple):
    """The constants of one EnsembleAcquirer call for its forward and reward launches (EnsembleAcquirer._setup)."""
    n: int
    M: int
    x: torch.Tensor  # fp32 [n, d] or [G, n, d]: the reward reads rows of d columns
    sx: int  # member stride of x (0: shared)
    img0: torch.Tensor  # member 0's weight image [enc | dec]
    simg: int  # row stride of the image stack
    xk: torch.Tensor = None  # x in rows of dk columns (x itself when dk == d)
    sxk: int = 0
    tiles_dev: torch.Tensor = None  # the tile table [T, 4] of (n, one batch of n rows, M passes)
    max_blocks: int = 0


class EnsembleAcquirer(EnsembleEvaluator):
    """The acquisition loop of active_learning_func (evaluate.py:300-511) for G stackable members at once.  Per acquisition step,
    whatever G:  vpc_impute_small_multi_f32 (mode 0: the M imputations `im` of every member) -> vpc_reward_matrix_multi (three
    launches per member chunk: R) -> vpc_acquire_multi (argmax, mask, action) -> vpc_impute_small_multi_f32 (mode 1) +
    vpc_target_mse_multi (the information curve's next point).  Masks, actions, rewards and the curve stay on the device: no host
    sync inside a repeat.  Members, stacking, image freshness and the Philox offset are EnsembleEvaluator's.  Only the q pass is
    computed (mask_p and the p pass reach no output of the loop, VAE.py:496-507)."""

    def _setup(self, x, n, M, forward=True, max_blocks=0):
        """What the launches of one call share; forward: also the device member table, the tile table, x at the row pitch."""
        d = self.lay.d
        self.params = stack_models(self.models, self.family.require)  # (idempotent; a member moved since is stacked again)
        per_x = _shared_or_per_member(x, "x", self.G, (n, d))
        x = ops._f32c(x)
        img0, simg = self._images()
        sx = x.stride(0) if per_x else 0
        if not forward:
            return _AcquireCall(n, M, x, sx, img0, simg)
        tiles_dev = self.tables(n, n, M)[1]
        self.table.update(1, 0.0, 1.0, False, 0)  # (the loop reads the seeds only)
        self._sync_table()
        xk = x if self.dk == d else pad_cols(self._pads, x, self.dk, 0, self.dev)  # (the reward reads rows of d columns)
        return _AcquireCall(n, M, x, sx, img0, simg, xk, xk.stride(0) if per_x else 0, tiles_dev, max_blocks)

    def _forward(self, c, strides, maskk, eps_plane, offset, mode, out, out_stride):
        lay = self.lay
        ops.impute_small_multi_f32(c.xk, maskk, eps_plane, c.img0[:lay.enc_img], c.img0[lay.enc_img:], self.table_dev, self.G,
                                   c.tiles_dev, c.tiles_dev.shape[0], c.n, c.M * c.n, eps_plane is None, offset,
                                   self.models[0]._x_logvar_value, mode, out, out_stride, strides, c.xk.shape[-1], lay.d, lay.L,
                                   c.max_blocks)

    def impute(self, x, mask, M, mode=0, *, eps=None, max_blocks=0):
        """ONE forward call of the loop under a given mask [G, n, d] (or [n, d], shared): mode 0 -> x_hat of the M passes
        [G, M, n, d] (`im`), mode 1 -> the target column's squared error per draw row [G, M n].  eps: [M n, L] or [G, M n, L],
        or None: drawn at the next eval_draw_counters offset."""
        G, lay, d, Ld = self.G, self.lay, self.lay.d, self.lay.L
        n, _, _, R = acquire_plan(G, d, Ld, x.shape, M)
        if eps is not None:
            _shared_or_per_member(eps, "eps", G, (R, Ld))
        _shared_or_per_member(mask, "mask", G, (n, d))
        if mode not in (0, 1):
            raise L.VpcError(f"mode 0 or 1, got {mode}")
        L.require_cuda(x, mask, eps)
        c = self._setup(x, n, M, max_blocks=max_blocks)
        maskk = torch.zeros(G, n, c.xk.shape[-1], dtype=torch.uint8, device=self.dev)
        maskk[:, :, :d].copy_(as_mask_u8(mask))
        [(offset, plane)], seps = self._draws(None if eps is None else eps.unsqueeze(-3), R)
        out = torch.empty((G, M, n, d) if mode == 0 else (G, R), device=self.dev)
        strides = stride_vector(ops.MS_COUNT, {ops.MS_X: c.sxk, ops.MS_MASK: maskk.stride(0), ops.MS_EPS: seps, ops.MS_IMG: c.simg,
                                               **self._family_strides()})
        self._forward(c, strides, maskk, plane, offset, mode, out, out.stride(0))
        self.launches = forward_launches(c.tiles_dev.shape[0], G, max_blocks)
        return out

    def _once_per_call(self):
        """What a family's reward needs once per run() / reward() call, launched here -> the launches it made."""
        return 0

    def _reward_sizes(self, n, M):
        """Floats per member of the reward workspaces pre / stat / w1t."""
        return ops.reward_scratch_multi(n, self.lay.d, M)

    def _reward_workspaces(self, n, M, ws_floats):
        """(floats per member of pre / stat / w1t, members per chunk); the buffers are kept between calls."""
        sizes = self._reward_sizes(n, M)
        chunk = reward_member_chunk(self.G, n, self.lay.d, M, ws_floats, sizes)
        key = (n, M, chunk)
        if getattr(self, "_reward_ws_key", None) != key:
            self._reward_ws = tuple(torch.empty(chunk * s, device=self.dev) for s in sizes)
            self._reward_ws_key = key
        return sizes, chunk

    def _reward_strides(self, c, mask, im, R, sizes):
        return stride_vector(ops.RM_COUNT, {
            ops.RM_X: c.sx, ops.RM_MASK: mask.stride(0), ops.RM_IM: im.stride(0), ops.RM_PARAM: self.params.stride(0),
            ops.RM_IMG: c.simg, ops.RM_PRE: sizes[0], ops.RM_STAT: sizes[1], ops.RM_W1T: sizes[2], ops.RM_R: R.stride(0)})

    def _reward(self, c, strides, mask, im, R, chunk):
        """mask [G, n, d] bytes, im / R: [G, ...] views whose member slices are dense; strides: _reward_strides of such views."""
        lay = self.lay
        w1 = self.params[0]  # seq_encoder.0.weight [100][d] opens a member's row of the parameter stack, its bias follows
        pre, stat, w1t = self._reward_ws
        ops.reward_matrix_multi(c.x, mask, im[0], w1, w1[100 * lay.d:], c.img0[:lay.enc_img], pre, stat, w1t, R[0], self.G, chunk,
                                strides, c.n, lay.d, lay.L, c.M)

    def reward(self, x, mask, im, *, ws_floats=REWARD_WS_FLOATS):
        """R [G, n, d-1] of ONE acquisition step: member g's reward_matrix on x (shared [n, d] or [G, n, d]), its mask [G, n, d]
        and its imputations im [G, M, n, d].  ws_floats bounds the workspaces: members go through them in chunks."""
        G, d = self.G, self.lay.d
        n = acquire_plan(G, d, self.lay.L, x.shape, im.shape[1] if im.dim() == 4 else 0)[0]
        M = im.shape[1]
        if tuple(mask.shape) != (G, n, d) or tuple(im.shape) != (G, M, n, d):
            raise L.VpcError(f"mask: expected [{G}, {n}, {d}], got {tuple(mask.shape)}; im: expected [{G}, M, {n}, {d}], got "
                             f"{tuple(im.shape)}")
        L.require_cuda(x, mask, im)
        c = self._setup(x, n, M, forward=False)
        sizes, chunk = self._reward_workspaces(n, M, ws_floats)
        R = torch.empty(G, n, d - 1, device=self.dev)
        mask, im = as_mask_u8(mask), ops._f32c(im)
        once = self._once_per_call()
        self._reward(c, self._reward_strides(c, mask, im, R, sizes), mask, im, R, chunk)
        self.launches = once + 3 * ((G + chunk - 1) // chunk)
        return R

    def run(self, x, M, *, repeats=1, max_steps=None, eps=None, keep_im=True, max_blocks=0, ws_floats=REWARD_WS_FLOATS):
        """x: [n, d] (shared) or [G, n, d]; the target is the last column and is never revealed.  Every member starts every
        repeat with nothing observed and reveals, per row, the best candidate of each step.  eps: [calls, M n, L] or
        [G, calls, M n, L] normals for ALL forward calls of the run in issue order (acquire_plan), draw row m n + i = row i of
        pass m; None: member g draws from its Philox stream, every call at the next eval_draw_counters offset.
        Returns device tensors (info [G, repeats, d], action [G, repeats, n, d-1] int32, R_hist [G, repeats, d-1, n, d-1],
        im_hist [G, repeats, d-1, M, n, d] or None when keep_im is false); slots past max_steps stay zero.
        max_blocks: workgroups per forward launch (0: the library's limit); ws_floats: bound of the reward workspaces (members
        go through them in chunks).  `launches`: the library's kernel launches of the call, `launches_per_step` of one step."""
        G, lay, d, Ld = self.G, self.lay, self.lay.d, self.lay.L
        n, steps, calls, R = acquire_plan(G, d, Ld, x.shape, M, repeats, max_steps, None if eps is None else eps.shape)
        L.require_cuda(x, eps)
        dev = self.dev
        c = self._setup(x, n, M, max_blocks=max_blocks)
        dk = c.xk.shape[-1]
        draws, seps = self._draws(eps, R, calls)
        draws = iter(draws)  # (offset, eps plane) of the forward calls in issue order
        info = torch.zeros(G, repeats, d, device=dev)
        action = torch.zeros(G, repeats, n, d - 1, dtype=torch.int32, device=dev)
        R_hist = torch.zeros(G, repeats, d - 1, n, d - 1, device=dev)
        im_hist = torch.zeros(G, repeats, d - 1, M, n, d, device=dev) if keep_im else None
        im_buf = None if keep_im else torch.empty(G, M, n, d, device=dev)
        sq = torch.empty(G, R, device=dev)
        mask = torch.zeros(G, n, d, dtype=torch.uint8, device=dev)
        maskk = mask if dk == d else torch.zeros(G, n, dk, dtype=torch.uint8, device=dev)
        sizes, chunk = self._reward_workspaces(n, M, ws_floats)
        f_launches, r_launches = forward_launches(c.tiles_dev.shape[0], G, max_blocks), 3 * ((G + chunk - 1) // chunk)
        strides = stride_vector(ops.MS_COUNT, {ops.MS_X: c.sxk, ops.MS_MASK: maskk.stride(0), ops.MS_EPS: seps, ops.MS_IMG: c.simg,
                                               **self._family_strides()})
        once = self._once_per_call()
        r_strides = self._reward_strides(c, mask, im_hist[:, 0, 0] if keep_im else im_buf, R_hist[:, 0, 0], sizes)

        def forward(mode, out, out_stride):
            offset, plane = next(draws)
            self._forward(c, strides, maskk, plane, offset, mode, out, out_stride)

        def curve_point(r, t):
            forward(1, sq, sq.stride(0))
            ops.target_mse_multi(sq, sq.stride(0), R, G, info[0, r, t:], info.stride(0))

        for r in range(repeats):
            if r > 0:
                mask.zero_()
                if maskk is not mask:
                    maskk.zero_()
            curve_point(r, 0)
            for t in range(steps):
                im = im_hist[:, r, t] if keep_im else im_buf
                forward(0, im[0], im.stride(0))
                Rt = R_hist[:, r, t]
                self._reward(c, r_strides, mask, im, Rt, chunk)
                ops.acquire_multi(Rt[0], Rt.stride(0), mask, mask.stride(0), d, None if maskk is mask else maskk,
                                  maskk.stride(0), dk, action[0, r, :, t:], action.stride(0), d - 1, G, n, d)
                curve_point(r, t + 1)
        self.launches_per_step = 2 * f_launches + r_launches + 2
        self.launches = once + repeats * (f_launches + 1 + steps * self.launches_per_step)
        return info, action, R_hist, im_hist


W23_FLOATS = 64 * 128 + 32 * 64  # [W2 | W3] at the tail of a packed encoder image (csrc/vpc_layout.h EncImg, oW2 .. total), any width


class _FamilyAcquirer(EnsembleAcquirer):
    """EnsembleAcquirer for a member family other than the plain one: run(), impute(), reward(), the draw rule and the launch
    accounting are EnsembleAcquirer's; members, images, pitch and for_trainer() are the family evaluator's (the class a subclass
    names first).  A subclass says which forward launch runs (_forward), which first-layer kind the reward has and where a
    member's W1 / b1 lie in its row of the parameter stack; [W2 | W3] is the tail of the member's encoder image."""
    kind = None  # ops.REWARD_*

    def _first_layer_cols(self):
        """Columns of W1 [100][.], which opens a member's row of the parameter stack with b1 [100] behind it."""
        raise NotImplementedError

    def _folded(self):
        """(AC of member 0, member stride, K) of the folded front-ends the reward reads; (None, 0, 0) for a kind without one."""
        return None, 0, 0

    def _reward_sizes(self, n, M):
        return ops.reward_scratch_multi_ex(self.kind, n, self.lay.d, M, self.lay.K)

    def _reward_strides(self, c, mask, im, R, sizes):
        return stride_vector(ops.RM_COUNT_EX, {
            ops.RM_X: c.sx, ops.RM_MASK: mask.stride(0), ops.RM_IM: im.stride(0), ops.RM_PARAM: self.params.stride(0),
            ops.RM_IMG: c.simg, ops.RM_PRE: sizes[0], ops.RM_STAT: sizes[1], ops.RM_W1T: sizes[2], ops.RM_R: R.stride(0),
            ops.RM_AC: self._folded()[1]})

    def _reward(self, c, strides, mask, im, R, chunk):
        lay = self.lay
        w1 = self.params[0]
        pre, stat, w1t = self._reward_ws
        AC, _, K = self._folded()
        ops.reward_matrix_multi_ex(self.kind, c.x, mask, im[0], w1, w1[100 * self._first_layer_cols():], AC, K,
                                   c.img0[lay.enc_img - W23_FLOATS:lay.enc_img], pre, stat, w1t, R[0], self.G, chunk, strides, c.n,
                                   lay.d, lay.L, c.M)


class MaskEnsembleAcquirer(MaskEnsembleEvaluator, _FamilyAcquirer):
    """EnsembleAcquirer for G Reg_VAE_mask or G vanilla_VAE_mask of one (obs_dim, latent_dim, reg_type): the loop of
    active_learning_func on VAE.py:570-580 / :1053-1060 through vpc_impute_small_multi_aug_f32 and vpc_reward_matrix_multi_ex
    (VPC_REWARD_DENSE_MASK).  W1 [100][2 obs_dim] / b1 open a member's row of the parameter stack; the images are the models' own,
    as under MaskEnsembleEvaluator."""
    kind = ops.REWARD_DENSE_MASK

    def _first_layer_cols(self):
        return 2 * self.lay.d

    def _forward(self, c, strides, maskk, eps_plane, offset, mode, out, out_stride):
        lay = self.lay
        ops.impute_small_multi_aug_f32(c.xk, maskk, eps_plane, c.img0[:lay.enc_img], c.img0[lay.enc_img:], self.table_dev, self.G,
                                       c.tiles_dev, c.tiles_dev.shape[0], c.n, c.M * c.n, eps_plane is None, offset,
                                       self.models[0]._x_logvar_value, mode, out, out_stride, strides, c.xk.shape[-1], lay.d,
                                       lay.L, c.max_blocks)


class EDDIEnsembleAcquirer(EDDIEnsembleEvaluator, _FamilyAcquirer):
    """EnsembleAcquirer for G Reg_EDDI or G vanilla_EDDI of one (obs_dim, emb_dim, latent_dim, reg_type): the loop on VAE.py:757-767
    / :935-950 through vpc_impute_small_multi_eddi_f32 and vpc_reward_matrix_multi_ex (VPC_REWARD_POINTNET).  W1 [100][emb_dim] /
    b1 = pnp_encoder2.0 open a member's row [trunk | decoder | front-end]; [W2 | W3] is the tail of the member's trunk image of the
    point-net layout (the evaluator's rows, or the trunk trainer's: for_trainer); the front-end is read in place and folded to
    AC [G][2][emb_dim][obs_dim] by ONE vpc_eddi_fold_multi launch per run() / reward() call - the parameters do not change inside
    a call - which `launches` counts."""
    kind = ops.REWARD_POINTNET

    def _first_layer_cols(self):
        return self.lay.K

    def _folded(self):
        return self._AC[0], self._AC.stride(0), self.lay.K

    def _once_per_call(self):
        lay = self.lay
        if getattr(self, "_AC", None) is None:
            self._AC = torch.empty(self.G, _pitch(2 * lay.K * lay.d), device=self.dev)
        ops.eddi_fold_multi(self.params[0, lay.n_params:], self.params.stride(0), self._AC, self._AC.stride(0), self.G, lay.d, lay.K)
        return 1

    def _forward(self, c, strides, maskk, eps_plane, offset, mode, out, out_stride):
        lay = self.lay
        ops.impute_small_multi_eddi_f32(c.xk, maskk, eps_plane, c.img0[:lay.enc_img], c.img0[lay.enc_img:], self.table_dev, self.G,
                                        c.tiles_dev, c.tiles_dev.shape[0], c.n, c.M * c.n, eps_plane is None, offset,
                                        self.models[0]._x_logvar_value, mode, out, out_stride, strides, c.xk.shape[-1], lay.d,
                                        lay.L, lay.K, self.params[0, lay.n_params:], c.max_blocks)
