"""What the chain-backed families (notmiwae.py, miwae.py, flow.py) share around the chain walkers of linear.py.  Each is a
FlatParams model whose encoder and decoder are GEMM chains, with the family's sampler between them and its loss behind them,
and a trainer that runs the q and p passes stacked along the batch.  Here, once:

  * the elementwise ops every family borrows (nm_mul, nm_prep, nm_sample, nm_sample_bwd, the one-sample Gaussian sampler),
  * ChainEncoderFn / ChainDecoderFn: the autograd frame (buffers, walkers, save_for_backward, gradient views), driven by the
    family's `Family` record, which states the launches that differ.  The eager path of the wide dense classes (wide.py) and
    of the two point-net families (eddi.py, eddi_mnist.py) runs on it too; their trainers keep their own frames,
  * _ChainTrainer: constructor, workspace guard, chain wiring, weight-gradient workspace, the inject-or-draw input step,
  * impute_stream: the host side of the streaming imputation kernels, with impute_chunk and impute_draws,
  * _ReferenceAttrs: the constructor prologue of the MNAR and MIWAE model classes.

Imports none of the family modules (DESIGN.md section 2.32 says where a new family plugs in)."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib as L
from ._lib import VpcError, check, lib, ptr, require_cuda, stream_ptr
from .linear import ACT_SIGMOID_HARDTANH, _f32c, chain_buffers, chain_bwd, chain_fwd, wgrad_now, wgrad_now_keys
from .ops import fill_normal
from .trainer import _FlatAdamTrainer

STREAM_MAX_L = 16  # latent limit of the streaming imputation kernels and of their draws


# ------------------------------------------------------------------------------------------------ raw ops
def nm_sample(heads, eps, z, B, K, Ld):
    check(lib().vpc_nm_sample(ptr(heads), 2 * Ld, ptr(eps), ptr(z), Ld, B, K, Ld, stream_ptr()), "vpc_nm_sample")


def nm_sample_bwd(dz, eps, heads, g_heads, out, B, K, Ld):
    check(lib().vpc_nm_sample_bwd(ptr(dz), Ld, ptr(eps), ptr(heads), 2 * Ld, ptr(g_heads), 2 * Ld, ptr(out), 2 * Ld, B,
                                  K, Ld, stream_ptr()), "vpc_nm_sample_bwd")


def gauss_sample(heads, eps, B, S, Ld):
    """The sampler of the dense and point-net families: one z = mean + eps * exp(logvar / 2) per row (eps None: the mean)
    -> (z [B, L], heads [B, mean L | logvar L]); encoder() splits the heads.  VAE.py:387-395."""
    z = torch.empty(B, Ld, device=heads.device)
    nm_sample(heads, eps, z, B, 1, Ld)
    return z, heads


def gauss_sample_bwd(heads, eps, dz, dheads, out, B, S, Ld):
    nm_sample_bwd(torch.zeros(B, Ld, device=heads.device) if dz is None else dz, eps, heads, dheads, out, B, 1, Ld)


def nm_mul(x, mask, out):
    check(lib().vpc_nm_mul(ptr(x), ptr(mask), ptr(out), out.numel(), stream_ptr()), "vpc_nm_mul")


def nm_prep(x, mask, mask_p_out, xin, B, d, keep_prob, seed, offset, eps_out=None, offset_eps=0, state=None,
            elem_lo=0, eps_shard=None):
    """eps_shard = (rows_local, rows_global, row_lo, pitch) of eps_out as rows of a global batch (None: flat)."""
    sh = (0, 0, 0, 4) if eps_shard is None else tuple(int(v) for v in eps_shard)
    check(lib().vpc_nm_prep(ptr(x), ptr(mask), ptr(mask_p_out), ptr(xin), B, d, float(keep_prob), ptr(eps_out),
                            0 if eps_out is None else eps_out.numel(), int(seed), int(offset), int(offset_eps),
                            ptr(state), int(elem_lo), *sh, stream_ptr()), "vpc_nm_prep")


def miw_impute_draws(eps_out, B, S, Ld, seed, offset, row0):
    check(lib().vpc_miw_impute_draws(ptr(eps_out), int(B), int(S), int(Ld), int(seed), int(offset), int(row0),
                                     stream_ptr()), "vpc_miw_impute_draws")


def _joined(parts, M, W):
    """n [.., W] tensors that are the adjacent column blocks of ONE [M, n W] buffer -> that buffer, else None."""
    a, n = parts[0], len(parts)
    stride, p0 = a.stride(), a.data_ptr()
    for i, t in enumerate(parts):
        if t.dtype != torch.float32 or not t.is_cuda or t.stride() != stride or t.data_ptr() != p0 + 4 * W * i:
            return None
    if a.dim() < 2 or stride[-1] != 1 or stride[-2] != n * W or \
            any(stride[i] != stride[i + 1] * a.shape[i + 1] for i in range(a.dim() - 2)):
        return None
    return a.as_strided((M, n * W), (n * W, 1))


# ------------------------------------------------------------------------------------------------ autograd
class Family(NamedTuple):
    """What differs between the families in the encoder / decoder Functions; one instance per family, next to its raw ops."""
    enc_names: tuple  # W1, b1, W2, b2, .. of the encoder chain in the model's named views
    dec_names: tuple
    enc_input: object  # (x, mask, out, B, d, *front weights): the launch that writes the encoder chain's input
    sample: object  # (heads, eps, B, S, Ld) -> the encoder's two outputs (allocates z, launches the sampler)
    sample_bwd: object  # (heads, eps, dz, d_second, out, B, S, Ld); dz / d_second: contiguous fp32 or None
    dec_blocks: int  # the decoder returns this many column blocks, obs_dim wide, of one buffer
    dec_heads: object = None  # None: the chain's last activation is an output gate passed to chain_bwd (Sigmoid | Hardtanh);
    # else (fwd(y_raw, M, d) -> activated buffer, bwd(y_raw, g_act, g_raw, M, d)): a head-activation launch pair
    input_bwd: object = None  # the point-net families, whose input op has n_front parameters of its own (the segment "front",
    n_front: int = 0  # the LAST weights of apply()): enc_input returns the tensors its backward reads again, and
    # input_bwd(saved, d_input, g, B, d) writes the front gradients g[name] from the gradient of the chain's input


class ChainEncoderFn(torch.autograd.Function):
    """(x, mask, eps) -> the family's (z, heads / activated heads / z_log_prob): input op, encoder chain, sampler."""

    @staticmethod
    def forward(ctx, fam, model, x, mask, eps, S, *weights):
        require_cuda(x, mask, eps, *weights)
        B, dev = x.shape[0], x.device
        layers = model._chains()[0]
        acts = chain_buffers(layers, B, dev)
        front = fam.enc_input(x, mask, acts[0], B, model.obs_dim, *weights[len(weights) - fam.n_front:])
        chain_fwd(layers, acts, B)
        out = fam.sample(acts[-1], eps, B, S, model.latent_dim)
        ctx.fam, ctx.model, ctx.S, ctx.has_eps, ctx.nw, ctx.layers = fam, model, S, eps is not None, len(weights), layers
        ctx.save_for_backward(*acts, eps if eps is not None else torch.empty(0, device=dev), *(front or ()))
        return out

    @staticmethod
    def backward(ctx, dz, d2):
        fam, model, layers = ctx.fam, ctx.model, ctx.layers  # (the forward's chain, kept: model._chains() is a flatten check per call)
        saved, n = ctx.saved_tensors, len(layers) + 1
        acts, eps, front = saved[:n], saved[n], saved[n + 1:]  # (front: what enc_input returned; empty but for the point-nets)
        B, dev = acts[0].shape[0], acts[0].device
        dacts = chain_buffers(layers, B, dev, first=None if front else False)
        fam.sample_bwd(acts[-1], eps if ctx.has_eps else None, None if dz is None else _f32c(dz),
                       None if d2 is None else _f32c(d2), dacts[-1], B, ctx.S, model.latent_dim)
        g = model._segment_views(torch.empty(model._n_enc, device=dev), "enc")
        chain_bwd(layers, acts, dacts, B, wgrad_now, wgrad_now_keys(layers, g, fam.enc_names, B), input_grad=bool(front))
        grads = tuple(g.values())[:ctx.nw - fam.n_front]  # (_segment_views: the segment's tensors in order, then the aliases)
        if front:
            g = model._segment_views(torch.empty(model._flat_table()[2]["front"][3], device=dev), "front")
            fam.input_bwd(front, dacts[0], g, B, model.obs_dim)
            grads += tuple(g.values())
        return (None,) * 6 + grads


class ChainDecoderFn(torch.autograd.Function):
    """z [.., L] -> the fam.dec_blocks column blocks of ONE [M, blocks * d] buffer (one block: the buffer itself)."""

    @staticmethod
    def forward(ctx, fam, model, z, *weights):
        require_cuda(z, *weights)
        d, n = model.obs_dim, fam.dec_blocks
        lead = z.shape[:-1]
        z2 = _f32c(z)
        if z2.dim() != 2:  # (a view per call is 1 - 2 us of host time: made only where the shape asks for one)
            z2 = z2.reshape(-1, model.latent_dim)
        M = z2.shape[0]
        layers = model._chains()[1]
        acts = chain_buffers(layers, M, z2.device, first=z2)
        chain_fwd(layers, acts, M)
        Y = acts[-1] if fam.dec_heads is None else fam.dec_heads[0](acts[-1], M, d)
        ctx.fam, ctx.model, ctx.lead, ctx.nw, ctx.layers = fam, model, lead, len(weights), layers
        ctx.save_for_backward(*acts)
        Y3 = Y if len(lead) == 1 else Y.view(*lead, n * d)
        return Y3 if n == 1 else tuple(Y3[..., i * d:(i + 1) * d] for i in range(n))

    @staticmethod
    def backward(ctx, *grads):
        fam, model, layers = ctx.fam, ctx.model, ctx.layers
        acts = ctx.saved_tensors
        d = model.obs_dim
        M, dev = acts[0].shape[0], acts[0].device
        # the fused losses hand back the column blocks of one [M, blocks * d] buffer: use it in place
        parts = [torch.zeros(M, d, device=dev) if t is None else t for t in grads]
        G = _f32c(parts[0]) if len(parts) == 1 else _joined(parts, M, d)
        if len(parts) == 1 and G.dim() != 2:
            G = G.reshape(M, d)
        if G is None:
            G = torch.cat([_f32c(t).reshape(M, d) for t in parts], 1)
        g = model._segment_views(torch.empty(model._n_dec, device=dev), "dec")
        wkeys = wgrad_now_keys(layers, g, fam.dec_names, M)
        if fam.dec_heads is None:
            dacts = chain_buffers(layers, M, dev, last=G)
            chain_bwd(layers, acts, dacts, M, wgrad_now, wkeys, y_gate=acts[-1], gate=ACT_SIGMOID_HARDTANH, gate_split=d)
        else:
            dacts = chain_buffers(layers, M, dev)
            fam.dec_heads[1](acts[-1], G, dacts[-1], M, d)
            chain_bwd(layers, acts, dacts, M, wgrad_now, wkeys)
        dz = dacts[0] if len(ctx.lead) == 1 else dacts[0].view(*ctx.lead, model.latent_dim)
        return (None, None, dz) + tuple(g.values())[:ctx.nw]


# ------------------------------------------------------------------------------------------------ model classes
class _ReferenceAttrs:
    """Constructor prologue of the MNAR and MIWAE classes: the kernels' shape limit and the reference's attributes."""

    def _init_reference_attrs(self, path, obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates):
        if obs_dim > 256 or latent_dim > 64:
            raise VpcError(f"the {path}-path kernels support obs_dim <= 256 and latent_dim <= 64")
        self.obs_dim = obs_dim
        self.hid_dim = hid_dim
        self.emb_dim = 10
        self.num_samples = num_samples
        self.num_estimates = num_estimates
        self.latent_dim = latent_dim
        self.batch_size = training_parameters["batch_size"]
        self.K = K
        self.obs_std = 0.1
        self.number_components = 500
        self.training_paramters = training_parameters  # (sic) VAE.py:2341 / :3024


# ------------------------------------------------------------------------------------------------ streaming imputation
def impute_chunk(B, S, n_cu):
    """The default s_chunk of impute_stream: the samples of a row one workgroup owns, a multiple of 16 and never below 16.
    A rule that was measured, not derived (profiles/miw_impute_notes.md, d = 12, L = 10, S = 5 000, 256 compute units;
    kept for the MNAR kernel by the sweep of profiles/nm_impute_notes.md):

      * B < n_cu: as few chunks per row as still give one workgroup per compute unit - the chunks of the largest multiple
        of 16 with B * ceil(S / s_chunk) >= n_cu (every further chunk repeats the encoder and the weight-fragment loads:
        B = 64 is fastest at 4 chunks, slower at 5, 10, 20, 40, 79) -
      * B >= n_cu: whole rows, unless the last round of n_cu workgroups would be less than 95 % full; then 2 or 4 chunks
        per row (B = 1 600: 6.25 rounds of whole rows, 7 % slower than 12.5 rounds of half rows),
      * and in both cases the chunks of a row balanced: the smallest multiple of 16 that keeps that number of chunks (4
        chunks of S = 5 000 as 3 x 1 664 + 8 are 30 % slower than as 3 x 1 264 + 1 208)."""
    B, S, n_cu = max(int(B), 1), max(int(S), 1), max(int(n_cu), 1)
    tiles = -(-S // 16)
    if B < n_cu:
        need = -(-n_cu // B)  # chunks per row for one workgroup per compute unit
        chunks = -(-S // max(16, (S - 1) // (need - 1) // 16 * 16))
    else:
        for chunks in (1, 2, 4):
            rounds = B * chunks / n_cu
            if rounds >= 0.95 * -(-B * chunks // n_cu):
                break
        chunks = min(chunks, tiles)
    return 16 * -(-(-(-S // chunks)) // 16)  # ceil(S / chunks), rounded up to a multiple of 16


def impute_draws(B, S, L, seed, offset=0, row0=0, device=None):
    """The draws of impute_stream(seed=seed, offset=offset, row0=row0) on B rows with S samples as [2, B, S, L]: plane 0
    the sampler's eps, plane 1 the fresh draw of the log-weight's prior / posterior term (the counter rule of
    trainer.impute_draw_counter).  (L, the latent width, hides the module's alias of _lib in here.)"""
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda":
        raise VpcError("impute_draws runs only on the GPU (HIP kernel, no CPU fallback)")
    if not (B >= 1 and S >= 1 and 1 <= L <= STREAM_MAX_L):
        raise VpcError(f"impute_draws: B = {B}, S = {S}, latent_dim = {L} outside B >= 1, S >= 1, latent_dim <= {STREAM_MAX_L}")
    eps = torch.empty(2, B, S, L, device=dev)
    with torch.cuda.device(dev):
        miw_impute_draws(eps, B, S, L, seed, offset, row0)
    return eps


def stream_seed(seed):
    """The seed of a streaming imputation's device draws: None takes one from torch's generator."""
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else seed


@torch.no_grad()
def impute_stream(model, x, mask, num_samples, eps, seed, offset, row0, s_chunk, return_lse, max_d, max_l, scratch, launch):
    """The host side of a streaming imputation kernel (miwae.impute_stream and notmiwae.impute_stream document the call):
    shape and limit checks, the s_chunk default, the seed, the partial buffer of `scratch(B, S, d, L, s_chunk)` floats, then
    launch(flat, x, mask, eps, seed, offset, row0, part, xm, lse, B, S, d, L, s_chunk)."""
    d, Ld = model.obs_dim, model.latent_dim
    S = model.num_samples if num_samples is None else int(num_samples)
    require_cuda(x, mask, eps)
    if not (1 <= d <= max_d and 1 <= Ld <= max_l):
        raise VpcError(f"impute_stream supports obs_dim <= {max_d} and latent_dim <= {max_l}: got {d}, {Ld}")
    xf, mf = _f32c(x.reshape(-1, d)), _f32c(mask.reshape(-1, d))
    B = xf.shape[0]
    if B < 1 or S < 1 or mf.shape != xf.shape:
        raise VpcError(f"impute_stream: B = {B}, num_samples = {S}, mask {tuple(mf.shape)} for x {tuple(xf.shape)}")
    if s_chunk is None:
        s_chunk = impute_chunk(B, S, L.max_blocks() // 2)
    if s_chunk < 1:
        raise VpcError(f"impute_stream: s_chunk = {s_chunk} < 1")
    if eps is not None:
        if tuple(eps.shape) != (2, B, S, Ld):
            raise VpcError(f"impute_stream: eps {tuple(eps.shape)}, expected {(2, B, S, Ld)}")
        eps = _f32c(eps)
    else:
        seed = stream_seed(seed)
    n = scratch(B, S, d, Ld, s_chunk)
    if n == 0:
        raise VpcError(f"impute_stream: shape (B, S, d, L) = {(B, S, d, Ld)} is outside the kernel's limits")
    flat = model.flatten_parameters()
    require_cuda(flat)
    with torch.cuda.device(xf.device):
        part = torch.empty(n, device=xf.device)
        xm = torch.empty(B, d, device=xf.device)
        lse = torch.empty(B, device=xf.device) if return_lse else None
        launch(flat, xf, mf, eps, seed or 0, offset, row0, part, xm, lse, B, S, d, Ld, s_chunk)
    return (xm, lse) if return_lse else xm


# ------------------------------------------------------------------------------------------------ fused step
class _ChainTrainer(_FlatAdamTrainer):
    """The frame of NMTrainer, MIWTrainer and FlowTrainer.  A family class states `family`, `model_base`, `model_names`,
    `single_process` (why it refuses world_size != 1; None: data parallel) and _buffers(); its step() runs on the wiring
    _ws leaves: enc_layers / dec_layers, enc_acts / enc_dacts, dec_acts / dec_dacts and the weight-gradient workspace."""
    step_timers = True
    single_process = None
    use_nmdec = False  # (NMTrainer: the GEMM chains are left out of the step, their workspaces are empty)

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, process_group=None, world_size=1, rank=0):
        name = type(self).__name__
        if not isinstance(model, self.model_base):
            raise TypeError(f"{name} supports {self.model_names}")
        if self.single_process and world_size != 1:
            raise VpcError(f"{name} is single-process: {self.single_process}")
        super().__init__(model, lr, betas, eps, seed, process_group, world_size, rank, 1)
        self.reg = model.regularised
        self.out8 = torch.zeros(8, dtype=torch.float64, device=self.dev)
        self.g = model._named_views(self.grad)
        self._B = self._v = None

    def _ws(self, B, v=None):
        """The step's workspace for batch B, made once per (batch size, flat parameter buffer)."""
        v = self.model._views() if v is None else v
        if self._B == B and self._v is v:
            return
        dev = self.dev
        R, M, self.enc_acts, self.enc_dacts, self.dec_acts, self.dec_dacts = \
            self._buffers(B, lambda *s: torch.empty(*s, device=dev))
        # the two GEMM chains on their workspaces, and the per-layer partials of the weight gradients in the backward pass's
        # launch order: the decoder's last layer first, on M rows; then the encoder's, on R rows
        self.enc_layers, self.dec_layers = self.model._chains()
        g, fam = self.g, self.family
        back = [(M, l) for l in self.dec_layers[::-1]] + [(R, l) for l in self.enc_layers[::-1]]
        names = fam.dec_names[::-1] + fam.enc_names[::-1]  # b, W of the last decoder layer, ..
        self._wgrad_workspace([(rows, l[3], l[2]) for rows, l in back], [(g[w], g[b]) for w, b in zip(names[1::2], names[0::2])],
                              sized=not self.use_nmdec)
        self._B, self._v = B, v

    def _buffers(self, B, e):
        """Family hook: allocate the step's buffers for batch B with e(*shape) -> (stacked rows R, decoder rows M, enc_acts,
        enc_dacts, dec_acts, dec_dacts)."""
        raise NotImplementedError

    def train_step(self, x, mask, *, alpha, p_missingness, **schedule):
        return self.step(x, mask, alpha=alpha, p_missingness=p_missingness)

    def _draw_inputs(self, xf, mf, mask_p, eps, B, d, p_missingness, rng_inc, _state=None, rank_off=0, eps_shard=None,
                     elem_lo=0):
        """The step's inputs, where mask_p is a float mask and the encoder input x * mask: an injected mask_p (nm_mul per
        pass, device normals unless eps is injected too) or the device draw (one launch: mask_p + stacked encoder input +
        normals); then the injected eps, then the counters.  Returns the mask_p the step reads (None: not regularised)."""
        if self.reg and mask_p is not None:
            mp = _f32c(mask_p.reshape(-1, d))
            nm_mul(xf, mf, self.xin[:B])
            nm_mul(xf, mp, self.xin[B:])
            if eps is None:
                fill_normal(self.eps, self.seed, self.rng_offset + (1 << 40) + rank_off, _state, eps_shard)
        else:
            mp = self.mask_p if self.reg else None
            self._timed("prep", nm_prep, xf, mf, mp, self.xin, B, d, 1.0 - p_missingness / 100.0, self.seed,
                        self.rng_offset + rank_off, self.eps if eps is None else None,
                        self.rng_offset + (1 << 40) + rank_off, _state, elem_lo, eps_shard)
        if eps is not None:
            self.eps.copy_(eps.reshape(self.eps.shape))
        self.rng_offset += rng_inc
        return mp
