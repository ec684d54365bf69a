"""What the step trainers (FusedTrainer, NMTrainer, EDDITrainer, WideTrainer, MIWTrainer, FlowTrainer, EDDIMnistTrainer)
share: Adam state on one flat parameter buffer and the Adam launch that closes a step, the flat bucket [grads | loss tail]
that data parallelism all-reduces in ONE collective, the deferred weight gradients of the GEMM chains (per-layer partials,
one reduction launch), timers, the loss readers and the capture / replay of a step as a HIP graph; and the counter rules of
the device draws, one function per rule.  (What NMTrainer, MIWTrainer and FlowTrainer share beyond this base - constructor,
workspace guard, chain wiring, input draws - is chainfamily._ChainTrainer.)"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib as L
from . import dist as dp_mod
from .images import flat_written
from .linear import linear_wgrad, wgrad_reduce
from .models import loss_coefficients
from .ops import adam_step


class Draws(NamedTuple):
    """Philox counters of one step's draws (draw_counters)."""
    offset_mask: int  # of the mask_p draw
    offset_eps: int  # of the eps planes
    next_offset: int  # the trainer's rng_offset after the step
    elem_lo: int  # index of this rank's first mask element inside the global [rows_global, row_width] array
    eps_shard: tuple  # (rows_local, rows_global, row_lo, pitch) as ops.draw_step / fill_normal / step_small_draw_f32 take it


def draw_counters(rng_offset, draw_mask, planes, rows_local, rows_global, row_lo, pitch, row_width):
    """THE counter rule of the dense-VAE step's draws, for every trainer that makes them.  mask_p
    comes first: one Philox call serves 8 bytes of the GLOBAL [rows_global, row_width] array, and the draw consumes one
    counter per 8 elements of that array, rounded up, and one more.  Then `planes` eps planes of `pitch` floats per row,
    one call per 4 floats.  Counters advance by what the GLOBAL batch consumes, so all ranks stay on one stream and a row's
    draws do not depend on the world size.  No mask draw: offset_mask == offset_eps == rng_offset; planes may be 0."""
    offset_eps = rng_offset + ((rows_global * row_width + 7) // 8 + 1 if draw_mask else 0)
    return Draws(rng_offset, offset_eps, offset_eps + planes * rows_global * (pitch // 4), row_lo * row_width,
                 (rows_local, rows_global, row_lo, pitch))


def chain_draw_increment(eps_floats, rows, row_width):
    """THE counter rule of the chain-backed steps' draws (NMTrainer, MIWTrainer, FlowTrainer, MIWEnsembleTrainer): what one
    step adds to the trainer's rng_offset.  The eps planes sit on their own stream position (rng_offset + 2^40) and take one
    Philox call per 4 floats of `eps_floats`, rounded up; the float mask_p draw takes one call per 4 elements of the
    [rows, row_width] array, rounded up, and one more.  Both streams advance by the sum, so no step reuses a counter of
    either.  Data parallel (NMTrainer): eps_floats and rows are those of the GLOBAL batch, so all ranks stay on one stream;
    every other caller passes its own."""
    return (eps_floats + 3) // 4 + (rows * row_width + 3) // 4 + 1


def eval_draw_counters(rng_offset, draw_rows, pitch=16):
    """THE counter rule of the ensemble evaluation's draws: one call draws eps for `draw_rows` rows
    (every row of every batch of every MC pass, in tile-table order) of `pitch` floats, one Philox call per 4 floats, on the
    eps stream with the member's seed.  The group of draw row r, columns 4 q .. 4 q + 3, has counter offset + r * (pitch / 4) + q:
    what ops.fill_normal(flat [draw_rows * pitch], seed, offset) writes at float index r * pitch + 4 q.
    Returns (offset of this call, the evaluator's rng_offset after it)."""
    return rng_offset, rng_offset + draw_rows * (pitch // 4)


def flow_eval_draw_counters(rng_offset, rows):
    """THE counter rule of the batched flow evaluation's draws (flow.FlowEvaluator): one evaluate call
    draws eps [rows][10] for every row of every batch of every MC pass, in tile-table order, as ONE flat array of 10 * rows
    floats on the eps stream with the evaluator's seed: one Philox call per 4 floats, the group of flat floats 4 q .. 4 q + 3 at
    counter offset + q - what ops.fill_normal(flat [10 * rows], seed, offset) writes.  A draw is a function of (seed, offset,
    flat index) alone: not of the tile table, nor of how the evaluator splits the rows into chunks.
    Returns (offset of this call, the evaluator's rng_offset after it = offset + ceil(10 * rows / 4))."""
    return rng_offset, rng_offset + (10 * rows + 3) // 4


def impute_draw_counter(offset, row0, row, sample, latent):
    """THE counter rule of the streaming MIWAE imputation's draws (miw_imp_ctr of csrc/vpc_rng.h):
    the 64-bit Philox counter of latent components 4 g .. 4 g + 3 (g = latent // 4) of `sample` of data row row0 + row is
    ((offset + row0 + row) << 32) | (4 * sample + g); the plane picks the Philox stream (5: the sampler's eps, 6: the fresh
    draw), the component its Box-Muller output (0, 1: radius of word x, cos / sin of word y; 2, 3: words z, w).  A function
    of (seed, offset, plane, row0 + row, sample, latent) alone - not of s_chunk, the grid or the workgroup that draws.
    offset + row0 + B <= 2^32 and sample < 2^28.  A call on B rows uses the high words offset + row0 .. offset + row0 + B - 1,
    so a caller that adds B to its offset after every call (harness.eval_miwae) never reuses a counter.
    Returns (counter, component)."""
    return ((offset + row0 + row) << 32) | (4 * sample + latent // 4), latent % 4


def padded_width(d, mask_augm=False):
    """Row pitch of the kernels' x / mask arrays: d rounded up to a multiple of 4 columns, so that the 16-byte-vector kernel
    variants run (FusedTrainer.step says why); the mask-augmented layouts take their rows unpadded (on the row-tiled path:
    their small-batch step pads by ops.small_aug_pitch)."""
    return d if (d % 4 == 0 or mask_augm) else 4 * ((d + 3) // 4)


def pad_cols(pads, t, dk, slot, dev):
    """[..., B, d] -> zero-padded [..., B, dk]: a persistent buffer per input slot, kept in the dict `pads`."""
    key = (slot, tuple(t.shape[:-1]), dk, t.dtype)
    buf = pads.get(key)
    if buf is None:
        buf = pads[key] = torch.zeros(*t.shape[:-1], dk, dtype=t.dtype, device=dev)
    buf[..., :t.shape[-1]].copy_(t)
    return buf


class _FlatAdamTrainer:
    timer_every = 1  # with timers enabled: bracket the launches of every timer_every-th step only
    step_timers = False  # the step brackets its GEMM-chain launches and Adam (NMTrainer, MIWTrainer, FlowTrainer); with timers
    # enabled its weight gradients then keep the per-layer form, so that every entry brackets a complete gradient
    prec = 0  # GEMM precision of the chains (ops.PRECISIONS)

    def __init__(self, model, lr, betas, eps, seed, process_group, world_size, rank, tail, collective=None):
        self.model = model
        self.lr, self.betas, self.adam_eps = lr, betas, eps
        self.seed, self.rng_offset, self.step_count = seed, 0, 0
        self.pg, self.world_size, self.rank = process_group, world_size, rank
        self.collective = collective
        self._coll_ready = collective is not None
        flat = model.flatten_parameters()
        L.require_cuda(flat)
        self.dev = flat.device
        n = flat.numel()
        # one flat bucket: [grads (n) | loss terms (tail)] -> a single all-reduce per step under DP
        self.bucket = torch.zeros(n + tail, device=self.dev)
        self.grad, self.tail = self.bucket[:n], self.bucket[n:]
        self.exp_avg = torch.zeros(n, device=self.dev)
        self.exp_avg_sq = torch.zeros(n, device=self.dev)
        self.accum = torch.zeros(1, device=self.dev)
        self.timers = None  # bench.py sets this to {} to collect per-kernel HIP event pairs
        self.timer_names = None  # restrict the event pairs to these launches (None = all)
        self._timer_tick = 0
        self._plist = model.trainable()
        self._repacked = ()
        # the trainable tensors' .grad are views of the flat gradient, so state is inspectable like torch's
        off = 0
        for p in self._plist:
            p.grad = self.grad[off:off + p.numel()].view_as(p)
            off += p.numel()

    def coefficients(self, epoch, alpha, beta, beta_annealing):
        return loss_coefficients(self.model, epoch, alpha, beta, beta_annealing)

    def train_step(self, x, mask, *, epoch, alpha, beta, beta_annealing, p_missingness, stage):
        """One batch of harness.train's fused loop: step() with what this trainer's step takes from the schedule (here all
        but stage; NMTrainer, MIWTrainer and FlowTrainer take less)."""
        return self.step(x, mask, epoch=epoch, alpha=alpha, beta=beta, beta_annealing=beta_annealing,
                         p_missingness=p_missingness)

    def _batch_rows(self, B, global_batch=None, row_lo=None):
        """(rows of the global batch, global index of this rank's first row): by default B * world_size rows of which this
        rank holds [rank * B, (rank + 1) * B)."""
        Bg = global_batch if global_batch is not None else B * self.world_size
        if row_lo is None:
            row_lo = self.rank * B if self.world_size > 1 else 0
        if row_lo < 0 or row_lo + B > Bg:
            raise ValueError(f"rows [{row_lo}, {row_lo + B}) are not inside the global batch of {Bg}")
        return Bg, row_lo

    def _timed(self, name, fn, *args, **kw):
        """Run one launch; with timers enabled bracket it with events on the launch stream."""
        if self.timers is None or self._timer_tick % self.timer_every or \
                (self.timer_names is not None and name not in self.timer_names):
            return fn(*args, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn(*args, **kw)
        e1.record()
        self.timers.setdefault(name, []).append((e0, e1))
        return r

    def _wgrad_workspace(self, shapes, grads, sized=True):
        """The per-layer partial buffers of the weight gradients `grads` [(dw, db)] of GEMMs `shapes` [(M, N, K)]: one
        buffer, sliced; summed by ONE launch at the end of the backward pass (_wgrad_reduce).  sized = False: empty slices
        (a path that leaves the GEMM chain out)."""
        sizes = [int(L.lib().vpc_linear_wgrad_scratch(*sh)) if sized else 0 for sh in shapes]
        buf = torch.empty(sum(sizes), device=self.dev)
        self._wg, o = [], 0
        for n, sh, (dw, db) in zip(sizes, shapes, grads):
            self._wg.append((buf[o:o + n], *sh, dw, db, False))
            o += n
        self._wg_cache = {}  # (buffers and gradient views are fixed for a batch size: the reduce's argument arrays are built once)

    def _wgrad(self, key, dy, x, y_gate=None, gate=0, gate_split=0):
        """Weight gradient key = (timer name, index in the workspace): partials now, summed by _wgrad_reduce; with timers on
        (step_timers) the complete gradient in this launch."""
        sc, M, N, K, dw, db, _ = self._wg[key[1]]
        if self.timers is not None and self.step_timers:
            return self._timed(key[0], linear_wgrad, dy, x, dw, db, M, N, K, y_gate, gate, gate_split, precision=self.prec)
        linear_wgrad(dy, x, None, None, M, N, K, y_gate, gate, gate_split, precision=self.prec, scratch=sc)

    def _wgrad_reduce(self):
        if self.timers is None or not self.step_timers:
            wgrad_reduce(self._wg, self._wg_cache)

    def _adam(self, state=None, loss_in=None, accum=None):
        """The step's tail: flat Adam on model._flat, then images.py's rule for a launch that wrote the parameters."""
        self.step_count += 1
        args = (self.model._flat, self.grad, self.exp_avg, self.exp_avg_sq, self.step_count, self.lr, self.betas[0],
                self.betas[1], self.adam_eps, None, None, state, loss_in, accum)
        if self.step_timers:
            self._timed("adam", adam_step, *args)
        else:
            adam_step(*args)
        self._flat_written(None)

    def _flat_written(self, key, *repacked):
        """After a launch that wrote the flat parameters (Adam): images.py's rule.  `key`: this step's parameter key."""
        flat_written(self.model, self._plist, key, repacked)
        self._repacked = repacked

    def _collective(self):
        if not self._coll_ready:
            self.collective = dp_mod.make_collective(self.world_size, self.rank, self.dev, self.pg)
            self._coll_ready = True
        return self.collective

    def _allreduce(self):
        """ONE collective per step over the flat bucket [grads | loss terms]: ncclAllReduce (RCCL over xGMI) on the
        compute stream when the process group is NCCL, torch.distributed.all_reduce otherwise (dist.py).  Every term
        is already normalised by the GLOBAL batch, so a plain SUM is the result of the concatenated batch."""
        dp_mod.allreduce_bucket(self.bucket, self.pg, self._collective())

    def _graph_step(self, key, inputs, step):
        """step_graph's body.  The first call with a new `key` runs step(*inputs) eagerly (LDS attributes, workspaces,
        packed images) and captures step(*copies of inputs, _state=self.state); later calls copy the inputs into the
        captured buffers and replay.  Step count and Philox offsets live on the device (`state`): kernel arguments are
        frozen in a graph."""
        if getattr(self, "_graph_key", None) != key:
            step(*inputs)
            self._ginputs = [t.clone() for t in inputs]
            self.state = torch.tensor([self.step_count, 0], dtype=torch.int64, device=self.dev)
            timers, self.timers = self.timers, None
            host = (self.rng_offset, self.step_count, self._timer_tick)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step(*self._ginputs, _state=self.state)
            self._graph_rng_inc = self.rng_offset - host[0]
            self.rng_offset, self.step_count, self._timer_tick = host  # capture executed nothing
            self.timers = timers
            self._graph, self._graph_key, self._graph_repacked = g, key, self._repacked
            return
        for src, dst in zip(inputs, self._ginputs):
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src)
        self._graph.replay()
        self.step_count += 1
        self.rng_offset += self._graph_rng_inc
        self._flat_written(None, *self._graph_repacked)

    def loss_value(self) -> float:
        """Loss of the last step (host sync)."""
        return float(self.tail[0].item())

    def epoch_total(self, reset=True) -> float:
        """Sum of train_loss over the steps since the last reset (train.py:117-118; one host sync per epoch)."""
        v = float(self.accum.item())
        if reset:
            self.accum.zero_()
        return v
