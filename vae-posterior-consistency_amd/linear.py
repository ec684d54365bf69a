"""The generic fp32 MFMA GEMM layer ops (csrc/vpc_gemm.hip), their few-row form (csrc/vpc_rows.hip: M <= 128 rows, split over
output features, one backward launch per layer) and the walkers of an MLP chain built from either.  A leaf module: every model
family imports from here.

A chain is an ordered list of layers `(w, b, K_in, N_out, act, split)`; its activations are a list `acts` with `acts[0]` the
chain's input and `acts[i + 1]` the output of layer i, and `dacts` the gradients laid out the same way (`dacts[i + 1]` is
d loss / d pre-activation of layer i once the GEMM below it has applied the gate).  Both walkers are plain loops over what
the caller prebuilt: no tensor view is made per layer."""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import check, lib, ptr, stream_ptr

ACT_NONE, ACT_ELU, ACT_SIGMOID_HARDTANH, ACT_RELU = 0, 1, 2, 3


def _f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def linear_fwd(x, w, b, y, M, N, K, act=ACT_NONE, split=0, ldx=None, ldy=None, precision=0):
    check(lib().vpc_linear_fwd(ptr(x), ldx or K, ptr(w), ptr(b), ptr(y), ldy or N, M, N, K, act, split, int(precision),
                               stream_ptr()), "vpc_linear_fwd")


def linear_dgrad(dy, w, dx, M, N, K, y_gate=None, gate=ACT_NONE, gate_split=0, x_out=None, act_prev=ACT_NONE,
                 lddy=None, lddx=None, ldyg=None, ldxo=None, precision=0):
    """Row pitches default to the dense width; ldyg (y_gate) defaults to dy's pitch, ldxo is x_out's."""
    check(lib().vpc_linear_dgrad(ptr(dy), lddy or N, ptr(y_gate), ldyg or lddy or N, gate, gate_split, ptr(w), ptr(x_out),
                                 ldxo or K, act_prev, ptr(dx), lddx or K, M, N, K, int(precision), stream_ptr()),
          "vpc_linear_dgrad")


_scratch = {}


def _wgrad_scratch(device, floats):
    key = str(device)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < floats:
        buf = torch.empty(max(floats, 1 << 20), device=device)
        _scratch[key] = buf
    return buf


def linear_wgrad(dy, x, dw, db, M, N, K, y_gate=None, gate=ACT_NONE, gate_split=0, accumulate=False, lddy=None,
                 ldx=None, ldyg=None, precision=0, scratch=None):
    """dw = None: write only the per-split partials into `scratch` (the caller's own buffer for this layer); they are summed
    later, together with other layers', by wgrad_reduce (one launch).  ldyg (y_gate's row pitch) defaults to dy's."""
    sc = _wgrad_scratch(dy.device, int(lib().vpc_linear_wgrad_scratch(M, N, K))) if scratch is None else scratch
    check(lib().vpc_linear_wgrad(ptr(dy), lddy or N, ptr(y_gate), ldyg or lddy or N, gate, gate_split, ptr(x), ldx or K,
                                 ptr(dw), ptr(db), ptr(sc), sc.numel(), M, N, K, int(accumulate), int(precision),
                                 stream_ptr()), "vpc_linear_wgrad")


def wgrad_reduce(layers, cache=None):
    """layers: [(scratch, M, N, K, dw, db, accumulate)] of linear_wgrad(dw=None) calls -> all gradients in ONE launch.
    `cache` (a dict owned by the caller): the argument arrays are built once per set of buffers, not per step."""
    if cache is not None and "args" in cache:
        check(lib().vpc_linear_wgrad_reduce(*cache["args"], stream_ptr()), "vpc_linear_wgrad_reduce")
        return
    n = len(layers)
    sc = (C.c_void_p * n)(*[t[0].data_ptr() for t in layers])
    Ms = (C.c_long * n)(*[int(t[1]) for t in layers])
    Ns = (C.c_int * n)(*[int(t[2]) for t in layers])
    Ks = (C.c_int * n)(*[int(t[3]) for t in layers])
    dw = (C.c_void_p * n)(*[t[4].data_ptr() for t in layers])
    db = (C.c_void_p * n)(*[None if t[5] is None else t[5].data_ptr() for t in layers])
    acc = (C.c_int * n)(*[int(bool(t[6])) for t in layers])
    if cache is not None:
        cache["args"] = (n, sc, Ms, Ns, Ks, dw, db, acc)
    check(lib().vpc_linear_wgrad_reduce(n, sc, Ms, Ns, Ks, dw, db, acc, stream_ptr()), "vpc_linear_wgrad_reduce")


# ------------------------------------------------------------------------------------------------ few-row layer ops
def rows_max_rows():
    """The row limit of rows_fwd / rows_bwd (csrc/vpc_rows.hip): 128."""
    return int(lib().vpc_rows_max_rows())


def rows_fwd(x, w, b, y, M, N, K, act=ACT_NONE, split=0, ldx=None, ldy=None):
    """linear_fwd for M <= 128 rows and N, K <= 1024 (fp32): split over output features, one launch."""
    check(lib().vpc_rows_fwd(ptr(x), ldx or K, ptr(w), ptr(b), ptr(y), ldy or N, M, N, K, act, split, stream_ptr()),
          "vpc_rows_fwd")


def rows_bwd(dy, w, x, dx, dw, db, M, N, K, y_gate=None, gate=ACT_NONE, gate_split=0, x_out=None, act_prev=ACT_NONE,
             accumulate=False, lddy=None, ldyg=None, ldx=None, ldxo=None, lddx=None):
    """One layer's whole backward in one launch for M <= 128 rows: dw / db (+)= the weight gradient, written complete (dw None:
    skipped), and dx = the data gradient gated by act_prev'(x_out) (dx None: skipped).  x is the layer's input, x_out the same
    activations where the data gradient is gated with them.  Pitches default as in linear_dgrad / linear_wgrad."""
    check(lib().vpc_rows_bwd(ptr(dy), lddy or N, ptr(y_gate), ldyg or lddy or N, gate, gate_split, ptr(w), ptr(x), ldx or K,
                             ptr(x_out), ldxo or ldx or K, act_prev, ptr(dx), lddx or K, ptr(dw), ptr(db), M, N, K,
                             int(accumulate), stream_ptr()), "vpc_rows_bwd")


# ------------------------------------------------------------------------------------------------ MLP chains
def chain(weights, acts, split=0):
    """[W1, b1, W2, b2, ..] (each W [N, K]) + the activation of every layer -> the chain's layers.  `split`: the column
    split of the LAST layer's activation (ACT_SIGMOID_HARDTANH: Sigmoid below it, Hardtanh from it on)."""
    n = len(acts)
    return [(weights[2 * i], weights[2 * i + 1], weights[2 * i].shape[1], weights[2 * i].shape[0], acts[i],
             split if i == n - 1 else 0) for i in range(n)]


def chain_buffers(layers, M, device, first=None, last=None):
    """Activation (or gradient) buffers of a chain on M rows: [[M, K_0], [M, N_0], [M, N_1], ..], freshly allocated but for
    the ends the caller already holds (`first`: the chain's input, or False where no input gradient is taken; `last`)."""
    out = [torch.empty(M, layers[0][2], device=device) if first is None else first]
    out += [torch.empty(M, l[3], device=device) for l in layers[:-1]]
    return out + [torch.empty(M, layers[-1][3], device=device) if last is None else last]


def chain_fwd(layers, acts, M, precision=0, run=None, names=None):
    """One linear_fwd per layer.  `run(names[i], fn, ...)`: how a trainer issues a launch (its timer bracket); None = call it."""
    for i, (w, b, K, N, act, split) in enumerate(layers):
        if run is None:
            linear_fwd(acts[i], w, b, acts[i + 1], M, N, K, act, split, precision=precision)
        else:
            run(names[i], linear_fwd, acts[i], w, b, acts[i + 1], M, N, K, act, split, precision=precision)


def wgrad_now(key, dy, x, y_gate=None, gate=ACT_NONE, gate_split=0):
    """The weight-gradient sink of the autograd Functions: key = (dw, db, M, N, K), written by this launch."""
    dw, db, M, N, K = key
    linear_wgrad(dy, x, dw, db, M, N, K, y_gate, gate, gate_split)


def wgrad_now_keys(layers, g, names, M):
    """wgrad_now keys of a chain whose gradients are the named views g[W1], g[b1], .. (names = W1, b1, W2, b2, ..)."""
    return [(g[w], g[b], M, l[3], l[2]) for l, w, b in zip(layers, names[0::2], names[1::2])]


def chain_bwd(layers, acts, dacts, M, wgrad, wkeys, input_grad=True, y_gate=None, gate=ACT_NONE, gate_split=0, precision=0,
              run=None, names=None):
    """From the last layer down: weight gradient (`wgrad(wkeys[i], dy, x, gate..)`: written now, or left as partials by a
    trainer), then linear_dgrad gated by the activation of the layer below.  The output gate (y_gate, gate, gate_split)
    applies to the last layer only.  input_grad: False = no dgrad into the chain's input (the encoders), True = an ungated
    dgrad into dacts[0] (z, the point-net aggregate)."""
    for i in range(len(layers) - 1, -1, -1):
        w, _, K, N, _, _ = layers[i]
        dy, x = dacts[i + 1], acts[i]
        wgrad(wkeys[i], dy, x, y_gate, gate, gate_split)
        if i > 0 or input_grad:  # gated by the activation of the layer below; the chain's input has none
            x_out, act_prev = (x, layers[i - 1][4]) if i > 0 else (None, ACT_NONE)
            if run is None:
                linear_dgrad(dy, w, dacts[i], M, N, K, y_gate, gate, gate_split, x_out, act_prev, precision=precision)
            else:
                run(names[i], linear_dgrad, dy, w, dacts[i], M, N, K, y_gate, gate, gate_split, x_out, act_prev,
                    precision=precision)
        y_gate, gate, gate_split = None, ACT_NONE, 0


def chain_fwd_rows(layers, acts, M, run=None, names=None):
    """chain_fwd on the few-row ops: one rows_fwd per layer (M <= rows_max_rows() rows)."""
    for i, (w, b, K, N, act, split) in enumerate(layers):
        if run is None:
            rows_fwd(acts[i], w, b, acts[i + 1], M, N, K, act, split)
        else:
            run(names[i], rows_fwd, acts[i], w, b, acts[i + 1], M, N, K, act, split)


def chain_bwd_rows(layers, acts, dacts, M, grads, input_grad=True, y_gate=None, gate=ACT_NONE, gate_split=0, run=None,
                   names=None):
    """chain_bwd on the few-row ops, from the last layer down: one rows_bwd per layer writes the complete weight gradient
    into grads[i] = (dw, db) - views of the flat gradient - and the data gradient, gated by the activation of the layer
    below, into dacts[i].  The output gate applies to the last layer only; input_grad False: the first layer has no data
    gradient."""
    for i in range(len(layers) - 1, -1, -1):
        w, _, K, N, _, _ = layers[i]
        dw, db = grads[i]
        dx = dacts[i] if (i > 0 or input_grad) else None
        x_out, act_prev = (acts[i], layers[i - 1][4]) if i > 0 else (None, ACT_NONE)
        if run is None:
            rows_bwd(dacts[i + 1], w, acts[i], dx, dw, db, M, N, K, y_gate, gate, gate_split, x_out, act_prev)
        else:
            run(names[i], rows_bwd, dacts[i + 1], w, acts[i], dx, dw, db, M, N, K, y_gate, gate, gate_split, x_out,
                act_prev)
        y_gate, gate, gate_split = None, ACT_NONE, 0
