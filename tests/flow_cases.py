"""Inputs and float64 / fp32-torch references of the flow-kernel parity cases shared by tests/test_flow_kernels_gpu.py
(GPU) and tests/test_flow_oracle.py (CPU), from seeded numpy generators, so that a case is the same arrays on every
machine.

vpc_flow_fwd / vpc_flow_bwd run one thread per (row, latent), 256 threads = 25.6 rows per workgroup, and every workgroup
works out which of the P <= 2 passes of B rows it touches and scans those passes for an inside draw in 256-element
chunks.  The shapes (B, P) put the pass boundary inside a block's last row (25: block 0 ends in row 25, the first of the
p pass; 51: the same for block 1, the first block whose 26 rows differ from 25 + 1), inside a block (26, 37), on a block
boundary (128) and give eleven chunks with a partial last one (257).
"""
import functools
import itertools

import numpy as np
import torch

import flow_oracle as FO

L = FO.L
FLOW_SHAPES = [(1, 1), (1, 2), (25, 2), (26, 2), (37, 2), (51, 2), (128, 1), (128, 2), (257, 1), (257, 2)]
NARROW, WIDE = (0.5, 1.0), 8.0
SIGMAS = [*NARROW, WIDE]   # std of the logits; nothing in between (2 -> 3 %, 3 -> 16 % flagged: neither capped nor wide)
ALL = ("dz", "dz2", "dzlp")
GIVEN = [ALL, ("dz",), ("dz2",), ("dzlp",), ("dz", "dzlp"), ()]


def _seed(*k):
    return [int(abs(v) * 1000) for v in k]


@functools.lru_cache(maxsize=None)
def flow_inputs(B, P, sigma):
    """t [R, 100] N(0, sigma^2), eps [R, 10] N(0, 1) (about 68 % inside) and the three upstream gradients, fp32."""
    rng = np.random.default_rng(_seed(B, P, sigma))
    R = B * P
    n = lambda *s: rng.normal(size=s).astype(np.float32)
    return dict(t=(sigma * rng.normal(size=(R, L * L))).astype(np.float32), eps=n(R, L), dz=n(R, L), dz2=n(R, L),
                dzlp=n(R, L))


# ---- inside-flag placement at B = 257 (2570 draws per pass: ten full chunks and one of 10).  (pass, idx): that pass has
# its only inside draw at flat element idx, the other pass has none; (pass, None): that pass has N(0, 1) draws, the other
# pass none
PLACE_B = 257
PLACE_IDX = (0, 255, 256, 2559, 2560, 2569)
PLACEMENTS = [(ps, i) for ps in "qp" for i in PLACE_IDX] + [("q", None), ("p", None)]


@functools.lru_cache(maxsize=None)
def placement_inputs(ps, idx):
    B = PLACE_B
    rng = np.random.default_rng(_seed(ord(ps), -1 if idx is None else idx))
    inp = {k: v.copy() for k, v in flow_inputs(B, 2, 1.0).items()}
    eps = (rng.choice([-1.0, 1.0], size=(2, B * L)) * (1.25 + rng.random((2, B * L)))).astype(np.float32)
    k = "qp".index(ps)
    if idx is None:
        eps[k] = rng.normal(size=B * L).astype(np.float32)
    else:
        eps[k, idx] = np.float32(rng.uniform(-1, 1))
    inp["eps"] = eps.reshape(2 * B, L)
    return inp


def planted_values():
    """The knots -1 + 0.2 k in fp32 with both fp32 neighbours (at +-1 these are the inside / outside threshold +- 1 ulp),
    +-0.0 and 5.0."""
    v = []
    for k in range(11):
        x = np.float32(-1 + 0.2 * k)
        v += [x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))]
    return np.array(v + [0.0, -0.0, 5.0], np.float32)


PLANT_B = 4


@functools.lru_cache(maxsize=None)
def planted_inputs(sigma):
    inp = {k: v.copy() for k, v in flow_inputs(PLANT_B, 1, sigma).items()}
    v = planted_values()
    inp["eps"].reshape(-1)[:v.size] = np.random.default_rng(3).permutation(v)
    return inp


UNDER_B = 37


@functools.lru_cache(maxsize=None)
def underflow_inputs():
    """Logits of spread 120: of a latent's ten, 1, 2, 4 or 8 among the columns the row's mask keeps are +60, the rest
    -60, so that exp(-120) = 0 exactly in fp32.  Every pdf entry is then 0, 2^-k or (a masked column) 2^-k e^-60, every
    cdf entry a multiple of 1 / 8, whatever the order of the sums: the decisions of layers 2 and 3, many of them at
    exact knots, come out the same in any correct fp32 evaluation."""
    inp = {k: v.copy() for k, v in flow_inputs(UNDER_B, 2, 1.0).items()}
    rng = np.random.default_rng(120)
    eps = inp["eps"]
    eps[~(np.abs(eps) <= 1).any(1), 0] = 0.5
    t = np.full((2 * UNDER_B, L, L), -60.0, np.float32)
    for r, i in itertools.product(range(2 * UNDER_B), range(L)):
        cols = np.flatnonzero(np.abs(eps[r]) <= 1)
        n = rng.choice([k for k in (1, 2, 4, 8) if k <= cols.size])
        t[r, i, rng.permutation(cols)[:n]] = 60.0
    inp["t"] = t.reshape(2 * UNDER_B, L * L)
    return inp


# ------------------------------------------------------------------------------------------------ references
def _passes(B, P):
    return [slice(p * B, (p + 1) * B) for p in range(P)]


def torch_flow(t, eps, dzs, dzlp, B, P, decisions=None):
    """The P passes through FO._torch_flow in the dtype of t, with autograd for d / d t: (z, z_log_prob, dt)."""
    tt = t.clone().requires_grad_()
    out = [FO._torch_flow(tt[sl], eps[sl], None if decisions is None else decisions[p])
           for p, sl in enumerate(_passes(B, P))]
    z, zlp = torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])
    s = (z * dzs).sum() + (zlp * dzlp).sum()
    dt = torch.autograd.grad(s, tt)[0] if s.requires_grad else torch.zeros_like(tt)
    return z.detach(), zlp.detach(), dt


def reference(inp, B, P, given=ALL):
    """float64 (FO.flow_fwd / flow_bwd, closed form) and fp32 torch forced onto the float64 run's decisions, for the
    upstream gradients named in `given` (the others are absent = 0); the flags of every element."""
    R = B * P
    t, eps = inp["t"].astype(np.float64), inp["eps"].astype(np.float64)
    g64 = lambda k: inp[k].astype(np.float64) if k in given else np.zeros((R, L))
    g32 = lambda k: torch.from_numpy(inp[k]) if k in given else torch.zeros(R, L)
    dzs, dzlp = g64("dz") + g64("dz2"), g64("dzlp")
    fwd = [FO.flow_fwd(t[sl], eps[sl]) for sl in _passes(B, P)]
    caches = [f[2] for f in fwd]
    dt = np.concatenate([FO.flow_bwd(c, dzs[sl], dzlp[sl]) for c, sl in zip(caches, _passes(B, P))])
    flags = [None if c is None else FO.flow_flags(c) for c in caches]
    fl = np.concatenate([np.zeros((B, L), bool) if f is None else FO.flagged(f) for f in flags])
    z32, zlp32, dt32 = torch_flow(torch.from_numpy(inp["t"]), torch.from_numpy(inp["eps"]), g32("dz") + g32("dz2"),
                                  g32("dzlp"), B, P, [None if c is None else c[4] for c in caches])
    return dict(z64=np.concatenate([f[0] for f in fwd]), zlp64=np.concatenate([f[1] for f in fwd]), dt64=dt,
                z32=z32.numpy(), zlp32=zlp32.numpy(), dt32=dt32.numpy(), flagged=fl, caches=caches, flags=flags,
                dzs=dzs, dzlp=dzlp, t=t, eps=eps, splined=np.concatenate([np.full((B, L), c is not None) for c in caches]),
                inside=np.abs(inp["eps"]) <= 1)


def alternative_reference(ref, B, P, c):
    """float64 (z_log_prob, dt) with the flagged decisions switched as bit pattern c says (FO.alternative)."""
    zlp, dt = [], []
    for p, sl in enumerate(_passes(B, P)):
        cache = ref["caches"][p]
        if cache is None:
            zlp.append(ref["zlp64"][sl])
            dt.append(ref["dt64"][sl])
            continue
        _, l, ca = FO.flow_fwd(ref["t"][sl], ref["eps"][sl], FO.alternative(cache, ref["flags"][p], c))
        zlp.append(l)
        dt.append(FO.flow_bwd(ca, ref["dzs"][sl], ref["dzlp"][sl]))
    return np.concatenate(zlp), np.concatenate(dt)


@functools.lru_cache(maxsize=None)
def grid_reference(B, P, sigma):
    return reference(flow_inputs(B, P, sigma), B, P)


def flag_counts(ref):
    """(flagged splined elements, unflagged inside elements, inside elements of the passes that run the spline)."""
    ins = ref["inside"] & ref["splined"]
    return int(ref["flagged"].sum()), int((ins & ~ref["flagged"]).sum()), int(ins.sum())


# ------------------------------------------------------------------------------------------------ vpc_flow_loss
# one wave per row (d in 64-lane trips: below, at, one past, two trips, four), 4 rows per workgroup (B below, at and off
# a multiple of 4), one partial block per workgroup summed by 32 lanes (B = 129: 33 blocks, B = 300: 75, the strided trip)
LOSS_D = (1, 9, 63, 64, 65, 128, 200)
LOSS_B = (1, 3, 4, 5, 129, 300)
KINDS = ("reg", "reg_eval", "van")
ALPHAS, BETAS = (0.0, 0.5, 1.0), (1.0, 0.25)


def _loss_cases():
    """The full cross of d, B and kind; alpha, beta and gated cycle so that every value meets every kind."""
    out = []
    for (di, d), (bi, B) in itertools.product(enumerate(LOSS_D), enumerate(LOSS_B)):
        for k, kind in enumerate(KINDS):
            out.append(dict(d=d, B=B, kind=kind, alpha=ALPHAS[(di + bi + k) % 3], beta=BETAS[(di + bi // 2 + k) % 2],
                            gated=(di + bi + k) % 2))
    return out


LOSS_CASES = _loss_cases()
LOSS_SHAPES = list(itertools.product(LOSS_D, LOSS_B))
PITCH_SHAPES = [(1, 1), (9, 5), (65, 5), (200, 129)]   # (d, B)
MASK_CASES = ("all_observed", "none_observed", "mask_p_is_mask", "mask_p_zero")


@functools.lru_cache(maxsize=None)
def loss_inputs(B, d, masks=None):
    """x, mask, mask_p [B, d]; x_mean (q, p) uniform on (0.02, 0.98) with an exact 0 in the first and an exact 1 in the
    last element (both observed in mask and mask_p: the gated gradient is 0 there); z, z_log_prob (q, p) [B, 10] = the
    float64 oracle's forward on sigma = 1 logits, rounded to fp32, with every seventh z_log_prob_p set to z_log_prob_q
    bitwise (`ties`)."""
    rng = np.random.default_rng(_seed(B, d, 77))
    x = rng.random((B, d)).astype(np.float32)
    m = (rng.random((B, d)) < 0.7).astype(np.float32)
    mp = m * (rng.random((B, d)) < 0.5).astype(np.float32)
    xm = [rng.uniform(0.02, 0.98, size=(B, d)).astype(np.float32) for _ in range(2)]
    for a in (m, mp):
        a.flat[0] = a.flat[-1] = 1.0
    xm[0].flat[-1], xm[1].flat[0] = 1.0, 0.0
    xm[0].flat[0], xm[1].flat[-1] = 0.0, 1.0   # B * d = 1: q holds the 0, p the 1
    if masks == "all_observed":
        m[:] = 1.0
    elif masks == "none_observed":
        m[:] = 0.0
        mp[:] = 0.0
    elif masks == "mask_p_is_mask":
        mp = m.copy()
    elif masks == "mask_p_zero":
        mp[:] = 0.0
    t, eps = rng.normal(size=(2 * B, L * L)), rng.normal(size=(2 * B, L))
    fwd = [FO.flow_fwd(t[sl], eps[sl]) for sl in _passes(B, 2)]
    z = [f[0].astype(np.float32) for f in fwd]
    zlp = [f[1].astype(np.float32) for f in fwd]
    ties = np.zeros(B * L, bool)
    ties[::7] = True
    ties = ties.reshape(B, L)
    zlp[1][ties] = zlp[0][ties]
    return dict(x=x, m=m, mp=mp, xm=xm, z=z, zlp=zlp, ties=ties)


def loss_reference(inp, kind, alpha, beta, gated, gscale, dtype):
    c = lambda a: torch.from_numpy(a).to(dtype)
    return FO.loss_terms(c(inp["x"]), c(inp["m"]), None if kind == "van" else c(inp["mp"]), [c(a) for a in inp["xm"]],
                         [c(a) for a in inp["z"]], [c(a) for a in inp["zlp"]], alpha, beta,
                         "evaluate" if kind == "reg_eval" else "train", gated, gscale)


# ------------------------------------------------------------------------------------------------ vpc_flow_prep
PREP_SHAPES = [(1, 1), (3, 9), (5, 13), (64, 12), (37, 128)]   # (B, d): B * d = 1, 27, 65 are no multiple of 4
PREP_MODES = ("vanilla", "mask_p_in", "mask_p_in_out", "mask_p_out")


@functools.lru_cache(maxsize=None)
def prep_inputs(B, d):
    rng = np.random.default_rng(_seed(B, d, 5))
    x = rng.random((B, d)).astype(np.float32)
    m = (rng.random((B, d)) < 0.7).astype(np.float32)
    mp = m * (rng.random((B, d)) < 0.5).astype(np.float32)
    return dict(x=x, m=m, mp=mp)
