"""Cases, inputs and float64 references for the narrow point-net front-end (csrc/vpc_eddi.hip: vpc_eddi_fold, vpc_eddi_front_fwd,
vpc_eddi_front_bwd and their tail eddi_reduce_kernel + eddi_param_bwd_kernel).

THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  No GPU is needed to import it: tests/test_eddi_front_cases_cpu.py proves the
cases sound (every instantiation reached, inputs and oracle well inside the bound), tests/test_eddi_front_edges_gpu.py runs the
kernels on them.

The backward kernel is compiled eight times: T = 1 (d <= 64) or 2 features per lane, and KP in {10, 16, 20, 32} register rows of
accumulators, the smallest KP >= K (`variant`).  For K strictly inside a bucket the rows K .. KP - 1 are masked off by `k < K`.
Forward and backward walk the rows in a grid-stride loop: the backward grid has at most 3 x CUs workgroups (12 x CUs waves), the
forward grid twice as many, so only a launch of more than 24 x CUs rows gives a forward wave a second row.

EDGE    every (d, K) of EDGE_D x EDGE_K at B in {1, 5, 37}, one mask and two (stacked passes): both sides of the T boundary
        d = 64 / 65 and of every KP boundary K = 10 / 11, 16 / 17, 20 / 21, the extremes d = 1, 128 and K = 1, 32.
STRIDE  one (d, K) per instantiation at B = 24 CUs + 3 rows (`stride_rows`): with one mask three forward waves take a second row
        and every backward wave takes 2 rows, three of them a third (the one-row-ahead prefetch runs); with two masks the forward
        waves take 2 - 3 rows, the backward waves 4 - 5, and because B is no multiple of the wave count a wave's stride crosses
        from pass 0 (mask) into pass 1 (mask_p, row r - B) in the middle of its loop.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import eddi_mnist_oracle as MO

KPS = (10, 16, 20, 32)
VARIANTS = frozenset((T, KP) for T in (1, 2) for KP in KPS)
AGG_TOL, GRAD_TOL = 1e-5, 2e-5  # the project's bounds for these kernels (header of tests/test_eddi_mnist_gpu.py), of the tensor's max
SOUND = 5.0                     # fp32 torch on the CPU has to stay under 1 / SOUND of them
KINK_CAP = 0.01                 # share of entries that may be taken out of the mask as near-kink
GRAD_KEYS = ("type_pars1", "type_bias1", "pnp_encoder1.0.weight", "pnp_encoder1.0.bias")
GRAD_NAMES = ("gE", "gtb", "gWp", "gcp")  # what the C ABI calls them

EDGE_D = (1, 63, 64, 65, 127, 128)
EDGE_K = (1, 10, 11, 16, 17, 20, 21, 31, 32)
EDGE_B = (1, 5, 37)
EDGE_SHAPES = tuple((d, K) for d in EDGE_D for K in EDGE_K)
# (d, K, B, two, x distribution): x is standard normal in one sub-case per shape (the fold holds for any x), uniform elsewhere
EDGE = tuple((d, K, B, two, "normal" if (B == 5 and two) else "uniform")
             for d, K in EDGE_SHAPES for B in EDGE_B for two in (False, True))
STRIDE = ((40, 10), (64, 16), (64, 20), (33, 32), (100, 7), (65, 11), (128, 20), (128, 32))  # (d, K), one per instantiation
CPU_CUS = 256  # the CU count the CPU test sizes the STRIDE cases with
# Cases whose first seed breaks a condition that tests/test_eddi_front_cases_cpu.py sets on the INPUTS take the next seed,
# base + 10^6 n.  (d, K, B, two): n.  The conditions: near-kink share <= KINK_CAP (at B d < 100 one flagged entry is over the cap),
# and fp32 torch within 1 / SOUND of the bound.  At B = 1 a pass observes one entry, and where its K activations are all tiny the
# tensor's own max is no scale ((65, 20, 1, True): 108 x the bound); at (65, 1, 37, True) the two passes' gWp cancel from 31 and 40 to
# 18, and fp32 torch lands at 0.22 of the bound with one BLAS thread, under 0.2 with four.  With these seeds every EDGE case stays
# under 0.08 of the bound with 1, 4 and 16 threads.
RESEED = {(1, 16, 37, False): 1, (1, 31, 37, False): 1, (65, 1, 37, True): 1, (65, 17, 1, True): 1, (65, 20, 1, False): 1,
          (65, 20, 1, True): 1, (65, 21, 1, True): 1, (127, 11, 1, False): 1, (127, 31, 1, False): 1}


def variant(d, K):
    """(T, KP) of the eddi_front_bwd_kernel<T, KP> that vpc_eddi_front_bwd launches for this shape."""
    if not (0 < d <= 128 and 0 < K <= 32):
        raise ValueError((d, K))
    return (1 if d <= 64 else 2), min(kp for kp in KPS if kp >= K)


def stride_rows(cus):
    return 24 * cus + 3


def bwd_blocks(rows, cus):
    """Workgroups (4 waves each) of the backward launch, eddi_blocks(): one partial block [2][K][d] of the scratch each."""
    return max(1, min((rows + 3) // 4, 3 * cus))


def loop_trips(rows, cus):
    """(fewest, most) rows a wave of the forward and of the backward launch walks: ((f_lo, f_hi), (b_lo, b_hi))."""
    blocks = bwd_blocks(rows, cus)  # the forward launch doubles it
    return tuple((rows // waves, -(-rows // waves)) for waves in (8 * blocks, 4 * blocks))


class Case:
    """Inputs (numpy, fp32 / bool) and float64 references of one case.  ref[p] = (agg [B][K], {key: gradient}) of pass p alone
    (pass 0: mask m and dagg[:B]; pass 1: mask m2 and dagg[B:]); the stacked call gives both agg blocks and the SUM of the
    gradients (`stacked`)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def masks(self):
        return (self.m, self.m2)[:self.npass]

    def stacked(self):
        agg = np.concatenate([r[0] for r in self.ref], 0)
        return agg, {k: sum(r[1][k] for r in self.ref) for k in GRAD_KEYS}


def make(B, d, K, two, seed=None, xdist="uniform"):
    """x, mask, m2 = mask & keep, E, tb, Wp, cp, dagg as tests/test_eddi_mnist_gpu._front_case makes them, with

    - entries within 1e-4 of a ReLU kink (eddi_mnist_oracle.front_near_kink) taken out of the mask: fp32 and float64 may gate
      them differently and the derivative is not defined there (`removed`: their share of all entries),
    - row 0 unobserved, row 1 fully observed (minus near-kink entries), and the last row of each pass observed in column d - 1
      only.  The rules are applied in this order, so at B = 2 row 1 is the last row, and at B = 1 the only row is;
    - the float64 result of eddi_mnist_oracle.front_chunked for each pass."""
    if seed is None:
        seed = 1000 * d + 10 * K + B + int(two) + 1000000 * RESEED.get((d, K, B, two), 0)
    rng = np.random.default_rng(seed)
    if xdist == "normal":
        x = rng.standard_normal((B, d), dtype=np.float32)
    else:
        x = rng.random((B, d), dtype=np.float32)
    m = rng.random((B, d)) < 0.6
    E, tb = rng.normal(size=(d, K)).astype(np.float32), rng.normal(size=(d, 1)).astype(np.float32)
    Wp, cp = rng.normal(size=(K, 2 + K)).astype(np.float32) * 0.3, rng.normal(size=K).astype(np.float32) * 0.3
    kink = MO.front_near_kink(x, E, tb, Wp, cp)
    m[0] = False
    if B > 1:
        m[1] = True
    m[B - 1] = False
    m[B - 1, d - 1] = True
    m &= ~kink
    keep = rng.random((B, d)) < 0.7
    keep[B - 1, d - 1] = True
    m2 = m & keep
    npass = 2 if two else 1
    dagg = rng.normal(size=(npass * B, K)).astype(np.float32)
    ref = [MO.front_chunked(x, mk, E, tb, Wp, cp, dagg[p * B:(p + 1) * B]) for p, mk in enumerate((m, m2)[:npass])]
    return Case(B=B, d=d, K=K, npass=npass, x=x, m=m, m2=m2, E=E, tb=tb, Wp=Wp, cp=cp, dagg=dagg, ref=ref, kink=kink,
                removed=float(kink.mean()), what=f"B={B} d={d} K={K} masks={npass} x={xdist}")


@functools.lru_cache(maxsize=None)
def edge_case(d, K, B, two, xdist):
    return make(B, d, K, two, xdist=xdist)


@functools.lru_cache(maxsize=None)
def stride_case(d, K, cus):
    """Both passes; the one-mask launch of a STRIDE shape is pass 0 of the same inputs, so one oracle run serves both."""
    return make(stride_rows(cus), d, K, True)


def fold_ref(c):
    """float64 AC [2][K][d] and the magnitude sums S of its dot products: |w_x| + sum_e |W_E[k][e] E[j][e]| and |w_t t_j| + |c_k|.
    A recursive fp32 sum of n products is within n 2^-24 / (1 - n 2^-24) of S from the exact value."""
    E, tb, Wp, cp = (t.astype(np.float64) for t in (c.E, c.tb, c.Wp, c.cp))
    K = c.K
    wx, WE, wt = Wp[:, 0], Wp[:, 1:1 + K], Wp[:, 1 + K]
    A = wx[:, None] + WE @ E.T
    C = wt[:, None] * tb[:, 0][None, :] + cp[:, None]
    SA = np.abs(wx)[:, None] + np.abs(WE) @ np.abs(E).T
    SC = np.abs(wt)[:, None] * np.abs(tb[:, 0])[None, :] + np.abs(cp)[:, None]
    return np.stack([A, C]), np.stack([SA, SC])


def _tree_sum(ts):
    """Pairwise fp32 sum of a list of tensors: the error grows with log2(len), not with len."""
    ts = list(ts)
    while len(ts) > 1:
        ts = [ts[i] + ts[i + 1] if i + 1 < len(ts) else ts[i] for i in range(0, len(ts), 2)]
    return ts[0]


def torch32(c, rows=16):
    """The same expression as the reference writes it (VAE.py:719-733: Linear(2 + K -> K) on the unfolded [B d][2 + K] tensor,
    ReLU, mask-weighted sum), in fp32 torch on the CPU with autograd, per pass: [(agg, {key: gradient})].  It only shows that
    fp32 arithmetic on these inputs reaches the bound; nothing is compared against it on the GPU.

    The sums over the batch are BLOCKED, as the bound's sqrt(n) 2^-24 argument assumes of the kernels: autograd runs on chunks of
    `rows` rows and the chunks' gradients are added pairwise.  Left to one GEMM over all B d rows the order of the sum is the
    BLAS's, and one that accumulates 393 216 terms one after the other (seen on one host: 5.1e-6 of max in gWp at B = 6147,
    d = 64) says nothing about the inputs.  In a chunk at most 16 x 128 terms are summed in whatever order, about
    sqrt(2048 / 2) 2^-24 = 1.9e-6 even one after the other."""
    p = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (c.E, c.tb, c.Wp, c.cp)]
    E, tb, Wp, cp = p
    x, dagg = torch.from_numpy(c.x), torch.from_numpy(c.dagg)
    out = []
    for ps, mk in enumerate(c.masks()):
        mk = torch.from_numpy(mk)
        aggs, grads = [], []
        for lo in range(0, c.B, rows):
            xs = x[lo:lo + rows]
            n = xs.shape[0]
            xf = xs.reshape(-1, 1)
            feat = torch.cat([xf, xf * E.repeat(n, 1), tb.repeat(n, 1)], 1)
            h = torch.relu(torch.nn.functional.linear(feat, Wp, cp))
            agg = (mk[lo:lo + rows].reshape(n, c.d, 1).float() * h.reshape(n, c.d, c.K)).sum(1)
            grads.append(torch.autograd.grad(agg, p, dagg[ps * c.B + lo:ps * c.B + lo + n]))
            aggs.append(agg.detach())
        out.append((torch.cat(aggs, 0).numpy(), {k: _tree_sum(g[i] for g in grads).numpy() for i, k in enumerate(GRAD_KEYS)}))
    return out


def stacked32(per_pass):
    """torch32's passes as the stacked call returns them: agg blocks one after the other, gradients added in fp32."""
    agg = np.concatenate([r[0] for r in per_pass], 0)
    return agg, {k: functools.reduce(np.add, [r[1][k] for r in per_pass]) for k in GRAD_KEYS}


def rel_err(got, ref):
    """max |got - ref| relative to the reference tensor's OWN maximum - no floor of 1, so a tensor of small values is held as
    tightly as a large one.  A reference that is all zero admits exact zeros only: the error is then 0 or inf."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(got - ref)))
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale
