"""Cases of the streaming MIWAE imputation (csrc/vpc_miw_impute.hip), shared by tests/test_miwae_stream_gpu.py (GPU) and
tests/test_miwae_stream_cases.py (CPU): whole-model cases of tests/miwae_cases.model_case with planted rows, and the
float64 reference of a case (tests/miwae_oracle.py, per-row pairing, injected draws).

The kernel gives a workgroup one data row and one chunk of its samples, tiles the chunk by 16 samples, holds d <= 32 and
L <= 16 as one or two 16-column tiles and is instantiated per <YT, LT> = (tiles of the 3 d decoder heads, tiles of the 2 L
encoder heads).  SHAPES are the smallest shapes at which each of these can break; INSTANCE_SHAPES add one small case per
instantiation the shapes above do not reach, at the widest d and L of the instantiation.

Planted rows (stream_case): row 0 fully observed; row 1 (B >= 2) with nothing observed, where the weights reduce to
softmax(log p(z') - log q(z')); row 2 (the SPAN_SHAPES) with one observed column far from the decoder's mean and
that column's df head made to swing from sample to sample, so that the row's log-weights span more than SPAN_NATS: the row
on which a missing rescale of the online softmax would show."""
import functools
import os
import re

import numpy as np
import torch

import miwae_cases as C
import miwae_oracle as O

SEED = 0
SHAPES = [                 # (B, S, d, L)
    (1, 9, 12, 10),        # the eval shape of miwae_cases.py
    (5, 700, 12, 10),      # the existing large-S case
    (3, 1, 12, 10),        # S = 1: every weight is exactly 1
    (2, 17, 17, 10),       # ragged tile, DT = 2
    (2, 33, 32, 16),       # the largest instantiation
    (2, 20, 1, 1),         # the smallest
    (300, 3, 12, 10),      # more workgroups than compute units
]
_YT_D = {1: 5, 2: 10, 3: 16, 4: 21, 5: 26, 6: 32}   # the widest d of each YT
_LT_L = {1: 8, 2: 9}                                 # 2 L = 16 exactly, and one past it
CHUNK_SHAPE = (5, 700, 12, 10)
CHUNKS = {16: 44, 48: 15, 112: 7, 700: 1, 10000: 1}  # s_chunk -> chunks per row at S = 700
# The span row needs many samples: at S = 3 a 100-nat span takes a planted value that also drives the encoder (x * mask is its
# input) to log-weights of thousands of nats, whose fp32 rounding alone exceeds the bound on xm.  At S = 700 a column at 30
# (data are in [0, 1]) with a 200-fold df head spans 110 - 120 nats at log-weights below 150, with several samples sharing the
# weight (tests/test_miwae_stream_cases.py asserts both).
SPAN_SHAPES = [(5, 700, 12, 10)]
SPAN_NATS = 100.0
SPAN_COLUMN, SPAN_X, SPAN_GAIN = 0, 30.0, 200.0


def instance(d, L):
    """<YT, LT> of a shape, as miw_impute_pick of csrc/vpc_miw_impute.hip picks it."""
    return (3 * d + 15) // 16, 1 if 2 * L <= 16 else 2


_reached = {instance(s[2], s[3]) for s in SHAPES}
INSTANCE_SHAPES = [(2, 17, _YT_D[yt], _LT_L[lt]) for yt in _YT_D for lt in _LT_L if (yt, lt) not in _reached]
ALL_SHAPES = SHAPES + INSTANCE_SHAPES


def built_instances():
    """The <YT, LT> instantiations csrc/vpc_miw_impute.hip lists: the YT cases of miw_impute_pick_y times the LT values
    miw_impute_pick passes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "vae-posterior-consistency_amd", "csrc", "vpc_miw_impute.hip")).read()
    yts = {int(v) for v in re.findall(r"return miw_impute_kernel<(\d+), LT>;", src)}
    lts = {int(v) for v in re.findall(r"miw_impute_pick_y<(\d+)>\(yt\)", src)}
    return {(yt, lt) for yt in yts for lt in lts}


@functools.lru_cache(maxsize=None)
def stream_case(shape, kind):
    """model_case(*shape, seed 0) with the planted rows; the cached arrays of model_case stay as they are."""
    c = dict(C.model_case(*shape, kind == "reg", SEED))
    B, S, d, Ld = shape
    x, m = c["x"].copy(), c["mask"].copy()
    mp = None if c["mask_p"] is None else c["mask_p"].copy()
    m[0] = 1.0
    if B >= 2:
        m[1] = 0.0
        if mp is not None:
            mp[1] = 0.0
    if shape in SPAN_SHAPES:
        k = SPAN_COLUMN
        m[2, k] = 1.0
        x[2, k] = SPAN_X
        p = dict(c["params"])
        w, b = p["seq_decoder.4.weight"].copy(), p["seq_decoder.4.bias"].copy()
        w[2 * d + k] *= SPAN_GAIN  # the raw df head of the column: df swings between 3 and tens from sample to sample
        b[2 * d + k] *= SPAN_GAIN
        p["seq_decoder.4.weight"], p["seq_decoder.4.bias"] = w, b
        c["params"] = p
    c.update(x=x, mask=m, mask_p=mp)
    return c


def other_mask_p(c):
    """A second mask_p of a Reg case: the observed entries the case's own mask_p leaves out, so the two differ wherever
    mask is 1 (the imputation must not depend on which one is used)."""
    return (c["mask"] * (1.0 - c["mask_p"])).astype(np.float32)


def stream_eps(c):
    """The kernel's draws of a case, [2, B, S, L]: the q pass's sampler draw and the q pass's fresh draw."""
    P = 2 if c["reg"] else 1
    return np.stack([c["eps"][0], c["eps"][P]])


@functools.lru_cache(maxsize=None)
def reference(shape, kind, second_mask_p=False):
    """float64: (xm [B, d], per-row log-sum-exp of the log-weights [B], the oracle's loss, log-weights a_q [S, B])."""
    c = stream_case(shape, kind)
    p, x, m, mp, eps = C.oracle_inputs(c)
    if second_mask_p:
        mp = torch.from_numpy(other_mask_p(c))
    with torch.no_grad():
        lo, a_q, q, _ = O.run(p, x, m, mp, eps, 0.5, "per_row")
        return O.impute(a_q, q[0][0]), torch.logsumexp(a_q, 0), lo, a_q
