"""Cases of the streaming MNAR imputation (csrc/vpc_nm_impute.hip), shared by tests/test_nm_stream_gpu.py (GPU) and
tests/test_nm_stream_cases.py (CPU): whole-model cases with planted rows, and the float64 reference of a case
(oracle.notmiwae_oracle.NMTorchPort on float64 parameters, injected draws).

The kernel gives a workgroup one data row and one chunk of its samples, tiles the chunk by 16 samples, splits the out
tiles of the 2 d decoder heads (xm | xl) over 8 waves and is instantiated per <HT, LT, REG> = (head tiles per wave: 1 up
to 2 d = 128, else 2; tiles of the 2 L encoder heads: 1 up to 2 L = 16, else 2; the model class).  SHAPES are the smallest
shapes at which each of these can break; INSTANCE_SHAPES add one small case per <HT, LT> the shapes above do not reach, at
the widest d and L of the instantiation; every shape runs for both classes.

Planted rows (stream_case): row 0 fully observed; row 1 (B >= 2) with nothing observed, where the weights come from
log p(s | x) of the decoder's own means (plus the fresh-draw term for the un-regularised class); row 2 of SPAN_SHAPE with
column 0 observed at SPAN_X, far outside the data's [0, 1], and that column's x_logvar head made SPAN_GAIN times as steep,
so that the row's log-weights span more than SPAN_NATS; the row's samples are then put into ascending order of the float64
log-weight (both draw planes together): every sample raises the running max, so a missing or wrong rescale of the online
softmax is gross there, not marginal."""
import functools
import os
import re

import numpy as np
import torch

from oracle import notmiwae_oracle as O

SEED = 0
SHAPES = [                 # (B, S, d, L)
    (1, 9, 14, 10),        # one row
    (3, 1, 12, 10),        # S = 1: every weight is exactly 1, xm = that sample's sigmoid
    (2, 17, 17, 10),       # ragged sample tile; the xm | xl boundary falls inside an out tile
    (2, 17, 64, 8),        # the last shape with one head tile per wave and 2 L = 16
    (2, 17, 65, 9),        # the first shape past both
    (2, 33, 128, 16),      # the largest
    (2, 20, 1, 1),         # the smallest
    (300, 3, 12, 10),      # more workgroups than compute units
    (5, 700, 12, 10),      # chunking and the span row
]
_HT_D = {1: 64, 2: 128}    # the widest d of each HT
_LT_L = {1: 8, 2: 16}      # the widest L of each LT
CHUNK_SHAPE = SPAN_SHAPE = (5, 700, 12, 10)
CHUNKS = {16: 44, 48: 15, 112: 7, 700: 1, 10000: 1}  # s_chunk -> chunks per row at S = 700
SPAN_NATS, SPAN_MAX_ABS = 100.0, 400.0
SPAN_ROW, SPAN_COLUMN, SPAN_X, SPAN_GAIN = 2, 0, 6.0, 8.0
KINDS = ("reg", "van")


def instance(d, L):
    """<HT, LT> of a shape, as nm_impute_pick of csrc/vpc_nm_impute.hip picks it."""
    return 1 if 2 * d <= 128 else 2, 1 if 2 * L <= 16 else 2


_reached = {instance(s[2], s[3]) for s in SHAPES}
INSTANCE_SHAPES = [(2, 17, _HT_D[ht], _LT_L[lt]) for ht in _HT_D for lt in _LT_L if (ht, lt) not in _reached]
ALL_SHAPES = SHAPES + INSTANCE_SHAPES


def built_instances():
    """The <HT, LT, REG> instantiations nm_impute_pick of csrc/vpc_nm_impute.hip lists."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "vae-posterior-consistency_amd", "csrc", "vpc_nm_impute.hip")).read()
    pick = src[src.index("NmImputeKernel nm_impute_pick("):]
    pick = pick[:pick.index("\n}\n")]
    return {(int(h), int(l), r == "true") for h, l, r in re.findall(r"return nm_impute_kernel<(\d+), (\d+), (true|false)>;", pick)}


def log_weights(port, x, mask, eps):
    """a [B, S] = -l_w of the q pass (VAE.py:2398-2435 / :2774-2802) and the decoder's means [B, S, d], in the dtype of the
    port's parameters: the terms of NMTorchPort.reg_loss / van_loss, whose llh_eval branch returns softmax(a) . x_mean."""
    z, mean, logvar = port.encoder(x, mask, eps[0])
    xm, xl = port.decoder(z)
    x3, m3 = (t.unsqueeze(1).expand(-1, port.K, -1) for t in (x, mask))
    RE = port._nll(x3 * m3, xm * m3, xl * m3)
    if port.reg:
        KL = torch.sum(0.5 * (torch.exp(logvar) + mean ** 2 - 1 - logvar), 2)
    else:
        sd = torch.exp(logvar / 2)
        zf = mean + eps[1] * sd
        KL = torch.sum(-0.5 * ((zf - mean) / sd) ** 2 - torch.log(sd) - O.HALF_LOG_2PI, 2) - \
            torch.sum(-0.5 * zf ** 2 - O.HALF_LOG_2PI, 2)
    return -(RE + KL - port._logp_s(x3, m3, xm)), xm


def _port(c, dtype):
    return O.NMTorchPort({k: torch.from_numpy(v).to(dtype) for k, v in c["params"].items()}, c["L"], c["S"], c["reg"])


@functools.lru_cache(maxsize=None)
def stream_case(shape, kind):
    """dict(params (fp32 numpy, keys O.NM_KEYS), x, mask, mask_p (reg), eps [2, B, S, L] (a | b), eps_p [B, S, L]) with the
    planted rows.  Treat the arrays as read-only."""
    B, S, d, Ld = shape
    g = torch.Generator().manual_seed(1000 * SEED + 7 * B + 3 * S + d + 31 * Ld)
    params = {k: v.numpy().copy() for k, v in O.nm_init_params(d, Ld, SEED).items()}
    x = torch.rand(B, d, generator=g).numpy()
    m = (torch.rand(B, d, generator=g) < 0.7).float().numpy()
    eps = torch.randn(2, B, S, Ld, generator=g).numpy()
    eps_p = torch.randn(B, S, Ld, generator=g).numpy()
    keep = (torch.rand(B, d, generator=g) < 0.5).float().numpy()
    m[0] = 1.0
    if B >= 2:
        m[1] = 0.0
    c = dict(reg=kind == "reg", B=B, S=S, d=d, L=Ld, params=params, x=x, mask=m, eps=eps, eps_p=eps_p)
    if shape == SPAN_SHAPE:
        k, r = SPAN_COLUMN, SPAN_ROW
        m[r, k] = 1.0
        x[r, k] = SPAN_X
        params["x_logvar.0.weight"][k] *= SPAN_GAIN
        params["x_logvar.0.bias"][k] *= SPAN_GAIN
        with torch.no_grad():
            a, _ = log_weights(_port(c, torch.float64), torch.from_numpy(x[r:r + 1]).double(),
                               torch.from_numpy(m[r:r + 1]).double(), torch.from_numpy(eps[:, r:r + 1]).double())
        order = torch.argsort(a[0]).numpy()
        eps[:, r] = eps[:, r][:, order]
    c["mask_p"] = m * keep if c["reg"] else None
    return c


def other_mask_p(c):
    """A second mask_p of a Reg case: the observed entries the case's own mask_p leaves out, so the two differ wherever
    mask is 1 (the imputation must not depend on which one is used)."""
    return (c["mask"] * (1.0 - c["mask_p"])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, dtype=torch.float64, second_mask_p=False):
    """(xm [B, d] of the port's llh_eval branch, lse [B] = logsumexp of the log-weights, the log-weights a [B, S], the
    decoder's means [B, S, d]) in `dtype`."""
    c = stream_case(shape, kind)
    port = _port(c, dtype)
    t = lambda a: torch.from_numpy(a).to(dtype)
    x, m, eps = t(c["x"]), t(c["mask"]), t(c["eps"])
    with torch.no_grad():
        if c["reg"]:
            mp = t(other_mask_p(c) if second_mask_p else c["mask_p"])
            xm = port.reg_loss(x, port.reg_forward(x, m, mp, eps[0], t(c["eps_p"])), m, mp, alpha=0.5, llh_eval=True)[0]
        else:
            xm = port.van_loss(x, port.van_forward(x, m, eps[0]), m, eps[1], llh_eval=True)[0]
        a, xmean = log_weights(port, x, m, eps)
    return xm, torch.logsumexp(a, 1), a, xmean
