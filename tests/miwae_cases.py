"""Inputs of the MIWAE parity cases shared by tests/test_miwae_gpu.py, tests/test_miwae_kernels_gpu.py (GPU) and
tests/test_miwae_oracle.py (CPU): random loss-kernel inputs in two head distributions, the inputs of the elementwise
kernels with the softplus threshold planted, and whole-model cases (parameters, data, masks, every draw) from a seeded
numpy generator, so that a case is the same arrays on every machine.

Loss-kernel shapes (B, S, d, L).  The row / slot kernels run one wave (64 lanes) per row or slot and MIW_WAVES = 4 waves
per workgroup, so the edges are 64 and one past it in S, d and L, B below and off a multiple of 4, and the family's
limits d = 256, L = 64.
"""
import functools

import numpy as np
import torch

import miwae_oracle as O

HID = 128  # the reference's hard-coded hidden width (VAE.py:3027-3042)

LOSS_GRID = [
    (1, 1, 1, 1),      # all-ones degenerate case
    (1, 9, 12, 10),    # the eval_miwae shape
    (3, 5, 12, 4),     # B < MIW_WAVES
    (5, 64, 14, 10),   # S at one wave
    (6, 65, 14, 10),   # S one past a wave
    (4, 130, 3, 2),    # three trips over S
    (33, 7, 64, 5),    # d at one wave
    (9, 3, 65, 64),    # d one past a wave, L at the limit
    (7, 2, 256, 64),   # d and L at their limits
]
PITCH_CASES = [(3, 5, 12, 4), (6, 65, 14, 10), (9, 3, 65, 64)]
SAMPLE_SHAPES = [(1, 1, 1), (3, 7, 10), (37, 65, 64), (5, 130, 3)]   # (R, S, L): 1, 210, 153 920, 1 950 elements of z
HEADS_SHAPES = [(1, 1), (37, 70), (259, 256), (5, 3)]                # (M, d): 1, 2 590, 66 304 (= 259 * 256), 15 threads


def rand_inputs(B, S, d, Ld, seed, dist="narrow"):
    """x, mask, mask_p [B, d] and per pass (raw decoder heads [B*S, 3d], encoder mean [B, L], encoder scale [B, L]), then
    the loss-time draws [2, B, S, L].  narrow: every raw head N(0, 1) (df in about [3, 8]).  wide: raw mean and scale
    heads N(0, 4^2), raw df head N(0, 16^2) (df from 3 to about 70: both regimes of the kernel's digamma and both sides
    of the softplus threshold), encoder scale uniform on [0.05, 3]; raw values are clipped to [-75, 75] so that exp() of
    them is a normal fp32 number."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, d)).astype(np.float32)
    m = (rng.random((B, d)) < 0.7).astype(np.float32)
    mp = m * (rng.random((B, d)) < 0.5).astype(np.float32)
    if dist == "narrow":
        mk = lambda: (rng.normal(size=(B * S, 3 * d)).astype(np.float32), rng.normal(size=(B, Ld)).astype(np.float32),
                      (0.2 + rng.random((B, Ld))).astype(np.float32))
    else:
        def mk():
            y = rng.normal(size=(B * S, 3 * d)) * np.repeat([4.0, 4.0, 16.0], d)[None, :]
            return (np.clip(y, -75, 75).astype(np.float32), rng.normal(size=(B, Ld)).astype(np.float32),
                    (0.05 + 2.95 * rng.random((B, Ld))).astype(np.float32))
    e = rng.normal(size=(2, B, S, Ld)).astype(np.float32)
    return x, m, mp, mk(), mk(), e


def raw_to_act(Y, d):
    t = torch.from_numpy(Y).double()
    return (torch.sigmoid(t[:, :d]), torch.nn.functional.softplus(t[:, d:2 * d]) + 0.001,
            torch.nn.functional.softplus(t[:, 2 * d:]) + 3)


def act_f32(Y, d):
    """The activated heads the raw = 0 runs are given: float64 activations of the raw draws, rounded to fp32 [N, 3d]."""
    return torch.cat(raw_to_act(Y, d), 1).float().numpy()


def plant_threshold(a):
    """In place on a raw block [rows, W]: column 0 cycles over 20, the next float above and the next float below down its
    rows (the kernels branch on v > 20), and row 0 carries the same three across its first columns, so that a block of
    fewer than three rows still holds as many of them as it has room for."""
    t = np.float32(20.0)
    vals = [t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))]
    for c in range(min(3, a.shape[1])):
        a[0, c] = vals[c]
    for r in range(a.shape[0]):
        a[r, 0] = vals[r % 3]
    return a


@functools.lru_cache(maxsize=None)
def sample_inputs(R, S, Ld):
    """heads [R, mean L | raw scale L] uniform on [-30, 30] with the threshold planted in the raw-scale block, eps and the
    two upstream gradients of miw_sample_bwd (dz [R, S, L], g_hact [R, 2L]) N(0, 1)."""
    rng = np.random.default_rng(1000 * R + 10 * S + Ld)
    heads = rng.uniform(-30, 30, size=(R, 2 * Ld)).astype(np.float32)
    plant_threshold(heads[:, Ld:])
    n = lambda *s: rng.normal(size=s).astype(np.float32)
    return dict(heads=heads, eps=n(R, S, Ld), dz=n(R, S, Ld), g_hact=n(R, 2 * Ld))


@functools.lru_cache(maxsize=None)
def heads_inputs(M, d):
    """raw decoder heads [M, 3d] uniform on [-30, 30] with the threshold planted in each of the three blocks, and the
    upstream gradient of miw_heads_bwd N(0, 1)."""
    rng = np.random.default_rng(7000 * M + d)
    y = rng.uniform(-30, 30, size=(M, 3 * d)).astype(np.float32)
    for i in range(3):
        plant_threshold(y[:, i * d:(i + 1) * d])
    return dict(y=y, g=rng.normal(size=(M, 3 * d)).astype(np.float32))


# ---- whole-model cases: one MIWTrainer step / one API forward + backward against the float64 oracle.
# (B, S, d, L) -> seed per class.  The seeds were picked with the oracle alone (tests/test_miwae_oracle.py
# ::test_trainer_case_seeds_keep_the_kink_band_small asserts the condition on the CPU): at most ceil(1e-4 * units) hidden
# units have a float64 pre-activation within O.KINK_BAND of their layer's max, where fp32 may gate them the other way.
TRAINER_CASES = {
    (1, 1, 12, 10): dict(reg=1, van=0),       # units in the band: 0 of 1 024, 0 of 512
    (3, 5, 1, 1): dict(reg=2, van=1),         # 0 of 9 216, 0 of 4 608
    (37, 5, 70, 10): dict(reg=12, van=1),     # 0 of 113 664, 0 of 56 832
    (130, 3, 256, 64): dict(reg=5, van=9),    # 3 of 266 240, 1 of 133 120
    (64, 20, 12, 10): dict(reg=29, van=23),   # 22 of 688 128, 6 of 344 064; the reference's wine shape
}
ALPHA = 0.3


def _uniform_linear(rng, out_f, in_f):
    k = 1.0 / np.sqrt(in_f)  # nn.Linear's initialisation
    return (rng.uniform(-k, k, size=(out_f, in_f)).astype(np.float32), rng.uniform(-k, k, size=(out_f,)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def model_case(B, S, d, Ld, reg, seed):
    """params (state_dict keys -> fp32 arrays), x, mask, mask_p [B, d] (None for MIWAE) and eps [2P, B, S, L] = forward q,
    (forward p,) loss q, (loss p)."""
    rng = np.random.default_rng(seed)
    dims = [(HID, d), (HID, HID), (2 * Ld, HID), (HID, Ld), (HID, HID), (3 * d, HID)]
    params = {}
    for (o, i), kw, kb in zip(dims, O.KEYS[0::2], O.KEYS[1::2]):
        params[kw], params[kb] = _uniform_linear(rng, o, i)
    x = rng.random((B, d)).astype(np.float32)
    m = (rng.random((B, d)) < 0.7).astype(np.float32)
    mp = (m * (rng.random((B, d)) < 0.5)).astype(np.float32) if reg else None
    eps = rng.normal(size=(4 if reg else 2, B, S, Ld)).astype(np.float32)
    return dict(params=params, x=x, mask=m, mask_p=mp, eps=eps, B=B, S=S, d=d, L=Ld, reg=reg)


def trainer_case(shape, kind):
    return model_case(*shape, kind == "reg", TRAINER_CASES[shape][kind])


def oracle_inputs(c):
    """The float64 oracle's view of a model case: (params as leaves, x, mask, mask_p, [eps])."""
    p = {k: torch.from_numpy(v).double().requires_grad_() for k, v in c["params"].items()}
    t = lambda a: None if a is None else torch.from_numpy(a)
    return p, t(c["x"]), t(c["mask"]), t(c["mask_p"]), [torch.from_numpy(e) for e in c["eps"]]


def band_limit(units):
    return -(-units // 10000)  # 1e-4 of all units, rounded up


def api_loss(model, x, m, mp, eps, alpha):
    """forward (with injected forward draws) + loss (with injected loss draws), as train.py:102-113."""
    if mp is not None:
        z_q, mean_q, scale_q = model._encode(x, m, eps=eps[0])
        xm_q, xs_q, df_q = model.decoder(z_q)
        z_p, mean_p, scale_p = model._encode(x, mp, eps=eps[1])
        xm_p, xs_p, df_p = model.decoder(z_p)
        outs = (mean_p, scale_p, xm_p, xs_p, df_p, mean_q, scale_q, xm_q, xs_q, df_q)
        _, tl = model.loss(x, xm_p, xs_p, df_p, mean_p, scale_p, xm_q, xs_q, df_q, mean_q, scale_q, m, mp, 1,
                           alpha=alpha, eps=[eps[2], eps[3]])
        return tl, outs
    z, mean, scale = model._encode(x, m, eps=eps[0])
    xm, xs, df = model.decoder(z)
    _, tl = model.loss(x, xm, xs, df, mean, scale, m, 1, eps=eps[1])
    return tl, (mean, scale, xm, xs, df)
