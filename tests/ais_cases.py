"""Inputs of the AIS parity cases shared by tests/test_ais_oracle.py (CPU) and tests/test_ais_gpu.py: decoder parameters,
x and every draw from a seeded torch generator, and the float64 oracle run of each case (computed once per session).

Shapes (6 temperatures each): the smallest at which the kernel can still go wrong.  A workgroup of the kernel carries
8 waves x 16 chains = 128 chains.
  a  d = 14,  L = 10, nb = 5,  n_sample = 7  ->  35 chains: ragged tiles, partial last wave
  b  d = 128, L = 15, nb = 16, n_sample = 8  -> 128 chains: full width
  c  d = 72,  L = 3,  nb = 37, n_sample = 7  -> 259 chains = two workgroups + 3: first width past the 64-column boundary
  d  d = 40,  L = 10, nb = 33, n_sample = 3  ->  99 chains
init_step_size = 0.2 (0.1 at d = 40) so that the reject branch runs; at the default 0.01 every proposal is accepted.
"""
import functools

import numpy as np
import torch

import ais_oracle as AO
from conftest import golden_params

# margin = 4 x the measured max |prob_fp32 - prob_fp64| of the CPU restatement (tests/ais_oracle.py) on the case, both
# likelihood signs, over the decisions with prob_fp64 <= 1 (u < 1: above that either format accepts).  The error grows
# with |H| ~ t * NLL, i.e. with d, so each case carries its own.  Seeds: the float64 oracle's smallest |prob - u| is
# above the margin (a 1.4e-2, b 4.7e-3, c 1.8e-3, d 4.7e-3, a_clip 6.4e-3), so it excludes no decision; the fp32
# restatement flips none.
CASES = {
    "a": dict(d=14, L=10, nb=5, n_sample=7, step=0.2, seed=38, margin=6.6e-5),      # measured 1.64e-5
    "b": dict(d=128, L=15, nb=16, n_sample=8, step=0.2, seed=80, margin=6.5e-4),    # measured 1.61e-4
    "c": dict(d=72, L=3, nb=37, n_sample=7, step=0.2, seed=2455, margin=1.38e-3),   # measured 3.43e-4
    "d": dict(d=40, L=10, nb=33, n_sample=3, step=0.1, seed=92, margin=2.1e-4),     # measured 5.07e-5
}
# case a again with grad_clip = 1.0, so that the clamp of AIS.py:196 is taken (the oracle counts the clamped components)
CLIP_CASE = {"a_clip": dict(d=14, L=10, nb=5, n_sample=7, step=0.2, seed=38, margin=1.8e-5)}  # measured 4.47e-6
T = 6
KEYS = ["seq_decoder.0.weight", "seq_decoder.0.bias", "seq_decoder.2.weight", "seq_decoder.2.bias",
        "seq_decoder.4.weight", "seq_decoder.4.bias"]


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = CASES[name] if name in CASES else CLIP_CASE[name]
    g = torch.Generator().manual_seed(c["seed"])
    d, L, B = c["d"], c["L"], c["nb"] * c["n_sample"]
    shapes = [(50, L), (50,), (100, 50), (100,), (d, 100), (d,)]
    fan = [L, L, 50, 50, 100, 100]
    # nn.Linear's uniform initialisation, weights doubled (as the goldens' models): a decoder that is not flat
    params = {k: (torch.rand(s, generator=g) * 2 - 1) / np.sqrt(f) * (2.0 if len(s) == 2 else 1.0)
              for k, s, f in zip(KEYS, shapes, fan)}
    x = torch.rand(c["nb"], d, generator=g)
    z0 = torch.randn(B, L, generator=g)
    v = torch.randn(T - 1, B, L, generator=g)
    u = torch.rand(T - 1, B, generator=g)
    return dict(params=params, x=x, z0=z0, v=v, u=u, schedule=AO.linear_schedule(T), **c)


@functools.lru_cache(maxsize=None)
def oracle(name, sign, dtype=torch.float64, grad_clip=1e4):
    i = inputs(name)
    return AO.run(i["params"], i["x"], i["schedule"], i["n_sample"], i["z0"], i["v"], i["u"], sign=sign, dtype=dtype,
                  init_step_size=i["step"], grad_clip=grad_clip)


# ---- the goldens recorded from the reference (tests/golden/make_golden_ais.py)
GOLDENS = ["ais_reg_d14.npz", "ais_van_d40.npz", "ais_corrected_d14.npz", "ais_backward_d14.npz"]


def golden_chain_inputs(g):
    """(params, x, z0, v, u, sign, mode, n_sample) of a golden; backward mode starts at the repeated post_z (AIS.py:173)."""
    n_sample, mode = int(g["n_sample"]), str(g["mode"])
    z0 = torch.from_numpy(g["z0"]) if mode == "forward" else torch.from_numpy(g["post_z"]).repeat(n_sample, 1)
    return dict(params=golden_params(g), x=torch.from_numpy(g["x"]), z0=z0, v=torch.from_numpy(g["v"]),
                u=torch.from_numpy(g["u"]), sign=-1.0 if bool(g["corrected"]) else 1.0, mode=mode, n_sample=n_sample)


def golden_chain_logw(g):
    """Per-chain logw: the reference hands log_mean_exp logw.view(n_sample, -1).transpose(0, 1) = [nb, n_sample]."""
    return torch.from_numpy(np.ascontiguousarray(g["logw_rows"].T)).reshape(-1)
