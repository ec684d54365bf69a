"""Inputs shared by the flow reward tests: the golden cases and the wide case (hid 500, d 128, n 32, M 4, a partly
observed mask, parameters of nn.Linear's default scale) that is checked against the float64 oracle."""
import numpy as np
import torch

import flow_oracle as F
from conftest import load_golden

GOLDEN = [("reg", "flow_reward_reg_d12.npz"), ("van", "flow_reward_van_d9.npz"), ("reg", "flow_reward_quirk_reg.npz")]
IDS = ["reg_d12", "van_d9", "quirk_reg"]
BIG = dict(d=128, hid=500, n=32, M=4, seed=35)


def params_of(g, prefix="param."):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def big_case():
    """x, mask, im, eps as float32 numpy arrays and the parameters.  The flagged share of this seed under the golden
    delta is asserted on the CPU (tests/test_flow_reward_oracle.py)."""
    c = BIG
    d, n, M = c["d"], c["n"], c["M"]
    g = np.random.default_rng(c["seed"])
    P = F.init_params(d, c["hid"], seed=c["seed"])
    x = g.random((n, d), dtype=np.float32)
    mask = (g.random((n, d)) < 0.4).astype(np.float32)
    mask[:, -1] = 0
    mask[3, -1] = 1
    mask[:, 17] = 1
    im = g.random((M, n, d), dtype=np.float32)
    eps = g.standard_normal((d - 1, M, 4, n, 10)).astype(np.float32)
    return P, x, mask, im, eps


def big_delta():
    """The wide case takes the delta of the reg golden (the same class and the same measurement)."""
    return float(load_golden("flow_reward_reg_d12.npz")["delta"])


def golden_delta():
    """The bin-edge distance the generator measured (the largest over the golden files)."""
    return max(float(load_golden(f)["delta"]) for _, f in GOLDEN)


def flow_model(fl, kind, d, hid, P, dev="cuda"):
    cls = fl.REG_VAEFlow if kind == "reg" else fl.VAEFlow
    m = cls(d, hid, 10, 10, {"batch_size": 64, "patience": 100})
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(np.asarray(v).copy()) for k, v in P.items() if k in sd})
    m.load_state_dict(sd)
    return m.to(dev)
