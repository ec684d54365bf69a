"""Golden vectors for the active-variable-selection reward (BASELINE config 5) of the encoder families beyond the plain
Reg_VAE: the reference's own R_lindley_chain (src/experiment_main/evaluate.py:514-542) for every candidate feature of every
row, on a briefly trained

    Reg_EDDI      (point-net encoder, K = 10, L = 10)      -> reward_eddi_d14.npz
    Reg_VAE_mask  (encoder input [x*mask | mask])           -> reward_vaemask_d14.npz
    Reg_VAE       at obs_dim = 129 (wider than one 128 tile) -> reward_d129.npz

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_reward_families.py

Authoring container only: imports /root/reference (never copied, never shipped) and stores DATA only.  Each file holds
param.* (state_dict, reference naming), x, im [M][n][d] and, for the masks t0 (target unobserved) and t1 (target observed
in about half the rows: exercises the temp_x[loc, -1] carry-over between MC samples, evaluate.py:531-536), mask_*, R_*
(-1e4 where observed) and chaini_I / chaini_II of candidate 3 (kl1_*, kl2_*).
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
tv = types.ModuleType("torchvision")
tv.datasets = types.ModuleType("torchvision.datasets")
tv.transforms = types.ModuleType("torchvision.transforms")
sys.modules["torchvision"] = tv
sys.modules["torchvision.datasets"] = tv.datasets
sys.modules["torchvision.transforms"] = tv.transforms

from src.models.VAE import Reg_EDDI, Reg_VAE, Reg_VAE_mask  # noqa: E402
from src.experiment_main.evaluate import R_lindley_chain, chaini_I, chaini_II  # noqa: E402

TP = {"batch_size": 64, "patience": 100}
L = 10


def correlated(rows, d, g):
    """Rows whose columns share three factors, so that a feature carries information about the target (last column)."""
    base = torch.rand(rows, 3, generator=g)
    mix = torch.rand(3, d, generator=g)
    data = torch.sigmoid(3.0 * (base @ mix / mix.sum(0) - 0.5)) + 0.05 * torch.rand(rows, d, generator=g)
    return (data - data.min(0).values) / (data.max(0).values - data.min(0).values)


def train_briefly(model, xtr, g, steps=150):
    """Reg_* training steps (model.forward + model.loss, kl_reg): rewards of a freshly initialised encoder are fp32
    round-off, those of a trained one are not."""
    B, d = xtr.shape
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    for s in range(steps):
        mtr = torch.rand(B, d, generator=g) < 0.7
        mp = mtr & (torch.rand(B, d, generator=g) < 0.7)
        o = model.forward(xtr, mtr, mp, "train")
        _, tl = model.loss(xtr, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mtr, mp, s + 1, alpha=1.0)
        opt.zero_grad()
        tl.backward()
        opt.step()


def gen(name, model, d, n, M, seed):
    g = torch.Generator().manual_seed(seed)
    data = correlated(n + 256, d, g)
    train_briefly(model, data[n:], g)
    model.eval()
    x = data[:n].clone()
    im = torch.rand(M, n, d, generator=g)
    out = {"param." + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    for tag, target_obs in (("t0", 0.0), ("t1", 0.5)):
        mask = (torch.rand(n, d, generator=g) < 0.6).float()
        mask[:, -1] = (torch.rand(n, generator=g) < target_obs).float()
        R = -1e4 * torch.ones(n, d - 1)
        with torch.no_grad():
            for u in range(d - 1):
                loc = np.where(mask[:, u] == 0)[0]
                if len(loc):
                    R[loc, u] = R_lindley_chain(u, x, mask, M, model, im, loc).float()
            k1 = chaini_I(x, mask, 3, model)
            k2 = chaini_II(x, mask, 3, model)
        live = R != -1e4
        rmax = float(R[live].abs().max())
        assert rmax > 1e-4, (name, tag, rmax)  # well above the ~5e-7 round-off of an untrained encoder
        out.update({f"mask_{tag}": mask.numpy(), f"R_{tag}": R.numpy(), f"kl1_{tag}": k1.numpy(), f"kl2_{tag}": k2.numpy()})
        print(name, tag, "max |R|", rmax)
    out.update(x=x.numpy(), im=im.numpy(), L=np.int64(L))
    np.savez_compressed(os.path.join(OUT, name), **out)


if __name__ == "__main__":
    torch.manual_seed(4242)
    gen("reward_eddi_d14.npz", Reg_EDDI(14, 500, 10, L, TP, "exp", "kl_reg"), 14, 24, 5, 4243)
    torch.manual_seed(4343)
    gen("reward_vaemask_d14.npz", Reg_VAE_mask(14, 500, 10, L, TP, "exp", "kl_reg"), 14, 24, 5, 4344)
    torch.manual_seed(4444)
    gen("reward_d129.npz", Reg_VAE(129, 500, 10, L, TP, "exp", "kl_reg"), 129, 6, 5, 4445)
