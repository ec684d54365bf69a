"""Golden vectors for the evaluate stage of the mask-augmented and the point-net classes, produced by running the REFERENCE.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_family_eval.py

Authoring container only: imports /root/reference (never copied, never shipped) and stores DATA only.

  family_eval_d14.npz   for each of Reg_VAE_mask (VAE.py:510-667), vanilla_VAE_mask (:995-1116), Reg_EDDI (:670-853) and
                        vanilla_EDDI (:856-992) at d = 14, L = 10, B = 48 (K = 10 for the point-net pair), under the prefixes
                        mask_reg / mask_van / eddi_reg / eddi_van:  the state_dict, x, mask, eps_q (the rsample() of the q pass)
                        and the reference's own loss(..., stage='evaluate', llh_eval=True) triple
                        (print_loss, RE_q / B, RE_q_imputed / B) as eval_llh
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

from src.models.VAE import Reg_EDDI, Reg_VAE_mask, vanilla_EDDI, vanilla_VAE_mask  # noqa: E402

TP = {"batch_size": 64, "patience": 100}
D, L, B, K = 14, 10, 48, 10


def peek_normals(shape):
    st = torch.get_rng_state()
    eps = torch.empty(shape).normal_()
    torch.set_rng_state(st)
    return eps


def make_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, D, generator=g)
    mask = torch.rand(B, D, generator=g) < 0.7
    mask_p = mask & (torch.rand(B, D, generator=g) < 0.7)
    return x, mask, mask_p


def gen(tag, cls, regularised, seed):
    torch.manual_seed(seed)
    model = cls(D, 500, K, L, TP, "exp", "kl_reg") if regularised else cls(D, 500, K, L, TP, "exp")
    x, mask, mask_p = make_inputs(seed + 1)
    eps_q = peek_normals((B, L))  # (the q pass samples first in every forward)
    with torch.no_grad():
        if regularised:
            o = model.forward(x, mask, mask_p, "evaluate")
            r = model.loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mask, mask_p, 7, llh_eval=True, beta=1.0,
                           stage="evaluate")
        else:
            mf = mask * torch.ones(mask.shape)  # train.py:58,97
            o = model.forward(x, mf)
            r = model.loss(x, o[2], o[3], o[0], o[1], 7, mf, llh_eval=True, beta=1.0, stage="evaluate")
    out = {f"{tag}.param." + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    out.update({f"{tag}.x": x.numpy(), f"{tag}.mask": mask.numpy(), f"{tag}.eps_q": eps_q.numpy(),
                f"{tag}.eval_llh": np.array([r[0].item(), r[2].item(), r[3].item()], np.float64)})
    print(tag, out[f"{tag}.eval_llh"])
    return out


if __name__ == "__main__":
    out = {"K": np.int64(K), "L": np.int64(L)}
    out.update(gen("mask_reg", Reg_VAE_mask, True, 611))
    out.update(gen("mask_van", vanilla_VAE_mask, False, 612))
    out.update(gen("eddi_reg", Reg_EDDI, True, 613))
    out.update(gen("eddi_van", vanilla_EDDI, False, 614))
    np.savez_compressed(os.path.join(OUT, "family_eval_d14.npz"), **out)
