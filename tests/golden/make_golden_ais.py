"""Golden vectors for annealed importance sampling (src/utils/AIS.py), produced by running the REFERENCE's own
ais_trajectory.

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ais.py

Authoring container only: imports the reference checkout (never copied, never shipped) and stores DATA only.
`AIS.model_loader` (called with the wrong arity at AIS.py:120-121) is replaced by a function that returns a model built
here; everything below that line is the reference's code, run in a temporary working directory.  Recorded per file:
the decoder parameters (seq_decoder.*; the chain reads nothing else of the model), x, the schedule, every torch.randn / torch.rand draw in call order (z0, then v and u per
temperature), the per-chain logw handed to AIS.log_mean_exp, epsilon / accept_hist returned by the last accept_reject,
the returned per-batch means and the two saved tensors with their paths.

  ais_reg_d14.npz         Reg_VAE, d = 14, L = 10, nb = 6, n_sample = 4, 6 temperatures, linear schedule
  ais_van_d40.npz         vanilla_VAE, d = 40, L = 6, nb = 5, n_sample = 7, 9 temperatures, sigmoidial schedule
  ais_corrected_d14.npz   as ais_reg_d14 with AIS.neg_gaussian_log_likelihood replaced by its negation (real AIS)
  ais_backward_d14.npz    as ais_reg_d14 in mode="backward" (chains start at the repeated post_z)
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = os.environ.get("VPC_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
tv = types.ModuleType("torchvision")
tv.datasets = types.ModuleType("torchvision.datasets")
tv.transforms = types.ModuleType("torchvision.transforms")
sys.modules["torchvision"] = tv
sys.modules["torchvision.datasets"] = tv.datasets
sys.modules["torchvision.transforms"] = tv.transforms

from src.models.VAE import Reg_VAE, vanilla_VAE  # noqa: E402
from src.utils import AIS  # noqa: E402

TP = {"batch_size": 64, "patience": 100}


def gen(name, kind, d, L, nb, n_sample, schedule, seed, mode="forward", corrected=False):
    torch.manual_seed(seed)
    model = Reg_VAE(d, 500, 10, L, TP, "exp", "kl_reg") if kind == "reg" else vanilla_VAE(d, 500, 10, L, TP, "exp")
    with torch.no_grad():  # the default initialisation gives an almost flat decoder: sharpen it
        for k, p in model.named_parameters():
            if k.startswith("seq_decoder") and k.endswith("weight"):
                p.mul_(2.0)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(nb, d, generator=g)
    post_z = torch.randn(nb, L, generator=g)
    rec = {"randn": [], "rand": [], "logw": [], "eps": None, "hist": None}
    real_randn, real_rand, real_lme, real_ar, real_nll = torch.randn, torch.rand, AIS.log_mean_exp, AIS.accept_reject, \
        AIS.neg_gaussian_log_likelihood

    def randn(*a, **k):
        t = real_randn(*a, **k)
        rec["randn"].append(t.detach().clone().numpy())
        return t

    def rand(*a, **k):
        t = real_rand(*a, **k)
        rec["rand"].append(t.detach().clone().numpy())
        return t

    def lme(t):
        rec["logw"].append(t.detach().clone().numpy())  # [nb, n_sample] = logw.view(n_sample, -1).transpose(0, 1)
        return real_lme(t)

    def ar(*a, **k):
        z, e, h = real_ar(*a, **k)
        rec["eps"], rec["hist"] = e.detach().clone().numpy(), h.detach().clone().numpy()
        return z, e, h

    vae_type, data_type, mr, ep, stage = "reg_vae1" if kind == "reg" else "vanilla_vae1", "toy", 40, 7, "test"
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for sub in ("elbos", "latents"):
                os.makedirs(f"experiments/{vae_type}/{data_type}/{sub}/{mr}_missing/{ep}_epochs")
            AIS.model_loader = lambda *a, **k: model
            AIS.log_mean_exp, AIS.accept_reject = lme, ar
            torch.randn, torch.rand = randn, rand
            if corrected:
                AIS.neg_gaussian_log_likelihood = lambda *a: -real_nll(*a)
                # log_f_i binds its default argument when ais_trajectory runs, so the patched name is the one it sees
            torch.manual_seed(seed + 2)
            means = AIS.ais_trajectory([(x, post_z)], d, 500, 10, L, mr, data_type, TP, ep, vae_type, stage, 1, 1,
                                       mode=mode, schedule=np.asarray(schedule), n_sample=n_sample)
            f_ais = f"experiments/{vae_type}/{data_type}/elbos/{mr}_missing/{ep}_epochs/{stage}_ais.pt"
            f_lat = f"experiments/{vae_type}/{data_type}/latents/{mr}_missing/{ep}_epochs/{stage}_ais_true_latents.pt"
            saved_ais, saved_lat = torch.load(f_ais), torch.load(f_lat)
        finally:
            torch.randn, torch.rand = real_randn, real_rand
            AIS.log_mean_exp, AIS.accept_reject, AIS.neg_gaussian_log_likelihood = real_lme, real_ar, real_nll
            os.chdir(cwd)
    T = len(schedule)
    normals = rec["randn"]
    out = {"param." + k: v.detach().numpy().copy() for k, v in model.state_dict().items() if k.startswith("seq_decoder")}
    if mode == "forward":
        out["z0"] = normals[0]
        normals = normals[1:]
    assert len(normals) == T - 1 and len(rec["rand"]) == T - 1 and len(rec["logw"]) == 1
    out.update(x=x.numpy(), post_z=post_z.numpy(), schedule=np.asarray(schedule, dtype=np.float64),
               v=np.stack(normals), u=np.stack(rec["rand"]), logw_rows=rec["logw"][0], epsilon=rec["eps"],
               accept_hist=rec["hist"], means=np.array([m.item() for m in means], dtype=np.float64),
               saved_ais=saved_ais.detach().numpy(), saved_latents=saved_lat.detach().numpy(),
               file_ais=np.array(f_ais), file_latents=np.array(f_lat), n_sample=np.int64(n_sample), L=np.int64(L),
               mode=np.array(mode), corrected=np.bool_(corrected), vae_type=np.array(vae_type),
               data_type=np.array(data_type), missing_rate=np.int64(mr), max_epochs=np.int64(ep), stage=np.array(stage),
               ref_linear_schedule=AIS.linear_schedule(T), ref_sigmoidial_schedule=np.array(AIS.sigmoidial_schedule(T)))
    np.savez_compressed(os.path.join(OUT, name), **out)
    print(name, out["means"], "accept_hist", rec["hist"].mean(), "eps", rec["eps"][:3])


if __name__ == "__main__":
    gen("ais_reg_d14.npz", "reg", 14, 10, 6, 4, AIS.linear_schedule(6), 9101)
    gen("ais_van_d40.npz", "van", 40, 6, 5, 7, AIS.sigmoidial_schedule(9), 9102)
    gen("ais_corrected_d14.npz", "reg", 14, 10, 6, 4, AIS.linear_schedule(6), 9101, corrected=True)
    gen("ais_backward_d14.npz", "reg", 14, 10, 6, 4, AIS.linear_schedule(6)[::-1].copy(), 9101, mode="backward")
