"""Golden vectors for annealed importance sampling (src/utils/AIS.py) on the families past the persistent kernel, produced by
running the REFERENCE's own ais_trajectory on the reference's own models.

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ais_families.py

Authoring container only: imports the reference checkout (never copied, never shipped) and stores DATA only.  The patching
is that of make_golden_ais.py: `AIS.model_loader` (called with the wrong arity at AIS.py:120-121) is replaced by a function
that returns a model built here; everything below that line is the reference's code, run in a temporary working
directory.  Recorded per file: the decoder tensors (the chain reads nothing else of the model), x, the schedule, every
torch.randn / torch.rand draw in call order (z0, then v and u per temperature), the per-chain logw handed to
AIS.log_mean_exp, epsilon / accept_hist returned by the last accept_reject, the returned per-batch means and the two saved
tensors with their paths.  The decoder weights are doubled (the default initialisation gives an almost flat decoder); the
MNAR log-variance head is doubled too and its bias set to -2, so that both Hardtanh bounds are reached.

  ais_nm_reg_d14.npz             REG_notMIWAE_v2, d = 14, L = 10, nb = 6, n_sample = 4, 6 temperatures, linear schedule
  ais_nm_van_d40_corrected.npz   notMIWAE_myversion, d = 40, L = 6, nb = 5, n_sample = 7, 9 temperatures, sigmoidial
                                 schedule, AIS.neg_gaussian_log_likelihood replaced by its negation (real AIS)
  ais_flow_van_d12.npz           VAEFlow (hid_dim 40), d = 12, L = 10, nb = 6, n_sample = 4, 6 temperatures, linear
  ais_wide_reg_d129.npz          Reg_VAE, d = 129, L = 10, nb = 6, n_sample = 4, 6 temperatures, linear
  ais_van_d14_L20.npz            vanilla_VAE, d = 14, L = 20, nb = 6, n_sample = 4, 6 temperatures, mode="backward"

No EDDI-mnist golden: its decoder tensors alone (L-200-500-500-784) are past the size of the largest .npz here.
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

from src.models import VAE  # noqa: E402
from src.utils import AIS  # noqa: E402

TP = {"batch_size": 64, "patience": 100}
DECODER_PREFIXES = {"mnar": ("seq_decoder", "x_mean", "x_logvar"), "flow": ("seq_decoder", "decoder_mean"),
                    "dense": ("seq_decoder",)}


def build(kind, d, L, hid):
    if kind == "nm_reg":
        return "mnar", "reg_notmiwae", VAE.REG_notMIWAE_v2(d, hid, 10, L, TP, 1, 1)
    if kind == "nm_van":
        return "mnar", "notmiwae", VAE.notMIWAE_myversion(d, hid, 10, L, TP, 1, 1)
    if kind == "flow_van":
        return "flow", "vaeflow", VAE.VAEFlow(d, hid, 10, L, TP)
    if kind == "reg":
        return "dense", "reg_vae1", VAE.Reg_VAE(d, hid, 10, L, TP, "exp", "kl_reg")
    return "dense", "vanilla_vae1", VAE.vanilla_VAE(d, hid, 10, L, TP, "exp")


def gen(name, kind, d, L, nb, n_sample, schedule, seed, mode="forward", corrected=False, hid=500):
    torch.manual_seed(seed)
    family, vae_type, model = build(kind, d, L, hid)
    prefixes = DECODER_PREFIXES[family]
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.split(".")[0] in prefixes and k.endswith("weight"):
                p.mul_(2.0)
            if k == "x_logvar.0.bias":
                p.fill_(-2.0)
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

    data_type, mr, ep, stage = "toy", 40, 7, "test"
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
            means = AIS.ais_trajectory([(x, post_z)], d, hid, 10, L, mr, data_type, TP, ep, vae_type, stage, 1, 1,
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
    out = {"param." + k: v.detach().numpy().copy() for k, v in model.state_dict().items() if k.split(".")[0] in prefixes}
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
               family=np.array(family), kind=np.array(kind), hid_dim=np.int64(hid),
               data_type=np.array(data_type), missing_rate=np.int64(mr), max_epochs=np.int64(ep), stage=np.array(stage))
    np.savez_compressed(os.path.join(OUT, name), **out)
    print(name, out["means"], "accept_hist", rec["hist"].mean(), "eps", rec["eps"][:3],
          os.path.getsize(os.path.join(OUT, name)), "bytes")


if __name__ == "__main__":
    gen("ais_nm_reg_d14.npz", "nm_reg", 14, 10, 6, 4, AIS.linear_schedule(6), 9201)
    gen("ais_nm_van_d40_corrected.npz", "nm_van", 40, 6, 5, 7, AIS.sigmoidial_schedule(9), 9202, corrected=True)
    gen("ais_flow_van_d12.npz", "flow_van", 12, 10, 6, 4, AIS.linear_schedule(6), 9203, hid=40)
    gen("ais_wide_reg_d129.npz", "reg", 129, 10, 6, 4, AIS.linear_schedule(6), 9204)
    gen("ais_van_d14_L20.npz", "van", 14, 20, 6, 4, AIS.linear_schedule(6)[::-1].copy(), 9205, mode="backward")
