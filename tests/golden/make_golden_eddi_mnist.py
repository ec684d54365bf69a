"""Golden vectors for the MNIST point-net pair Reg_EDDI_mnist / vanilla_EDDI_mnist, produced by running the REFERENCE.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eddi_mnist.py

Authoring container only: imports /root/reference (never copied, never shipped) and stores DATA only.

  eddi_mnist_reg_d784.npz   Reg_EDDI_mnist (VAE.py:10-201), B = 8, K = 20, L = 10: inputs (x, bool masks), eps of the rsample()
                            calls, the 8 forward outputs, loss (kl_reg alpha in {0.5, 1.0}; ml_reg + its third draw) with the
                            parameter gradients, the train-stage llh_eval extras, the evaluate / llh_eval branch
  eddi_mnist_van_d784.npz   vanilla_EDDI_mnist (VAE.py:204-347): same (float mask as train.py:58, 97 passes it)
  eddi_mnist_reg_d200.npz   a ragged width (d not a multiple of 64, K = 7, L = 6)
  eddi_mnist_traj_{reg,van}_d784.npz  5 Adam steps exactly as train.py:87-117 runs them (B = 8)

The layer widths 500 / 500 / 200 are hard-coded in the classes, so one d = 784 model is 1.13 M floats.  Therefore
  * weights are NOT stored: `seed` is, and torch.manual_seed(seed) followed by this package's constructor reproduces the
    reference's initial state_dict bit for bit (tests/test_eddi_mnist_oracle.py checks that against `param_crc` and the
    sampled `param.*` entries);
  * the five large matrices (pnp_encoder2.{2,4}.weight, seq_decoder.{2,4,6}.weight) are stored - as parameters and as
    gradients - as every 97th element of the flattened tensor, gradients with the tensor's max-abs (`gmax.*`) beside them;
    every other tensor is stored in full.
"""
import os
import sys
import types
import zlib

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

from src.models.VAE import Reg_EDDI_mnist, vanilla_EDDI_mnist  # noqa: E402

TP = {"batch_size": 64, "patience": 100}
STRIDE = 97
SAMPLED = ("pnp_encoder2.2.weight", "pnp_encoder2.4.weight", "seq_decoder.2.weight", "seq_decoder.4.weight",
           "seq_decoder.6.weight")


def stored(k, a):
    return a.reshape(-1)[::STRIDE].copy() if k in SAMPLED else a.copy()


def peek_normals(shapes):
    st = torch.get_rng_state()
    eps = [torch.empty(s).normal_() for s in shapes]
    torch.set_rng_state(st)
    return eps


def sd_np(model, prefix):
    out = {}
    crc = 0
    for k, v in model.state_dict().items():
        a = v.detach().numpy()
        out[prefix + k] = stored(k, a)
        crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    return out, crc


def grads_np(model, tag):
    out = {}
    for k, p in model.named_parameters():
        if p.grad is not None:
            a = p.grad.detach().numpy()
            out[f"grad.{tag}.{k}"] = stored(k, a)
            out[f"gmax.{tag}.{k}"] = np.float64(np.abs(a).max())
    return out


def make_inputs(B, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, d, generator=g)
    mask = torch.rand(B, d, generator=g) < 0.7
    mask_p = mask & (torch.rand(B, d, generator=g) < 0.7)
    return x, mask, mask_p


def save(name, out):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes")


def gen_reg(d, K, L, B, seed):
    torch.manual_seed(seed)
    model = Reg_EDDI_mnist(d, 500, K, L, TP, "exp", "kl_reg")
    x, mask, mask_p = make_inputs(B, d, seed + 1)
    out, crc = sd_np(model, "param.")
    out.update(seed=np.int64(seed), param_crc=np.int64(crc), keys=np.array(list(model.state_dict().keys())),
               x=x.numpy(), mask=mask.numpy(), mask_p=mask_p.numpy(), K=np.int64(K), L=np.int64(L))
    eps_q, eps_p, eps_ml = peek_normals([(B, L), (B, L), (B, L)])
    names = ["mean_p", "logvar_p", "x_mean_p", "x_logvar_p", "mean_q", "logvar_q", "x_mean_q", "x_logvar_q"]
    xi = x.reshape(B, -1)  # the classes reshape any leading shape themselves
    for tag, reg_type, alpha in (("kl0.5", "kl_reg", 0.5), ("kl1.0", "kl_reg", 1.0), ("ml0.8", "ml_reg", 0.8)):
        st = torch.get_rng_state()
        model.reg_type = reg_type
        model.zero_grad()
        o = model.forward(xi, mask, mask_p, "train")
        r = model.loss(xi, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mask, mask_p, 1400, beta=0.9, alpha=alpha,
                       beta_annealing=(tag == "kl1.0"), llh_eval=True)
        r[1].backward()
        out[f"loss.{tag}"] = np.float64(r[1].item())
        out[f"re.{tag}"] = np.float64(r[2].item())
        out[f"re_imp.{tag}"] = np.float64(float(r[3]))
        out.update(grads_np(model, tag))
        torch.set_rng_state(st)
    model.reg_type = "kl_reg"
    for n, t in zip(names, o):
        out["fwd." + n] = t.detach().numpy()
    out.update(eps_q=eps_q.numpy(), eps_p=eps_p.numpy(), eps_ml=eps_ml.numpy())
    with torch.no_grad():
        r = model.loss(xi, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mask, mask_p, 7, llh_eval=True, stage="evaluate")
    out.update(eval_loss=np.float64(r[1].item()), eval_re=np.float64(r[2].item()), eval_re_imp=np.float64(r[3].item()))
    save(f"eddi_mnist_reg_d{d}.npz", out)
    print({k: float(v) for k, v in out.items() if k.startswith("loss.")})


def gen_van(d, K, L, B, seed):
    torch.manual_seed(seed)
    model = vanilla_EDDI_mnist(d, 500, K, L, TP, "exp")
    x, mask, _ = make_inputs(B, d, seed + 1)
    maskf = mask * torch.ones(mask.shape)  # train.py:58, 97
    out, crc = sd_np(model, "param.")
    out.update(seed=np.int64(seed), param_crc=np.int64(crc), keys=np.array(list(model.state_dict().keys())),
               x=x.numpy(), mask=mask.numpy(), K=np.int64(K), L=np.int64(L))
    (eps_q,) = peek_normals([(B, L)])
    model.zero_grad()
    o = model.forward(x, maskf)
    r = model.loss(x, o[2], o[3], o[0], o[1], 3, maskf, beta=0.8, llh_eval=True)
    r[1].backward()
    out.update(loss=np.float64(r[1].item()), re=np.float64(r[2].item()), re_imp=np.float64(r[3].item()))
    out.update(grads_np(model, "v"))
    for n, t in zip(["mean", "logvar", "x_mean", "x_logvar"], o):
        out["fwd." + n] = t.detach().numpy()
    out.update(eps_q=eps_q.numpy())
    save(f"eddi_mnist_van_d{d}.npz", out)
    print(out["loss"])


def gen_traj(kind, d=784, K=20, L=10, B=8, steps=5, seed=919):
    torch.manual_seed(seed)
    model = Reg_EDDI_mnist(d, 500, K, L, TP, "exp", "kl_reg") if kind == "reg" else vanilla_EDDI_mnist(d, 500, K, L, TP, "exp")
    opt = torch.optim.Adam(model.parameters(), lr=0.001)
    x, mask, _ = make_inputs(B, d, seed + 1)
    out, crc = sd_np(model, "param0.")
    out.update(seed=np.int64(seed), param_crc=np.int64(crc), x=x.numpy(), mask=mask.numpy(), K=np.int64(K), L=np.int64(L))
    g = torch.Generator().manual_seed(seed + 2)
    losses, eps_all, mp_all = [], [], []
    for s in range(steps):
        if kind == "reg":
            mask_p = mask & (torch.rand(B, d, generator=g) < 0.7)
            mp_all.append(mask_p.numpy())
            eps = peek_normals([(B, L), (B, L)])
            o = model.forward(x, mask, mask_p, stage="train")
            _, tl = model.loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mask, mask_p, s + 1,
                               beta_annealing=False, beta=1.0, alpha=0.5, alpha_annealing=True, stage="train")
        else:
            eps = peek_normals([(B, L)])
            mf = mask * torch.ones(mask.shape)
            o = model.forward(x, mf)
            _, tl = model.loss(x, o[2], o[3], o[0], o[1], s + 1, mf, beta_annealing=False, beta=1.0, stage="train")
        eps_all.append(np.stack([e.numpy() for e in eps]))
        opt.zero_grad()
        tl.backward()
        opt.step()
        losses.append(tl.item())
    out.update(sd_np(model, "param5.")[0])
    out.update(losses=np.array(losses, dtype=np.float64), eps=np.stack(eps_all))
    if mp_all:
        out["mask_p"] = np.stack(mp_all)
    save(f"eddi_mnist_traj_{kind}_d{d}.npz", out)
    print("traj", kind, losses)


if __name__ == "__main__":
    gen_reg(784, 20, 10, 8, 171)
    gen_van(784, 20, 10, 8, 181)
    gen_reg(200, 7, 6, 8, 172)
    gen_traj("reg")
    gen_traj("van")
