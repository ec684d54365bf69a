"""Digest of what the host code of the wide dense classes and the two point-net families (wide.py, eddi.py, eddi_mnist.py,
ais._decoder_chain) computes: one line `case tensor sha256` per tensor, to compare two trees that load the same build of the
library.  Only names that both trees have are used.

  * trainers, 3 steps each, seed = 1, B = 16; model._flat, exp_avg, exp_avg_sq, tail, rng_offset, step_count:
      WideTrainer with device draws on Reg_VAE at obs_dim 129, vanilla_VAE_mask at obs_dim 65, Reg_VAE at obs_dim 14 with
      latent_dim 16;
      EDDITrainer, both classes (K = 10, latent 10) at obs_dim 12 and 14, chain path (VPC_STEP_SMALL=0) and small path (prints
      last_path), with device draws and with mask_p and eps injected;
      EDDIMnistTrainer, both classes (K = 4, latent 3) at obs_dim 784 and 20, drawn and injected,
  * eager, the seven classes of tests/test_trainer_images.py's B = 5 rows at B = 16: torch.manual_seed(0), forward_loss under
    grad, backward: the loss and every p.grad,
  * ais_chains(engine="gemm", seed=11) on Reg_VAE at obs_dim 129 and at obs_dim 14: logw, z, epsilon, accept_hist,
  * --construct (runs on the CPU): after torch.manual_seed(0), the state_dict key order and every tensor of the four
    point-net classes and Reg_VAE,
  * --time-wide: no digest; the median over five blocks of 400 WideTrainer steps (Reg_VAE, obs_dim 129, B = 128) in us.

    python tools/gemm_family_host_digest.py > profiles/gemm_family_host_digest_new.txt
"""
import hashlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vpc_amd as vpc  # noqa: E402

TP = {"batch_size": 16, "patience": 1}
B = 16
DENSE = {"Reg_VAE_d129": lambda: vpc.Reg_VAE(129, 500, 10, 10, TP, "exp", "kl_reg"),
         "vanilla_VAE_mask_d65": lambda: vpc.vanilla_VAE_mask(65, 500, 10, 10, TP, "exp"),
         "Reg_VAE_d14_L16": lambda: vpc.Reg_VAE(14, 500, 10, 16, TP, "exp", "kl_reg")}
EDDI = {"Reg_EDDI": lambda d: vpc.Reg_EDDI(d, 500, 10, 10, TP, "exp", "kl_reg"),
        "vanilla_EDDI": lambda d: vpc.vanilla_EDDI(d, 500, 10, 10, TP, "exp")}
MNIST = {"Reg_EDDI_mnist": lambda d: vpc.Reg_EDDI_mnist(d, 500, 4, 3, TP, "exp", "kl_reg"),
         "vanilla_EDDI_mnist": lambda d: vpc.vanilla_EDDI_mnist(d, 500, 4, 3, TP, "exp")}


def emit(case, name, value):
    if torch.is_tensor(value):
        data = value.detach().contiguous().cpu().numpy().tobytes()
    else:
        data = repr(value).encode()
    print(f"{case} {name} {hashlib.sha256(data).hexdigest()}", flush=True)


def data(d, L, seed=0, rows=B):
    g = torch.Generator().manual_seed(seed)
    x, m = torch.rand(rows, d, generator=g), torch.rand(rows, d, generator=g) < 0.7
    mp = m & (torch.rand(rows, d, generator=g) < 0.7)
    eps = torch.randn(3, rows, L, generator=g)
    return x.cuda(), m.cuda(), mp.cuda(), eps.cuda()


def seeded(make, *a):
    torch.manual_seed(0)
    return make(*a).cuda()


def trainer_case(case, tr, step, note=None):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    if note is not None:
        print(f"{case} note {note()}", flush=True)
    for name in ("exp_avg", "exp_avg_sq", "tail", "rng_offset", "step_count"):
        emit(case, name, getattr(tr, name))
    emit(case, "flat", tr.model._flat)


def trainers():
    for name, make in DENSE.items():
        model = seeded(make)
        x, m, _, _ = data(model.obs_dim, model.latent_dim)
        tr = vpc.WideTrainer(model, seed=1)
        trainer_case(f"wide_{name}", tr, lambda: tr.step(x, m, alpha=0.5, p_missingness=30))
    for path, rows in (("chain", "0"), ("small", str(1 << 30))):
        os.environ["VPC_STEP_SMALL"] = rows
        for name, make in EDDI.items():
            for d in (12, 14):
                x, m, mp, eps = data(d, 10)
                for draws, inj in (("drawn", {}), ("injected", dict(mask_p=mp, eps_q=eps[0], eps_p=eps[1], eps_ml=eps[2]))):
                    tr = vpc.EDDITrainer(seeded(make, d), seed=1)
                    trainer_case(f"eddi_{path}_{name}_d{d}_{draws}", tr, lambda: tr.step(x, m, alpha=0.5, p_missingness=30, **inj),
                                 lambda: f"last_path={tr.last_path}")
    del os.environ["VPC_STEP_SMALL"]
    for name, make in MNIST.items():
        P = 2 if name.startswith("Reg") else 1
        for d in (784, 20):
            x, m, mp, eps = data(d, 3)
            for draws, inj in (("drawn", {}), ("injected", dict(mask_p=mp, eps=eps[:P], eps_ml=eps[2]))):
                tr = vpc.EDDIMnistTrainer(seeded(make, d), seed=1)
                trainer_case(f"mnist_{name}_d{d}_{draws}", tr, lambda: tr.step(x, m, alpha=0.5, p_missingness=30, **inj))


def eager():
    cases = list(DENSE.items()) + [(k, lambda f=f: f(14)) for k, f in EDDI.items()] + \
        [(k, lambda f=f: f(20)) for k, f in MNIST.items()]
    for name, make in cases:
        model = seeded(make)
        x, m, mp, _ = data(model.obs_dim, model.latent_dim)
        if "mnist" in name:
            x, m, mp = (t.view(B, 4, 5) for t in (x, m, mp))
        torch.manual_seed(0)
        _, ret = model.forward_loss(x, m, mp if model.regularised else None, epoch=1, alpha=0.5)
        ret[1].backward()
        torch.cuda.synchronize()
        emit(f"eager_{name}", "loss", ret[1])
        for k, p in model.named_parameters():
            if p.grad is not None:
                emit(f"eager_{name}", f"grad:{k}", p.grad)


def ais():
    for d in (129, 14):
        model = seeded(lambda: vpc.Reg_VAE(d, 500, 10, 10, TP, "exp", "kl_reg"))
        x = data(d, 10, 4, rows=4)[0]
        out = vpc.ais.ais_chains(model, x, np.linspace(0.0, 1.0, 6), 3, seed=11, engine="gemm")
        torch.cuda.synchronize()
        for k, t in zip(("logw", "z", "epsilon", "accept_hist"), out):
            emit(f"ais_gemm_Reg_VAE_d{d}", k, t)


def construct():
    for name, make in [(k, lambda f=f: f(14)) for k, f in EDDI.items()] + [(k, lambda f=f: f(20)) for k, f in MNIST.items()] + \
            [("Reg_VAE_d129", DENSE["Reg_VAE_d129"])]:
        torch.manual_seed(0)
        sd = make().state_dict()
        emit(f"construct_{name}", "keys", list(sd))
        for k, t in sd.items():
            emit(f"construct_{name}", k, t)


def time_wide(blocks=5, steps=400):
    torch.manual_seed(0)
    model = vpc.Reg_VAE(129, 500, 10, 10, {"batch_size": 128, "patience": 1}, "exp", "kl_reg").cuda()
    x, m, _, _ = data(129, 10, rows=128)
    tr = vpc.WideTrainer(model, seed=1)
    times = []
    for _ in range(blocks):
        for _ in range(50):
            tr.step(x, m, alpha=0.5, p_missingness=30)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step(x, m, alpha=0.5, p_missingness=30)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / steps * 1e6)
    print(f"wide_step_us {statistics.median(times):.1f} " + " ".join(f"{t:.1f}" for t in times), flush=True)


if __name__ == "__main__":
    if "--construct" in sys.argv:
        construct()
        raise SystemExit(0)
    if not torch.cuda.is_available():
        raise SystemExit("gemm_family_host_digest.py runs on the GPU: no device found")
    if "--time-wide" in sys.argv:
        time_wide()
        raise SystemExit(0)
    trainers()
    eager()
    ais()
