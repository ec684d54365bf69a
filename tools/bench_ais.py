"""Timings of annealed importance sampling (vpc_amd.ais), one JSON line per measurement:

  * ais_chains at the wine shape (d = 12, nb = 64, n_sample = 100) and at d = 128, nb = 1 600, n_sample = 100 with the
    full 500-point schedule, and the GEMM-equivalent rate of the kernel (11 forwards + 11 dgrads per temperature),
  * "launch" records: the time of ONE launch carrying k temperatures at the large shape - what fixes temps_per_launch,
  * the same loop on the API path (model.decoder + torch.autograd.grad on the GPU) on a short schedule, scaled to 500,
  * the CPU restatement (tests/ais_oracle.py, fp32, 16 threads) on a short schedule and fewer chains, scaled likewise.

    python tools/bench_ais.py [--out profiles/ais.jsonl] [--only small|large|launch|api|cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vpc_amd  # noqa: E402
import ais_oracle as AO  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
L = 10
SHAPES = {"small": (12, 64, 100), "large": (128, 1600, 100)}


def gemm_flops(d, B, temps, leapfrog=10):
    """Forward + dgrad of the decoder chain, leapfrog + 1 passes per temperature, 2 FLOP per MAC."""
    macs = L * 50 + 50 * 100 + 100 * d
    return 2 * 2 * macs * B * (leapfrog + 1) * temps


def model_for(d):
    torch.manual_seed(0)
    return vpc_amd.Reg_VAE(d, 500, 10, L, TP, "exp", "kl_reg").cuda()


def timed(fn, reps=1):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def bench_chains(name, emit, tpl):
    d, nb, ns = SHAPES[name]
    model = model_for(d)
    x = torch.rand(nb, d, generator=torch.Generator().manual_seed(1)).cuda()
    sched = vpc_amd.ais.linear_schedule(500)
    ms = timed(lambda: vpc_amd.ais_chains(model, x, sched, ns, seed=3, temps_per_launch=tpl))
    fl = gemm_flops(d, nb * ns, 499)
    logw = vpc_amd.ais_chains(model, x, sched, ns, seed=3, temps_per_launch=tpl)[0]
    emit(dict(name=f"ais_chains_{name}", path="ais_chains (persistent kernel)", d=d, nb=nb, n_sample=ns, temps=499,
              temps_per_launch=tpl, ms=ms, gemm_gflop=fl / 1e9, gemm_tflops=fl / ms / 1e9,
              logw_mean=float(logw.mean())))


def bench_launch(emit):
    d, nb, ns = SHAPES["large"]
    model = model_for(d)
    x = torch.rand(nb, d, generator=torch.Generator().manual_seed(1)).cuda()
    for k in (1, 2, 4, 8, 16, 32):
        sched = vpc_amd.ais.linear_schedule(k + 1)
        ms = timed(lambda: vpc_amd.ais_chains(model, x, sched, ns, seed=3, temps_per_launch=k), reps=3)
        emit(dict(name=f"launch_large_k{k}", path="one vpc_ais_run launch", d=d, nb=nb, n_sample=ns, temps=k, ms=ms))


def api_loop(model, x, sched, ns, step=0.01, leapfrog=10):
    """AIS.py:155-217 on the API path: model.decoder + torch.autograd.grad, every tensor on the GPU."""
    B = x.shape[0] * ns
    xb = x.repeat(ns, 1)
    xlv = model._x_logvar_value
    z = torch.randn(B, L, device="cuda")
    eps = torch.full((B,), step, device="cuda")
    hist = torch.zeros(B, device="cuda")
    logw = torch.zeros(B, device="cuda")

    def log_f(zz, t):
        mean, _ = model.decoder(zz)
        nll = torch.sum(0.5 * (xb - mean) ** 2 * np.exp(-xlv) + 0.5 * xlv + 0.9189385332, 1)
        return -0.5 * (zz * zz).sum(1) + t * nll

    for j, (t0, t1) in enumerate(zip(sched[:-1], sched[1:]), 1):
        with torch.no_grad():
            logw += log_f(z, float(t1)) - log_f(z, float(t0))
        v0 = torch.randn(B, L, device="cuda")

        def grad_U(zz):
            zz = zz.detach().requires_grad_(True)
            (g,) = torch.autograd.grad((-log_f(zz, float(t1))).sum(), zz)
            return g.clamp(-1e4, 1e4)
        e = eps.view(-1, 1)
        zz = z
        vv = v0 - grad_U(zz) * e * 0.5
        for i in range(1, leapfrog + 1):
            zz = zz + vv * e
            if i < leapfrog:
                vv = vv - grad_U(zz) * e
        vv = -(vv - grad_U(zz) * e * 0.5)
        with torch.no_grad():
            h0 = 0.5 * (v0 * v0).sum(1) - log_f(z, float(t1))
            h1 = 0.5 * (vv * vv).sum(1) - log_f(zz, float(t1))
            acc = torch.exp(h0 - h1) > torch.rand(B, device="cuda")
            z = torch.where(acc.view(-1, 1), zz, z).detach()
            hist += acc.float()
            eps = (eps * torch.where(hist / j > 0.65, 1.02, 0.98)).clamp(1e-4, 0.5)
    return logw


def bench_api(emit, temps=4):
    for name, (d, nb, ns) in SHAPES.items():
        model = model_for(d)
        x = torch.rand(nb, d, generator=torch.Generator().manual_seed(1)).cuda()
        sched = vpc_amd.ais.linear_schedule(500)[:temps + 1]
        ms = timed(lambda: api_loop(model, x, sched, ns))
        emit(dict(name=f"api_loop_{name}", path="API path (model.decoder + autograd.grad)", d=d, nb=nb, n_sample=ns,
                  temps_measured=temps, ms_measured=ms, ms_scaled_499=ms * 499 / temps))


def bench_cpu(emit, temps=2):
    for name, (d, nb, ns) in SHAPES.items():
        nbc = min(nb, 64)  # the large shape does not fit a 16-thread budget: measured on 64 rows, scaled by rows
        g = torch.Generator().manual_seed(1)
        m = vpc_amd.Reg_VAE(d, 500, 10, L, TP, "exp", "kl_reg")
        params = {k: v for k, v in m.state_dict().items() if k.startswith("seq_decoder")}
        B = nbc * ns
        args = (params, torch.rand(nbc, d, generator=g), vpc_amd.ais.linear_schedule(500)[:temps + 1], ns,
                torch.randn(B, L, generator=g), torch.randn(temps, B, L, generator=g), torch.rand(temps, B, generator=g))
        AO.run(*args, dtype=torch.float32)
        t0 = time.perf_counter()
        AO.run(*args, dtype=torch.float32)
        ms = (time.perf_counter() - t0) * 1e3
        emit(dict(name=f"cpu_restatement_{name}", path="CPU restatement fp32, 16 threads", d=d, nb=nbc, n_sample=ns,
                  temps_measured=temps, ms_measured=ms, ms_scaled_499_full_rows=ms * 499 / temps * nb / nbc,
                  threads=torch.get_num_threads()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--temps-per-launch", type=int, default=None)
    a = ap.parse_args()
    torch.set_num_threads(16)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    jobs = {
        "launch": lambda: bench_launch(emit),
        "small": lambda: bench_chains("small", emit, a.temps_per_launch),
        "large": lambda: bench_chains("large", emit, a.temps_per_launch),
        "api": lambda: bench_api(emit),
        "cpu": lambda: bench_cpu(emit),
    }
    for name, fn in jobs.items():
        if a.only is None or a.only == name:
            fn()


if __name__ == "__main__":
    main()
