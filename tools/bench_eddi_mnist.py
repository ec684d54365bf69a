"""Timings of the MNIST point-net pair (Reg_EDDI_mnist / vanilla_EDDI_mnist, d = 784, K = 20, L = 10), one JSON line per
measurement:

  * the EDDIMnistTrainer step and the API-path step (forward -> loss -> backward -> optim.Adam, train.py:87-117) at B = 64
    (the batch size of Data/imputation_args.json) and at B = 8 192, on synthetic [B, 28, 28] rows in [0, 1],
  * beside each, the CPU restatement (tests/eddi_mnist_oracle.py: the same network in fp32 torch with autograd and Adam) on
    16 threads of the same host - at B = 8 192 on 1 024 rows (the [B * 784, 22] tensor the reference materialises),
  * the device launches of one trainer step, counted by torch's profiler.

Each GPU figure is the median of `--reps` timed blocks of `--steps` steps after `--warmup` steps.

    python tools/bench_eddi_mnist.py [--out profiles/eddi_mnist.jsonl] [--only small|large] [--kinds reg,van] [--no-api] [--no-cpu]
    rocprofv3 --kernel-trace --stats -d DIR -o eddi_mnist -- python tools/bench_eddi_mnist.py --only large --kinds reg --no-api --no-cpu
    python tools/rocpd_stats.py DIR > profiles/eddi_mnist_kernel_stats.csv
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vpc_amd  # noqa: E402
import eddi_mnist_oracle as MO  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
D, K, L = 784, 20, 10


def macs_per_row():
    """MAC of one forward pass of one row: front end d (2 + K) K, trunk K-500-500-200-2L, decoder L-200-500-500-d."""
    return D * (2 + K) * K + K * 500 + 500 * 500 + 500 * 200 + 200 * 2 * L + L * 200 + 200 * 500 + 500 * 500 + 500 * D


def gpu_time(fn, steps, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return statistics.median(out), min(out), max(out)


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def make(kind):
    torch.manual_seed(0)
    if kind == "reg":
        return vpc_amd.Reg_EDDI_mnist(D, 500, K, L, TP, "exp", "kl_reg")
    return vpc_amd.vanilla_EDDI_mnist(D, 500, K, L, TP, "exp")


def bench(kind, B, a, emit, cpu_B):
    reg = kind == "reg"
    g = torch.Generator().manual_seed(0)
    x, m = torch.rand(B, 28, 28, generator=g), torch.rand(B, 28, 28, generator=g) < 0.7
    xd, md = x.cuda(), m.cuda()
    gflop = 2 * 3 * macs_per_row() * B * (2 if reg else 1) / 1e9  # forward + dgrad + wgrad, both passes for reg
    steps = a.steps if B <= 1024 else max(5, a.steps // 10)
    model = make(kind).cuda()
    tr = vpc_amd.EDDIMnistTrainer(model, lr=1e-3, seed=1)
    step = lambda: tr.step(xd, md, epoch=1, alpha=0.5, p_missingness=30)
    ms, lo, hi = gpu_time(step, steps, a.warmup, a.reps)
    rec = dict(name=f"trainer_{kind}_b{B}", path="EDDIMnistTrainer", kind=kind, B=B, d=D, K=K, L=L, ms_per_step=ms, ms_min=lo,
               ms_max=hi, samples_per_s=B / ms * 1e3, gflop_per_step=gflop, tflops=gflop / ms, loss=tr.loss_value())
    try:
        rec["launches_per_step"] = count_launches(step)
    except Exception as e:  # the profiler is optional: the timing stands without it
        rec["launches_per_step"] = None
        rec["launch_count_error"] = repr(e)[:200]
    emit(rec)
    if not a.no_api:
        model = make(kind).cuda()
        model.flatten_parameters()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)

        def api():
            mp = vpc_amd.create_missing_uci(xd.shape, 30, device="cuda") * md if reg else None
            _, (_, tl) = model.forward_loss(xd, md, mp, epoch=1, alpha=0.5)
            opt.zero_grad()
            tl.backward()
            opt.step()
        ms, lo, hi = gpu_time(api, max(3, steps // 2), max(2, a.warmup // 2), a.reps)
        emit(dict(name=f"api_{kind}_b{B}", path="API (forward/loss/backward/optim.Adam)", kind=kind, B=B, d=D, K=K, L=L,
                  ms_per_step=ms, ms_min=lo, ms_max=hi, samples_per_s=B / ms * 1e3, gflop_per_step=gflop, tflops=gflop / ms))
    if not a.no_cpu:
        cB = min(B, cpu_B)
        xc, mc = x[:cB].reshape(cB, D), m[:cB].reshape(cB, D)
        mp = mc & (torch.rand(cB, D) < 0.7) if reg else None
        ct = MO.TorchTrainer({k: v for k, v in make(kind).state_dict().items()}, L, vanilla=not reg)
        eps = torch.randn(2 if reg else 1, cB, L)
        ct.step(xc, mc, mp, eps)
        reps = 5 if cB <= 64 else 2
        t0 = time.perf_counter()
        for _ in range(reps):
            ct.step(xc, mc, mp, eps)
        ms = (time.perf_counter() - t0) / reps * 1e3
        emit(dict(name=f"cpu_restatement_{kind}_b{B}", path="CPU restatement fp32, 16 threads", kind=kind, B=cB, d=D, K=K, L=L,
                  ms_per_step=ms, samples_per_s=cB / ms * 1e3, threads=torch.get_num_threads()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--kinds", default="reg,van")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-api", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(16)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for name, B in (("small", 64), ("large", 8192)):
        if a.only is None or a.only == name:
            for kind in a.kinds.split(","):
                bench(kind, B, a, emit, 1024)


if __name__ == "__main__":
    main()
