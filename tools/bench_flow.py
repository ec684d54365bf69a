"""Timings of the flow path (VAEFlow / REG_VAEFlow), one JSON line per measurement:

  * the FlowTrainer step and the API-path step (forward -> loss -> backward -> optim.Adam, train.py:77-117) at the
    config file's shape (Data/imputation_args.json: B = 64, wine d = 12, hid = 500, L = 10) and at B = 65 536,
  * eval_vae (evaluate.py:136-297, the flow branch) on 1 600 rows in batches of 64, M = 5,
  * beside each, the CPU restatement on 16 threads: the same network and flow in fp32 torch with autograd and Adam.

Each step line carries the GEMM FLOPs of one step, computed from the shapes (forward, dgrad and wgrad of every layer;
the encoder's first layer has no dgrad), and the rate they imply.

    python tools/bench_flow.py [--out profiles/flow.jsonl] [--only small|large|eval] [--steps N]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vpc_amd  # noqa: E402
import flow_oracle as FO  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
H, L = 500, 10


def gemm_flops(B, d, reg):
    """GEMM FLOPs of one training step: 2 MAC per FLOP pair, forward + dgrad + wgrad, both passes for REG."""
    layers = [(2 * d, H), (H, H), (H, 100), (L, H), (H, H), (H, H), (H, H), (H, d)]
    fwd = sum(k * n for k, n in layers)
    macs = 3 * fwd - 2 * d * H  # no dgrad into the encoder input
    return 2 * macs * B * (2 if reg else 1)


def gpu_time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def cpu_time(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def data(B, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, d, generator=g), torch.rand(B, d, generator=g) < 0.7


def cpu_step(model, x, m, alpha=0.5):
    """One fp32 CPU training step of the restatement (forward, loss, autograd backward, Adam)."""
    p = {k: model.state_dict()[k].detach().clone().requires_grad_() for k in FO.TRAINABLE}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    act = {"elu": torch.nn.functional.elu, "sigmoid": torch.sigmoid, None: lambda a: a}
    reg = model.regularised
    mf = m.float()
    mp = (m & (torch.rand(m.shape) < 0.7)).float() if reg else None
    B = x.shape[0]

    def mlp(layers, h):
        for n, k in layers:
            h = act[k](torch.nn.functional.linear(h, p[n + ".weight"], p[n + ".bias"]))
        return h

    def nll(xr, w):
        return ((x * w - xr * w) ** 2 / (2 * torch.exp(-8 * w)) - 4 * w + FO.HL).sum()

    def run():
        outs = []
        for mk in [mf] + ([mp] if reg else []):
            t = mlp(FO.ENC, torch.cat([x * mk, mk], 1))
            z, zlp = FO._torch_flow(t, torch.randn(B, L))
            outs.append((z, zlp, mlp(FO.DEC, z)))
        kl = lambda o: (o[1] + o[0] ** 2 / 2 + FO.HL).sum()
        q = outs[0]
        loss = nll(q[2], mf) + kl(q)
        if reg:
            pp = outs[1]
            loss = loss + alpha * ((q[1] - pp[1]).abs().sum() - loss + nll(pp[2], mp) + kl(pp) +
                                   nll(q[2], mf * (1 - mp)))
        opt.zero_grad()
        (loss / B).backward()
        opt.step()
    return run


def bench_step(kind, B, d, steps, warmup, emit, cpu_reps, cpu_B=None):
    """cpu_B: batch of the CPU measurement (a B = 65 536 step does not fit a 16-thread budget)."""
    cls = vpc_amd.REG_VAEFlow if kind == "reg" else vpc_amd.VAEFlow
    reg = kind == "reg"
    x, m = data(B, d)
    xd, md = x.cuda(), m.cuda()
    fl = gemm_flops(B, d, reg)
    torch.manual_seed(0)
    model = cls(d, H, 10, L, TP).cuda()
    tr = vpc_amd.FlowTrainer(model, lr=1e-3, seed=1)
    ms = gpu_time(lambda: tr.step(xd, md, alpha=0.5, p_missingness=30), steps, warmup)
    emit(dict(name=f"trainer_{kind}_b{B}_d{d}", path="FlowTrainer", kind=kind, B=B, d=d, hid=H, L=L, ms_per_step=ms,
              gemm_gflop=fl / 1e9, gemm_tflops=fl / ms / 1e9, loss=tr.loss_value()))
    torch.manual_seed(0)
    model = cls(d, H, 10, L, TP).cuda()
    model.flatten_parameters()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def api():
        mp = vpc_amd.create_missing_uci(xd.shape, 30, device="cuda") * md if reg else None
        _, (_, tl) = model.forward_loss(xd, md, mp, alpha=0.5)
        opt.zero_grad()
        tl.backward()
        opt.step()
    ms = gpu_time(api, max(2, steps // 2), max(1, warmup // 2))
    emit(dict(name=f"api_{kind}_b{B}_d{d}", path="API (forward/loss/backward/optim.Adam)", kind=kind, B=B, d=d, hid=H,
              L=L, ms_per_step=ms, gemm_gflop=fl / 1e9, gemm_tflops=fl / ms / 1e9))
    cB = cpu_B or B
    ms = cpu_time(cpu_step(cls(d, H, 10, L, TP), x[:cB], m[:cB]), cpu_reps)
    emit(dict(name=f"cpu_restatement_{kind}_b{B}_d{d}", path="CPU restatement fp32, 16 threads", kind=kind, B=cB, d=d,
              hid=H, L=L, ms_per_step=ms, threads=torch.get_num_threads()))


def bench_eval(kind, N, d, M, emit, reps):
    cls = vpc_amd.REG_VAEFlow if kind == "reg" else vpc_amd.VAEFlow
    vae_type = "reg_flow1" if kind == "reg" else "vanilla_flow1"
    x, m = data(N, d, 3)
    torch.manual_seed(0)
    model = cls(d, H, 10, L, TP).cuda()
    loaders = [([(x[i:i + 64], m[i:i + 64]) for i in range(0, N, 64)], "test")]

    def run():
        return vpc_amd.eval_vae(loaders, 50, d, H, 10, M, L, "wine", TP, "exp", vae_type, 10, 1, 1, model=model,
                                save=False)
    ms = gpu_time(run, reps, 1)
    emit(dict(name=f"eval_vae_{kind}_n{N}_d{d}", path="eval_vae (flow branch, batches of 64)", kind=kind, N=N, d=d,
              M=M, hid=H, ms=ms, rmse=float(run()["test"]["rmse"])))
    cpu_model = cls(d, H, 10, L, TP)

    def cpu():
        with torch.no_grad():
            for _ in range(M):
                for xb, mb in loaders[0][0]:
                    mk = [mb.float()] + ([(mb & (torch.rand(mb.shape) < 0.7)).float()] if kind == "reg" else [])
                    for mm in mk:
                        o = cpu_model.seq_encoder(torch.cat([xb * mm, mm], 1))
                        z, _ = FO._torch_flow(o, torch.randn(xb.shape[0], L))
                        cpu_model.decoder_mean(cpu_model.seq_decoder(z))
    ms = cpu_time(cpu, 1)
    emit(dict(name=f"cpu_restatement_eval_{kind}_n{N}_d{d}", path="CPU restatement fp32, 16 threads (forward only)",
              kind=kind, N=N, d=d, M=M, hid=H, ms=ms, threads=torch.get_num_threads()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
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
        "small": lambda: [bench_step(k, 64, 12, a.steps, a.warmup, emit, 20) for k in ("reg", "van")],
        "large": lambda: [bench_step(k, 65536, 12, max(3, a.steps // 10), 2, emit, 1, 4096) for k in ("reg", "van")],
        "eval": lambda: [bench_eval(k, 1600, 12, 5, emit, 3) for k in ("van", "reg")],
    }
    for name, fn in jobs.items():
        if a.only is None or a.only == name:
            fn()


if __name__ == "__main__":
    main()
