"""Timings of the MIWAE path (MIWAE / Reg_MIWAE), one JSON line per measurement:

  * the MIWTrainer step and the API-path step (forward -> loss -> backward -> optim.Adam, train.py:102-117) at the
    config file's shape (Data/imputation_args.json: B = 64, S = train_k = 20, L = 10, wine d = 12) and at B = 65 536,
    d = 128,
  * eval_miwae on 1 600 rows with valid_k = 5000, d = 12,
  * beside each, the CPU restatement on 16 threads: fp32 network, the bound of tests/miwae_oracle.py.

    python tools/bench_miwae.py [--out profiles/miwae.jsonl] [--only NAME] [--steps N]
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
import miwae_oracle as O  # noqa: E402

TP = {"batch_size": 64, "patience": 1}


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
    return torch.rand(B, d, generator=g), torch.rand(B, d, generator=g) < 0.5


def cpu_step(model, x, m, S, L, alpha=0.5):
    """One fp32 CPU training step of the restatement (forward, loss, autograd backward, Adam)."""
    p = {k: v.detach().clone().requires_grad_() for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    reg = model.regularised
    mp = m & (torch.rand(m.shape) < 0.7) if reg else None
    eps = [torch.randn(x.shape[0], S, L) for _ in range(4 if reg else 2)]

    def run():
        P = 2 if reg else 1
        mq, sq, zq = _enc32(p, x, m, eps[0])
        q = (_dec32(p, zq), mq, sq)
        pp = None
        if reg:
            mpm, sp, zp = _enc32(p, x, mp, eps[1])
            pp = (_dec32(p, zp), mpm, sp)
        lo, _ = _loss32(x, m, mp, q, pp, eps[P:], alpha)
        opt.zero_grad()
        lo.backward()
        opt.step()
    return run


def _enc32(p, x, m, e):
    h = torch.relu(torch.nn.functional.linear(x * m, p["seq_encoder.0.weight"], p["seq_encoder.0.bias"]))
    h = torch.relu(torch.nn.functional.linear(h, p["seq_encoder.2.weight"], p["seq_encoder.2.bias"]))
    mean, raw = torch.nn.functional.linear(h, p["seq_encoder.4.weight"], p["seq_encoder.4.bias"]).chunk(2, 1)
    sc = torch.nn.functional.softplus(raw)
    return mean, sc, mean[:, None] + sc[:, None] * e


def _dec32(p, z):
    h = torch.relu(torch.nn.functional.linear(z, p["seq_decoder.0.weight"], p["seq_decoder.0.bias"]))
    h = torch.relu(torch.nn.functional.linear(h, p["seq_decoder.2.weight"], p["seq_decoder.2.bias"]))
    a, b, c = torch.nn.functional.linear(h, p["seq_decoder.4.weight"], p["seq_decoder.4.bias"]).chunk(3, -1)
    return torch.sigmoid(a), torch.nn.functional.softplus(b) + 0.001, torch.nn.functional.softplus(c) + 3


def _loss32(x, m, mp, q, pp, e2, alpha, pairing="reference"):
    """The oracle's bound (float64 elementwise) on the fp32 network outputs."""
    return O.loss(x.double(), m, mp, _dbl(q), None if pp is None else _dbl(pp), [e.double() for e in e2], alpha,
                  pairing)


def _dbl(t):
    return (tuple(u.double() for u in t[0]), t[1].double(), t[2].double())


def bench_step(kind, B, d, S, L, steps, warmup, emit, cpu_reps, cpu_B=None):
    """cpu_B: batch of the CPU measurement (the float64 bound of a B = 65 536 step does not fit a 16-thread budget)."""
    cls = vpc_amd.Reg_MIWAE if kind == "reg" else vpc_amd.MIWAE
    x, m = data(B, d)
    xd, md = x.cuda(), m.cuda()
    torch.manual_seed(0)
    model = cls(d, 500, 10, L, TP, S, 1).cuda()
    tr = vpc_amd.MIWTrainer(model, lr=1e-3, seed=1)
    ms = gpu_time(lambda: tr.step(xd, md, alpha=0.5, p_missingness=30), steps, warmup)
    emit(dict(name=f"trainer_{kind}_b{B}_d{d}", path="MIWTrainer", kind=kind, B=B, d=d, S=S, L=L, ms_per_step=ms,
              loss=tr.loss_value()))
    torch.manual_seed(0)
    model = cls(d, 500, 10, L, TP, S, 1).cuda()
    model.flatten_parameters()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def api():
        mp = vpc_amd.create_missing_uci(xd.shape, 30, device="cuda") * md if kind == "reg" else None
        _, (_, tl) = model.forward_loss(xd, md, mp, epoch=1, alpha=0.5)
        opt.zero_grad()
        tl.backward()
        opt.step()
    ms = gpu_time(api, max(2, steps // 4), max(1, warmup // 4))
    emit(dict(name=f"api_{kind}_b{B}_d{d}", path="API (forward/loss/backward/optim.Adam)", kind=kind, B=B, d=d, S=S,
              L=L, ms_per_step=ms))
    cpu_model = cls(d, 500, 10, L, TP, S, 1)
    cB = cpu_B or B
    ms = cpu_time(cpu_step(cpu_model, x[:cB], m[:cB], S, L), cpu_reps)
    emit(dict(name=f"cpu_oracle_{kind}_b{B}_d{d}", path="CPU restatement, 16 threads", kind=kind, B=cB, d=d, S=S, L=L,
              ms_per_step=ms, threads=torch.get_num_threads()))


def bench_eval(kind, N, d, valid_k, emit, reps):
    cls = vpc_amd.Reg_MIWAE if kind == "reg" else vpc_amd.MIWAE
    vae_type = "reg_MIWAE1" if kind == "reg" else "vanilla_MIWAE1"
    x, m = data(N, d, 3)
    torch.manual_seed(0)
    model = cls(d, 500, 10, 10, TP, valid_k, 1).cuda()
    loaders = [([(x[i:i + 64], m[i:i + 64]) for i in range(0, N, 64)], "test")]

    def run():
        return vpc_amd.eval_miwae(loaders, 50, d, 500, 10, 1, 10, "wine", TP, "exp", vae_type, 10, valid_k, 1,
                                  model=model, save=False)
    ms = gpu_time(run, reps, 1)
    emit(dict(name=f"eval_miwae_{kind}_n{N}_d{d}", path="eval_miwae (batched, per-row pairing)", kind=kind, N=N, d=d,
              valid_k=valid_k, ms=ms, rmse=float(run()["test"])))
    # the same imputation on the CPU restatement: all rows at once, fp32 network, float64 bound
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}

    def cpu():
        with torch.no_grad():
            for xb, mb in loaders[0][0]:
                mq, sq, zq = _enc32(p, xb, mb, torch.randn(xb.shape[0], valid_k, 10))
                dec = _dec32(p, zq)
                e2 = [torch.randn(xb.shape[0], valid_k, 10)]
                _, a = _loss32(xb, mb, None, (dec, mq, sq), None, e2, 0.5, "per_row")
                O.impute(a, dec[0].double())
    ms = _once(cpu)
    emit(dict(name=f"cpu_oracle_eval_{kind}_n{N}_d{d}", path="CPU restatement, 16 threads (vanilla q pass only)",
              kind=kind, N=N, d=d, valid_k=valid_k, ms=ms, threads=torch.get_num_threads()))


def _once(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--steps", type=int, default=50)
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
        "small": lambda: [bench_step(k, 64, 12, 20, 10, a.steps, a.warmup, emit, 20) for k in ("reg", "van")],
        "large": lambda: [bench_step(k, 65536, 128, 20, 10, max(3, a.steps // 10), 2, emit, 1, 4096) for k in ("reg", "van")],
        "eval": lambda: [bench_eval(k, 1600, 12, 5000, emit, 3) for k in ("van", "reg")],
    }
    for name, fn in jobs.items():
        if a.only is None or a.only == name:
            fn()


if __name__ == "__main__":
    main()
