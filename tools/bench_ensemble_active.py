"""The ensemble acquisition loop against the loop it replaces: active_learning_func, one member after the other.

    python tools/bench_ensemble_active.py [--cases 12:160:0:1,8,64;128:256:8:1,8] [--M 50] [--out profiles/ensemble_active.jsonl]

A case is d:n:max_steps:G,G,.. (max_steps 0 = all d - 1 steps).  For every (class, case, G) - Reg_VAE kl_reg and vanilla_VAE, one
test set of n rows shared by the members, M Monte-Carlo passes, one repeat:
    (a) ensemble     one EnsembleAcquirer.run (device draws, keep_im=True): device time by HIP events around the calls of a block,
                     and wall time of the block with ONE synchronise at its end; launches per step and per run
    (b) api          the path this replaces: active_learning_func(model=m, save=False) once per member, back to back (it ends
                     every step in .cpu() copies: synchronised).  Above --api-members members (default 8) it is timed on that many
                     and scaled to G; the record says so (`api_scaled_from`).
The two alternate in blocks; medians of five blocks with their spread (min, max), as tools/bench_ensemble_eval.py.  One JSON line
per case, appended to --out.  Warm-up: both forms run once at the timed shape before the first block; no gc.collect() anywhere."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpc_amd as vpc  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
BLOCKS = 5
L = 10


def stats(v, nd=1):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def case(cls_name, G, d, n, M, max_steps, api_members):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mk = (lambda: vpc.Reg_VAE(d, 500, 10, L, TP, "bench", "kl_reg").to(dev)) if cls_name == "Reg_VAE" else \
        (lambda: vpc.vanilla_VAE(d, 500, 10, L, TP, "bench").to(dev))
    g = torch.Generator().manual_seed(5)
    x_cpu = torch.rand(n, d, generator=g)
    tmask = torch.rand(n, d, generator=g) < 0.7
    x = x_cpu.to(dev)
    models = [mk() for _ in range(G)]
    acq = vpc.EnsembleAcquirer(models, seeds=list(range(G)))
    n_api = min(G, api_members)
    api_models = [mk() for _ in range(n_api)]  # (their own models: the API path must not re-pack the ensemble's images)
    vt = "reg_vae1" if cls_name == "Reg_VAE" else "vanilla_vae1"
    steps = d - 1 if not max_steps else min(max_steps, d - 1)

    def ens_call():
        return acq.run(x, M, repeats=1, max_steps=steps, keep_im=True)

    def api_round():
        for m in api_models:
            vpc.active_learning_func(None, x_cpu, tmask, 30, d, 500, 10, M, L, "bench", TP, "bench", vt, 1000, 1, 1, device=dev,
                                     reg_type="kl_reg", Repeat=1, model=m, save=False, max_steps=steps)

    # warm-up at the timed shape, and the number of calls that makes an ensemble block ~0.3 s
    ens_call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ens_call()
    torch.cuda.synchronize()
    calls = max(2, min(50, int(0.3 / max(time.perf_counter() - t0, 1e-6))))
    api_round()
    torch.cuda.synchronize()
    ens_dev, ens_wall, api = [], [], []
    for _ in range(BLOCKS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(calls):
            ens_call()
        e1.record()
        torch.cuda.synchronize()
        ens_wall.append((time.perf_counter() - t0) / calls * 1e3)
        ens_dev.append(e0.elapsed_time(e1) / calls)
        t0 = time.perf_counter()
        api_round()
        torch.cuda.synchronize()
        api.append((time.perf_counter() - t0) * 1e3 * G / n_api)
    ew, ed, ap = stats(ens_wall, 3), stats(ens_dev, 3), stats(api, 1)
    return dict(model=cls_name, d=d, G=G, n=n, M=M, steps=steps, repeats=1, keep_im=True, blocks=BLOCKS, calls_per_block=calls,
                launches_per_step=acq.launches_per_step, launches_per_run=acq.launches,
                ensemble_wall_ms=ew, ensemble_device_ms=ed, ensemble_wall_us_per_member_step=round(ew["median"] * 1e3 / (G * steps), 2),
                api_ms=ap, api_scaled_from=(n_api if n_api < G else None), api_ms_per_member=round(ap["median"] / G, 1),
                api_over_ensemble=round(ap["median"] / ew["median"], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="12:160:0:1,8,64;128:256:8:1,8")
    ap.add_argument("--M", type=int, default=50)
    ap.add_argument("--models", default="Reg_VAE,vanilla_VAE")
    ap.add_argument("--api-members", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_active.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble_active.py measures on the GPU: no device found")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in a.models.split(","):
        for c in a.cases.split(";"):
            d, n, max_steps, Gs = c.split(":")
            for G in [int(v) for v in Gs.split(",")]:
                line = json.dumps(case(name, G, int(d), int(n), a.M, int(max_steps), a.api_members))
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
