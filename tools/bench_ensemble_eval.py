"""Ensemble evaluation against the evaluation it replaces: eval_vae, one member after the other.

    python tools/bench_ensemble_eval.py [--G 1,8,64] [--d 12,128] [--N 1600] [--batch 64] [--M 50] [--out profiles/ensemble_eval.jsonl]

For every (class, d, G) - Reg_VAE kl_reg and vanilla_VAE, one data set of N rows shared by the members, M Monte-Carlo passes:
    (a) ensemble     one EnsembleEvaluator.evaluate call (device draws): device time by HIP events around the calls of a block,
                     and wall time of the block with ONE synchronise at its end; launches per call; ns per (member x row x pass)
    (b) api          the path this replaces: harness.eval_vae(model=..., save=False) once per member, back to back.  Its loader is
                     a list of DEVICE-resident batches (no host-to-device copy per batch: this favours (b)).  Above --api-members
                     members (default 8) it is timed on that many and scaled to G; the record says so (`api_scaled_from`).
The two alternate in blocks; medians of five blocks with their spread (min, max), as tools/bench_ensemble.py.  One JSON line per
case, appended to --out.  Warm-up: both forms run once at the timed shape before the first block; no gc.collect() anywhere."""
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
from vpc_amd import harness as H  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
BLOCKS = 5
L = 10


def stats(v, nd=1):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def case(cls_name, G, d, N, batch, M, api_members):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mk = (lambda: vpc.Reg_VAE(d, 500, 10, L, TP, "bench", "kl_reg").to(dev)) if cls_name == "Reg_VAE" else \
        (lambda: vpc.vanilla_VAE(d, 500, 10, L, TP, "bench").to(dev))
    g = torch.Generator().manual_seed(5)
    x = torch.rand(N, d, generator=g).to(dev)
    mask = (torch.rand(N, d, generator=g) < 0.7).to(dev)
    models = [mk() for _ in range(G)]
    ev = vpc.EnsembleEvaluator(models, seeds=list(range(G)))
    n_api = min(G, api_members)
    api_models = [mk() for _ in range(n_api)]  # (their own models: eval_vae must not re-pack the ensemble's images)
    loader = [(x[lo:lo + batch], mask[lo:lo + batch]) for lo in range(0, N, batch)]
    vt = "reg_vae1" if cls_name == "Reg_VAE" else "vanilla_vae1"

    def ens_call():
        return ev.evaluate(x, mask, batch, M, epoch=1000, beta=1.0)

    def api_round():
        for m in api_models:
            H.eval_vae([(loader, "test")], 30, d, 500, 10, M, L, "bench", TP, "bench", vt, 1000, 1, 1, device=dev,
                       reg_type="kl_reg", model=m, save=False)

    # warm-up at the timed shape, and the number of calls that makes an ensemble block ~0.3 s
    ens_call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ens_call()
    torch.cuda.synchronize()
    calls = max(3, min(200, int(0.3 / max(time.perf_counter() - t0, 1e-6))))
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
        api_round()  # (eval_vae ends in .cpu(): synchronised)
        torch.cuda.synchronize()
        api.append((time.perf_counter() - t0) * 1e3 * G / n_api)
    ew, ed, ap = stats(ens_wall, 3), stats(ens_dev, 3), stats(api, 1)
    tb = ev.tables(N, batch, M)[0]
    return dict(model=cls_name, d=d, G=G, N=N, batch=batch, M=M, blocks=BLOCKS, calls_per_block=calls,
                tiles=int(tb.tiles.shape[0]), batches=int(tb.batches.shape[0]), launches_per_call=ev.launches,
                ensemble_wall_ms=ew, ensemble_device_ms=ed, ns_per_member_row_pass=round(ed["median"] * 1e6 / (G * N * M), 3),
                api_ms=ap, api_scaled_from=(n_api if n_api < G else None), api_ms_per_member=round(ap["median"] / G, 1),
                api_loader="device-resident batches", api_over_ensemble=round(ap["median"] / ew["median"], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", default="1,8,64")
    ap.add_argument("--d", default="12,128")
    ap.add_argument("--N", type=int, default=1600)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--M", type=int, default=50)
    ap.add_argument("--models", default="Reg_VAE,vanilla_VAE")
    ap.add_argument("--api-members", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_eval.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble_eval.py measures on the GPU: no device found")
    ints = lambda s: [int(v) for v in s.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in a.models.split(","):
        for d in ints(a.d):
            for G in ints(a.G):
                line = json.dumps(case(name, G, d, a.N, a.batch, a.M, a.api_members))
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
