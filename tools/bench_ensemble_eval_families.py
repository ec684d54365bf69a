"""Ensemble evaluation of the mask-augmented and point-net members against the evaluation it replaces and against the plain kernel.

    python tools/bench_ensemble_eval_families.py [--G 1,8,64] [--d 12] [--N 1600] [--batch 64] [--M 50]
                                                 [--out profiles/ensemble_eval_families.jsonl] [--notes profiles/..._notes.md]

For every (family, G) - Reg_VAE_mask, Reg_EDDI at K = 10 and at K = 20, all kl_reg; one data set of N rows shared by the members,
M Monte-Carlo passes - the protocol of tools/bench_ensemble_eval.py:
    (a) ensemble     one MaskEnsembleEvaluator / EDDIEnsembleEvaluator.evaluate call (device draws): device time by HIP events
                     around the calls of a block, wall time of the block with ONE synchronise at its end; launches per call
    (b) api          harness.eval_vae(model=..., save=False) once per member, back to back, on a list of DEVICE-resident batches
                     (this favours (b)).  Above --api-members members (default 8) it is timed on that many and scaled to G
    (c) plain        EnsembleEvaluator on G Reg_VAE at the same N, M, G and d in the same process: the time per member x row x pass
                     the family's kernel is set against (per tile: both calls walk the same tile table)
The three alternate in blocks; medians of five blocks with their spread (min, max).  One JSON line per case, appended to --out;
--notes writes the table of the lines of this run and the two conditions (a) < (b) at every G, (c) within the spread
profiles/ensemble_eval_notes.md reports.  Warm-up: all three run once at the timed shape before the first block."""
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
FAMILIES = {  # name: (evaluator, model factory (d) -> model, vae_type of the api path)
    "Reg_VAE_mask": (vpc.MaskEnsembleEvaluator, lambda d: vpc.Reg_VAE_mask(d, 500, 10, L, TP, "bench", "kl_reg"), "reg_vae1_mask_augm"),
    "Reg_EDDI K=10": (vpc.EDDIEnsembleEvaluator, lambda d: vpc.Reg_EDDI(d, 500, 10, L, TP, "bench", "kl_reg"), "reg_EDDI1"),
    "Reg_EDDI K=20": (vpc.EDDIEnsembleEvaluator, lambda d: vpc.Reg_EDDI(d, 500, 20, L, TP, "bench", "kl_reg"), "reg_EDDI1"),
}


def stats(v, nd=1):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def timed_block(call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3, e0.elapsed_time(e1) / calls


def calls_for(call):
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return max(3, min(200, int(0.3 / max(time.perf_counter() - t0, 1e-6))))


def case(name, G, d, N, batch, M, api_members):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ev_cls, mk, vt = FAMILIES[name]
    g = torch.Generator().manual_seed(5)
    x = torch.rand(N, d, generator=g).to(dev)
    mask = (torch.rand(N, d, generator=g) < 0.7).to(dev)
    ev = ev_cls([mk(d).to(dev) for _ in range(G)], seeds=list(range(G)))
    plain = vpc.EnsembleEvaluator([vpc.Reg_VAE(d, 500, 10, L, TP, "bench", "kl_reg").to(dev) for _ in range(G)], seeds=list(range(G)))
    n_api = min(G, api_members)
    api_models = [mk(d).to(dev) for _ in range(n_api)]  # (their own models: eval_vae must not re-pack the ensemble's images)
    loader = [(x[lo:lo + batch], mask[lo:lo + batch]) for lo in range(0, N, batch)]
    ens_call = lambda: ev.evaluate(x, mask, batch, M, epoch=1000, beta=1.0)
    plain_call = lambda: plain.evaluate(x, mask, batch, M, epoch=1000, beta=1.0)

    def api_round():
        for m in api_models:
            H.eval_vae([(loader, "test")], 30, d, 500, 10, M, L, "bench", TP, "bench", vt, 1000, 1, 1, device=dev,
                       reg_type="kl_reg", model=m, save=False)

    calls, pcalls = calls_for(ens_call), calls_for(plain_call)
    api_round()
    torch.cuda.synchronize()
    ens_dev, ens_wall, pl_dev, api = [], [], [], []
    for _ in range(BLOCKS):
        w, dv = timed_block(ens_call, calls)
        ens_wall.append(w)
        ens_dev.append(dv)
        pl_dev.append(timed_block(plain_call, pcalls)[1])
        t0 = time.perf_counter()
        api_round()  # (eval_vae ends in .cpu(): synchronised)
        torch.cuda.synchronize()
        api.append((time.perf_counter() - t0) * 1e3 * G / n_api)
    ew, ed, pd, ap = stats(ens_wall, 3), stats(ens_dev, 3), stats(pl_dev, 3), stats(api, 1)
    tb = ev.tables(N, batch, M)[0]
    T = int(tb.tiles.shape[0])
    return dict(model=name, d=d, G=G, N=N, batch=batch, M=M, blocks=BLOCKS, calls_per_block=calls, tiles=T,
                batches=int(tb.batches.shape[0]), launches_per_call=ev.launches, ensemble_wall_ms=ew, ensemble_device_ms=ed,
                ns_per_member_row_pass=round(ed["median"] * 1e6 / (G * N * M), 3), us_per_tile=round(ed["median"] * 1e3 / (G * T), 4),
                plain_device_ms=pd, plain_ns_per_member_row_pass=round(pd["median"] * 1e6 / (G * N * M), 3),
                plain_us_per_tile=round(pd["median"] * 1e3 / (G * T), 4), family_over_plain=round(ed["median"] / pd["median"], 2),
                api_ms=ap, api_scaled_from=(n_api if n_api < G else None), api_ms_per_member=round(ap["median"] / G, 1),
                api_loader="device-resident batches", api_over_ensemble=round(ap["median"] / ew["median"], 1))


def notes(rows, path):
    out = ["<!-- table and conditions written by tools/bench_ensemble_eval_families.py from the lines of its run -->", "",
           "| model | d | G | (a) ms per call | ns per member x row x pass | launches | (b) ms | (b) / (a) | (c) plain ms | (a) / (c) |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        b = f"{r['api_ms']['median']:.0f}" + (f" (scaled from {r['api_scaled_from']})" if r["api_scaled_from"] else "")
        out.append(f"| {r['model']} | {r['d']} | {r['G']} | {r['ensemble_device_ms']['median']:.3f} | {r['ns_per_member_row_pass']:.2f} | "
                   f"{r['launches_per_call']} | {b} | {r['api_over_ensemble']:.0f} | {r['plain_device_ms']['median']:.3f} | "
                   f"{r['family_over_plain']:.2f} |")
    faster = all(r["ensemble_wall_ms"]["max"] < r["api_ms"]["min"] for r in rows)
    out += ["", f"**Condition 1** (at every G measured the one-call evaluation is faster than G per-member calls, worst block of (a) "
                f"against best block of (b)): {'met' if faster else 'NOT met'}."]
    # the plain evaluator of this run against the blocks of profiles/ensemble_eval.jsonl (what ensemble_eval_notes.md reports)
    ref = {}
    with open(os.path.join(ROOT, "profiles", "ensemble_eval.jsonl")) as f:
        for r in map(json.loads, f):
            if r["model"] == "Reg_VAE":
                ref[(r["d"], r["G"], r["N"], r["batch"], r["M"])] = r["ensemble_device_ms"]
    parts, ok = [], True
    for r in rows:
        key = (r["d"], r["G"], r["N"], r["batch"], r["M"])
        if key not in ref:
            continue
        p, q = r["plain_device_ms"], ref[key]
        inside = p["min"] <= q["max"] and q["min"] <= p["max"]  # the two runs' min - max ranges overlap
        ok = ok and inside
        parts.append(f"G = {r['G']} beside {r['model']}: {p['median']:.3f} ms ({p['min']:.3f} - {p['max']:.3f}) against "
                     f"{q['median']:.3f} ({q['min']:.3f} - {q['max']:.3f}), {100 * (p['median'] / q['median'] - 1):+.1f} %")
    out += ["", "**Condition 2** (the plain evaluator of this run inside the min - max of the blocks `ensemble_eval_notes.md` "
                "reports, d = 12): " + "; ".join(parts) + f": {'met' if ok and parts else 'NOT met'}.", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", default="1,8,64")
    ap.add_argument("--d", default="12")
    ap.add_argument("--N", type=int, default=1600)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--M", type=int, default=50)
    ap.add_argument("--models", default=",".join(FAMILIES))
    ap.add_argument("--api-members", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_eval_families.jsonl"))
    ap.add_argument("--notes", default=None, help="write the table and the conditions of this run's lines here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble_eval_families.py measures on the GPU: no device found")
    ints = lambda s: [int(v) for v in s.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rows = []
    for name in a.models.split(","):
        for d in ints(a.d):
            for G in ints(a.G):
                rows.append(case(name, G, d, a.N, a.batch, a.M, a.api_members))
                line = json.dumps(rows[-1])
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    if a.notes:
        notes(rows, a.notes)


if __name__ == "__main__":
    main()
