"""The acquisition loop of a mask-augmented / point-net sweep against the loop it replaces and against the plain sweep's.

    python tools/bench_ensemble_active_families.py [--G 1,8,64] [--out profiles/ensemble_active_families.jsonl]
                                                   [--notes profiles/ensemble_active_families_notes.md]

Shape: d = 12, n = 160, M = 50, one repeat, all 11 steps, device draws, one test set shared by the members.  Cases: Reg_VAE_mask,
Reg_EDDI at emb_dim 10 and 20, each at every G.  Three arms per case, alternating in five blocks (the protocol of
tools/bench_ensemble_active.py: medians with min - max over the blocks, one synchronise per block, both sides warmed up at the
timed shape, no gc.collect()):
    (a) family    one MaskEnsembleAcquirer / EDDIEnsembleAcquirer.run (keep_im=True): wall time of a block of calls, and device
                  time by HIP events around them
    (b) api       active_learning_func(model=m, save=False) once per member, back to back: what a sweep of these families ran
                  before.  Above --api-members members (default 8) it is timed on that many and scaled to G (`api_scaled_from`)
    (c) plain     one EnsembleAcquirer.run on G Reg_VAE at the same shape, in the same process: the yardstick (a) is compared with
One JSON line per case, appended to --out; the table between the two marker lines of --notes is rewritten from the lines of
this run (the prose around it is kept)."""
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
L, D, N, M = 10, 12, 160, 50
CASES = {"Reg_VAE_mask": ("mask", 0, "reg_vae1_mask_augm"), "Reg_EDDI K=10": ("eddi", 10, "reg_EDDI1"),
         "Reg_EDDI K=20": ("eddi", 20, "reg_EDDI1")}
BEGIN, END = "<!-- table: tools/bench_ensemble_active_families.py -->", "<!-- end of table -->"


def stats(v, nd=3):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def case(name, G, api_members):
    family, K, vt = CASES[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mk = (lambda: vpc.Reg_VAE_mask(D, 500, 10, L, TP, "bench", "kl_reg").to(dev)) if family == "mask" else \
        (lambda: vpc.Reg_EDDI(D, 500, K, L, TP, "bench", "kl_reg").to(dev))
    g = torch.Generator().manual_seed(5)
    x_cpu = torch.rand(N, D, generator=g)
    tmask = torch.rand(N, D, generator=g) < 0.7
    x = x_cpu.to(dev)
    cls = vpc.MaskEnsembleAcquirer if family == "mask" else vpc.EDDIEnsembleAcquirer
    acq = cls([mk() for _ in range(G)], seeds=list(range(G)))
    plain = vpc.EnsembleAcquirer([vpc.Reg_VAE(D, 500, 10, L, TP, "bench", "kl_reg").to(dev) for _ in range(G)], seeds=list(range(G)))
    n_api = min(G, api_members)
    api_models = [mk() for _ in range(n_api)]  # (their own models: the API path must not re-pack the ensemble's images)
    steps = D - 1

    def api_round():
        for m in api_models:
            vpc.active_learning_func(None, x_cpu, tmask, 30, D, 500, K or 10, M, L, "bench", TP, "bench", vt, 1000, 1, 1, device=dev,
                                     reg_type="kl_reg", Repeat=1, model=m, save=False, max_steps=steps)

    def block(a, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(calls):
            a.run(x, M, repeats=1, max_steps=steps, keep_im=True)
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3, e0.elapsed_time(e1) / calls

    # warm-up at the timed shape, and the number of calls that makes a block ~0.3 s
    block(acq, 1), block(plain, 1)
    calls = max(2, min(50, int(0.3 / max(block(acq, 1)[0] * 1e-3, 1e-6))))
    api_round()
    torch.cuda.synchronize()
    fam_wall, fam_dev, api, pl_wall = [], [], [], []
    for _ in range(BLOCKS):
        w, dv = block(acq, calls)
        fam_wall.append(w), fam_dev.append(dv)
        t0 = time.perf_counter()
        api_round()
        torch.cuda.synchronize()
        api.append((time.perf_counter() - t0) * 1e3 * G / n_api)
        pl_wall.append(block(plain, calls)[0])
    fw, fd, ap, pw = stats(fam_wall), stats(fam_dev), stats(api, 1), stats(pl_wall)
    return dict(case=name, d=D, G=G, n=N, M=M, steps=steps, repeats=1, keep_im=True, blocks=BLOCKS, calls_per_block=calls,
                launches_per_step=acq.launches_per_step, launches_per_run=acq.launches,
                family_wall_ms=fw, family_device_ms=fd, family_us_per_member_step=round(fw["median"] * 1e3 / (G * steps), 2),
                api_ms=ap, api_scaled_from=(n_api if n_api < G else None), api_ms_per_member=round(ap["median"] / G, 1),
                api_best_over_family_worst=round(ap["min"] / fw["max"], 1), plain_wall_ms=pw,
                family_over_plain=round(fw["median"] / pw["median"], 3))


def table(lines):
    rows = ["| case | G | (a) ms per run (min - max) | us per member-step | launches per step | (b) ms (min - max) | (b) ms per member | "
            "best (b) / worst (a) | (c) plain ms per run (min - max) | (a) / (c) |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in lines:
        a, b, c = r["family_wall_ms"], r["api_ms"], r["plain_wall_ms"]
        scaled = f" (scaled from {r['api_scaled_from']})" if r["api_scaled_from"] else ""
        rows.append(f"| {r['case']} | {r['G']} | {a['median']} ({a['min']} - {a['max']}) | {r['family_us_per_member_step']} | "
                    f"{r['launches_per_step']} | {b['median']} ({b['min']} - {b['max']}){scaled} | {r['api_ms_per_member']} | "
                    f"{r['api_best_over_family_worst']} | {c['median']} ({c['min']} - {c['max']}) | {r['family_over_plain']} |")
    return "\n".join(rows)


def write_table(path, lines):
    text = open(path).read() if os.path.exists(path) else f"# Ensemble acquisition for the mask-augmented and point-net sweeps\n\n{BEGIN}\n{END}\n"
    if BEGIN not in text or END not in text:
        raise SystemExit(f"{path}: the table's marker lines are missing")
    head, rest = text.split(BEGIN, 1)
    with open(path, "w") as f:
        f.write(head + BEGIN + "\n" + table(lines) + "\n" + END + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", default="1,8,64")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--api-members", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_active_families.jsonl"))
    ap.add_argument("--notes", default=os.path.join(ROOT, "profiles", "ensemble_active_families_notes.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble_active_families.py measures on the GPU: no device found")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lines = []
    for name in a.cases.split(","):
        for G in [int(v) for v in a.G.split(",")]:
            lines.append(case(name, G, a.api_members))
            print(json.dumps(lines[-1]), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(lines[-1]) + "\n")
    write_table(a.notes, lines)


if __name__ == "__main__":
    main()
