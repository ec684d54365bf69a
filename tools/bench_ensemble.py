"""Ensemble step against the same work done one model after the other.

    python tools/bench_ensemble.py [--G 1,8,64,128] [--B 64,128] [--d 12,128] [--out profiles/ensemble.jsonl]

For every (G, B, d), Reg_VAE kl_reg, device draws and Adam included, eager:
    ensemble       us per EnsembleTrainer.step (G members, one pair of launches), in both workgroup orders of the step launch
                   (order 0: member-major; order 1: all tiles of a member on one XCD), and us per member-step
    sequential     the parent's way: G stand-alone FusedTrainer.step calls back to back on one stream
    single_GB      the single-model step at G x B rows (the physical analogue: the same rows as one model's batch)
    enqueue_us     host time to issue one ensemble step (no sync): what the eager step costs when the GPU is not the limit
The three forms alternate in blocks; medians of five blocks with their spread (min, max), the convention of
profiles/fp32_issue_trim_notes.md.  One JSON line per case, appended to --out."""
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


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) / n * 1e6, (t1 - t0) / n * 1e6


def stats(v):
    return dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))


def case(G, B, d, steps):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mk = lambda: vpc.Reg_VAE(d, 500, 10, 10, TP, "bench", "kl_reg").to(dev)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(G, B, d, generator=g).to(dev)
    mask = (torch.rand(G, B, d, generator=g) < 0.7).to(dev)
    alphas = [0.5 + 0.4 * i / max(1, G - 1) for i in range(G)]
    ens = vpc.EnsembleTrainer([mk() for _ in range(G)], seeds=list(range(G)))
    seq = [vpc.FusedTrainer(mk(), seed=i) for i in range(G)]
    big = vpc.FusedTrainer(mk(), seed=0)
    xb, mb = x.reshape(G * B, d), mask.reshape(G * B, d)

    def ens_step():
        ens.step(x, mask, alpha=alphas)

    def seq_round():
        for i, tr in enumerate(seq):
            tr.step(x[i], mask[i], alpha=alphas[i])

    def big_step():
        big.step(xb, mb, alpha=0.7)

    rounds = max(3, steps // G)  # a sequential round is G steps
    for order in (0, 1):
        ens.order = order
        for _ in range(20):
            ens_step()
    for _ in range(3):
        seq_round()
    for _ in range(20):
        big_step()
    res = {"ens0": [], "ens1": [], "seq": [], "big": [], "enq0": [], "enq1": []}
    for _ in range(BLOCKS):
        for order in (0, 1):
            ens.order = order
            t, enq = timed(ens_step, steps)
            res[f"ens{order}"].append(t)
            res[f"enq{order}"].append(enq)
        res["seq"].append(timed(seq_round, rounds)[0])
        res["big"].append(timed(big_step, steps)[0])
    e0, e1, sq = stats(res["ens0"]), stats(res["ens1"]), stats(res["seq"])
    best = min(e0["median"], e1["median"])
    return dict(G=G, B=B, d=d, model="Reg_VAE kl_reg", steps_per_block=steps, blocks=BLOCKS,
                ensemble_us={"order0": e0, "order1": e1}, enqueue_us={"order0": stats(res["enq0"]), "order1": stats(res["enq1"])},
                member_step_us=round(best / G, 2), sequential_us=sq, sequential_member_step_us=round(sq["median"] / G, 2),
                single_GB_rows=G * B, single_GB_us=stats(res["big"]), single_GB_launch=big.dominant_launch(),
                sequential_over_ensemble=round(sq["median"] / best, 2),
                ensemble_in_sequential_steps=round(best / (sq["median"] / G), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", default="1,8,64,128")
    ap.add_argument("--B", default="64,128")
    ap.add_argument("--d", default="12,128")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble.jsonl"))
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for d in ints(a.d):
        for B in ints(a.B):
            for G in ints(a.G):
                line = json.dumps(case(G, B, d, a.steps))
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
