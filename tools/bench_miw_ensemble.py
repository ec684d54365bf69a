"""Ensemble step of G MIWAE / Reg_MIWAE members against the same work done one model after the other.

    python tools/bench_miw_ensemble.py [--G 1,8,64] [--kinds reg,van] [--out profiles/miw_ensemble.jsonl] [--no-candidates]

At the wine shape (B = 64, S = 20, d = 12, L = 10), device draws and Adam included, eager:
    ensemble       us per MIWEnsembleTrainer step (G members, seven kernels) at the trainer's own (rb, blocks_per_member, order),
                   and us per member-step
    sequential     G stand-alone MIWTrainer steps back to back on one stream, each on its small-batch path (VPC_MIW_SMALL)
    enqueue_us     host time to issue one ensemble step (no sync)
    candidates     the ensemble step at every (rb, blocks_per_member, order) behind the default rule: medians of three blocks
The two forms alternate in blocks; medians of five blocks with their spread (min, max), as tools/bench_ensemble_families.py.
One JSON line per case, appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["VPC_MIW_SMALL"] = str(1 << 20)  # the stand-alone trainers on their small-batch path
import vpc_amd as vpc  # noqa: E402
from vpc_amd import miw_ensemble as E  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
BLOCKS = 5
B, S, D, LD = 64, 20, 12, 10


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


def build(kind, G):
    cls = vpc.Reg_MIWAE if kind == "reg" else vpc.MIWAE
    torch.manual_seed(0)
    return [cls(D, 500, 10, LD, TP, S, 1).cuda() for _ in range(G)]


def case(kind, G, candidates):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, D, generator=g).cuda()
    mask = (torch.rand(B, D, generator=g) < 0.7).cuda()
    ens = E.MIWEnsembleTrainer(build(kind, G), lr=1e-3)
    solo = [vpc.MIWTrainer(m, lr=1e-3, seed=i) for i, m in enumerate(build(kind, G))]
    alphas = [0.1 + 0.8 * i / max(G - 1, 1) for i in range(G)]

    def run_ens():
        ens.step(x, mask, alpha=alphas, p_missingness=30)

    def run_seq():
        for tr, a in zip(solo, alphas):
            tr.step(x, mask, alpha=a, p_missingness=30)

    n_ens, n_seq = max(20, 400 // G), max(3, 200 // G)
    for _ in range(3):
        run_ens()
        run_seq()
    assert all(tr.last_path == "small" for tr in solo)
    te, ts, tq = [], [], []
    for _ in range(BLOCKS):
        t, q = timed(run_ens, n_ens)
        te.append(t)
        tq.append(q)
        ts.append(timed(run_seq, n_seq)[0])
    P = 2 if kind == "reg" else 1
    rec = dict(kind=kind, G=G, B=B, S=S, d=D, L=LD, rb=ens.rb, blocks_per_member=ens.blocks_per_member, order=ens.order,
               part_MB=round(E.partial_floats(G, ens.blocks_per_member, ens.n) * 4 / 1e6, 1),
               solo_rb=vpc.miwae.small_rows_per_workgroup(P * B, S), ensemble_us=stats(te), sequential_us=stats(ts),
               enqueue_us=stats(tq), per_member_us=round(statistics.median(te) / G, 2),
               speedup=round(statistics.median(ts) / statistics.median(te), 2),
               worst_ensemble_beats_best_sequential=max(te) < min(ts))
    del solo
    if candidates:
        units = lambda rb: -(-P * B // rb)
        c = max(1, -(-ens.n_cu // G))
        cand = []
        for rb in (1, 2, 4):
            for blocks in sorted({min(k, units(rb)) for k in (c, 2 * c, 4 * c, 8 * c, units(rb))}):
                if E.partial_floats(G, blocks, ens.n) > E.PART_MAX_FLOATS:
                    continue
                for order in (0, 1):
                    e2 = E.MIWEnsembleTrainer(build(kind, G), lr=1e-3, rb=rb, blocks_per_member=blocks)
                    e2.order = order
                    step = lambda: e2.step(x, mask, alpha=alphas, p_missingness=30)
                    for _ in range(3):
                        step()
                    t = [timed(step, n_ens)[0] for _ in range(3)]
                    cand.append(dict(rb=rb, blocks=blocks, order=order, us=round(statistics.median(t), 1)))
                    del e2
        rec["candidates"] = cand
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", default="1,8,64")
    ap.add_argument("--kinds", default="reg,van")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "miw_ensemble.jsonl"))
    ap.add_argument("--no-candidates", action="store_true")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for kind in a.kinds.split(","):
        for G in (int(v) for v in a.G.split(",")):
            rec = case(kind, G, not a.no_candidates)
            print(json.dumps(rec), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
