"""Ensemble step of G VAEFlow / REG_VAEFlow members against the same work done one model after the other.

    python tools/bench_flow_ensemble.py [--G 1,2,3,8,64] [--kinds reg,van] [--out profiles/flow_ensemble.jsonl]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_flow_ensemble.py --kernel-stats [--G 64] [--kinds reg]

At the wine shape (d = 12, hid 500, B = 64), device draws and Adam included, eager, one process:
    ensemble       us per FlowEnsembleTrainer step (G members, 22 launches) at the trainer's own workgroup order, and us per
                   member-step
    sequential     G stand-alone FlowTrainer steps back to back on one stream, each on its few-row path (VPC_FLOW_SMALL=128)
    enqueue_us     host time to issue one ensemble step (no sync)
    orders         at G >= 8: the ensemble step under both workgroup orders (0 member-major, 1 a member on one XCD)
The two forms alternate in blocks; medians of five blocks with their spread (min, max), as tools/bench_miw_ensemble.py.
One JSON line per case, appended to --out.  --kernel-stats runs ensemble steps only (no timing, nothing written): the command to
profile in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["VPC_FLOW_SMALL"] = "128"  # the stand-alone trainers on their few-row path
import vpc_amd as vpc  # noqa: E402
from vpc_amd import flow_ensemble as E  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
BLOCKS = 5
B, D, HID = 64, 12, 500


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
    cls = vpc.REG_VAEFlow if kind == "reg" else vpc.VAEFlow
    torch.manual_seed(0)
    return [cls(D, HID, 10, 10, TP).cuda() for _ in range(G)]


def batch():
    g = torch.Generator().manual_seed(1)
    return torch.rand(B, D, generator=g).cuda(), (torch.rand(B, D, generator=g) < 0.7).cuda().float()


def case(kind, G):
    x, mask = batch()
    ens = E.FlowEnsembleTrainer(build(kind, G), lr=1e-3)
    solo = [vpc.FlowTrainer(m, lr=1e-3, seed=i) for i, m in enumerate(build(kind, G))]
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
    rec = dict(kind=kind, G=G, B=B, d=D, hid=HID, order=ens.order,
               workspace_MB=round(E.workspace_floats(G, (2 if kind == "reg" else 1) * B, B, D, HID, kind == "reg") * 4 / 1e6, 1),
               ensemble_us=stats(te), sequential_us=stats(ts), enqueue_us=stats(tq),
               per_member_us=round(statistics.median(te) / G, 2), speedup=round(statistics.median(ts) / statistics.median(te), 2),
               worst_ensemble_beats_best_sequential=max(te) < min(ts))
    del solo
    if G >= 8:
        orders = {}
        for _ in range(BLOCKS):  # the two orders alternate on one trainer: same bits, so the state does not matter
            for order in (0, 1):
                ens.order = order
                run_ens()
                orders.setdefault(order, []).append(timed(run_ens, n_ens)[0])
        rec["orders"] = {str(o): stats(v) for o, v in orders.items()}
    return rec


def kernel_stats(kind, G, steps=100):
    x, mask = batch()
    ens = E.FlowEnsembleTrainer(build(kind, G), lr=1e-3)
    for _ in range(steps):
        ens.step(x, mask, alpha=0.5, p_missingness=30)
    torch.cuda.synchronize()
    print(f"{steps} ensemble steps, {kind}, G = {G}, order {ens.order}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", default="1,2,3,8,64")
    ap.add_argument("--kinds", default="reg,van")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_ensemble.jsonl"))
    ap.add_argument("--kernel-stats", action="store_true")
    a = ap.parse_args()
    Gs = [int(v) for v in a.G.split(",")]
    if a.kernel_stats:
        kernel_stats(a.kinds.split(",")[0], Gs[-1])
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for kind in a.kinds.split(","):
        for G in Gs:
            rec = case(kind, G)
            print(json.dumps(rec), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
