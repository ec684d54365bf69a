"""Ensemble step of the mask-augmented and point-net members against the same work done one model after the other.

    python tools/bench_ensemble_families.py [--G 1,8,64] [--B 64] [--d 12] [--K 10,20] [--out profiles/ensemble_families.jsonl]

Per family - "mask": Reg_VAE_mask kl_reg; "eddi": Reg_EDDI kl_reg at every K - and (G, B, d), device draws and Adam
included, eager:
    ensemble       us per MaskEnsembleTrainer / EDDIEnsembleTrainer step (G members, one pair of launches) in the trainer's
                   own workgroup order, and us per member-step
    sequential     G stand-alone FusedTrainer / EDDITrainer steps back to back on one stream, each on its small-batch path
    enqueue_us     host time to issue one ensemble step (no sync)
    kernel_us      the ensemble's two launches bracketed by events: the step kernel and the tail
The forms alternate in blocks; medians of five blocks with their spread (min, max), as tools/bench_ensemble.py.  One JSON line
per case, appended to --out."""
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


def kernel_times(ens, step, n=50):
    """Median us of the ensemble's two launches, each between its own pair of events."""
    pairs = {"step": [], "tail": []}

    def bracket(name, fn):
        def run(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(*a, **kw)
            e1.record()
            pairs[name].append((e0, e1))
        return run

    ens._launch_step, ens._launch_tail = bracket("step", ens._launch_step), bracket("tail", ens._launch_tail)
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    del ens._launch_step, ens._launch_tail  # (the instance attributes: the class's methods are back)
    return {k: round(statistics.median(a.elapsed_time(b) * 1e3 for a, b in v), 2) for k, v in pairs.items()}


def case(family, G, B, d, K, steps):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if family == "mask":
        mk = lambda: vpc.Reg_VAE_mask(d, 500, 10, 10, TP, "bench", "kl_reg").to(dev)
        ens_cls, solo_cls = vpc.MaskEnsembleTrainer, vpc.FusedTrainer
    else:
        mk = lambda: vpc.Reg_EDDI(d, 500, K, 10, TP, "bench", "kl_reg").to(dev)
        ens_cls, solo_cls = vpc.EDDIEnsembleTrainer, vpc.EDDITrainer
    g = torch.Generator().manual_seed(5)
    x = torch.rand(G, B, d, generator=g).to(dev)
    mask = (torch.rand(G, B, d, generator=g) < 0.7).to(dev)
    alphas = [0.5 + 0.4 * i / max(1, G - 1) for i in range(G)]
    ens = ens_cls([mk() for _ in range(G)], seeds=list(range(G)))
    seq = [solo_cls(mk(), seed=i) for i in range(G)]

    def ens_step():
        ens.step(x, mask, alpha=alphas)

    def seq_round():
        for i, tr in enumerate(seq):
            tr.step(x[i], mask[i], alpha=alphas[i])

    rounds = max(3, steps // G)  # a sequential round is G steps
    for _ in range(20):
        ens_step()
    for _ in range(3):
        seq_round()
    small = all((tr.dominant_launch() == "step_small") if family == "mask" else (tr.last_path == "small") for tr in seq)
    res = {"ens": [], "enq": [], "seq": []}
    for _ in range(BLOCKS):
        t, enq = timed(ens_step, steps)
        res["ens"].append(t)
        res["enq"].append(enq)
        res["seq"].append(timed(seq_round, rounds)[0])
    e, sq = stats(res["ens"]), stats(res["seq"])
    return dict(family=family, model="Reg_VAE_mask kl_reg" if family == "mask" else f"Reg_EDDI kl_reg K={K}", G=G, B=B, d=d,
                K=K if family == "eddi" else None, steps_per_block=steps, blocks=BLOCKS, order=ens.order, ensemble_us=e,
                enqueue_us=stats(res["enq"]), member_step_us=round(e["median"] / G, 2), sequential_us=sq,
                sequential_member_step_us=round(sq["median"] / G, 2), sequential_on_small_path=small,
                sequential_over_ensemble=round(sq["median"] / e["median"], 2), kernel_us=kernel_times(ens, ens_step))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", default="1,8,64")
    ap.add_argument("--B", default="64")
    ap.add_argument("--d", default="12")
    ap.add_argument("--K", default="10,20")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_families.jsonl"))
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for family, Ks in (("mask", [0]), ("eddi", ints(a.K))):
        for K in Ks:
            for d in ints(a.d):
                for B in ints(a.B):
                    for G in ints(a.G):
                        line = json.dumps(case(family, G, B, d, K, a.steps))
                        print(line, flush=True)
                        with open(a.out, "a") as f:
                            f.write(line + "\n")


if __name__ == "__main__":
    main()
