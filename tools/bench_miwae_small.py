"""Small-batch MIWAE step (csrc/vpc_miw_small.hip) against the launch chain of MIWTrainer.step, in one process:

  * shapes d = 12, L = 10, S = 20, B in {16, 64, 256, 1 024, 4 096}, Reg_MIWAE and MIWAE,
  * variants: the chain (VPC_MIW_SMALL=0) and the small path with RB = 1, 2, 4 data rows per workgroup,
  * five rounds; a round times one block of every variant in turn (alternating), a block is `steps` eager steps - device
    draws and Adam included - between two device synchronisations, after a warm-up of the variant,
  * one JSON line per (kind, B, variant): the five block times in us per step, their median, min and max; then one line
    per (kind, B) with the best RB and whether the small path's worst block beats the chain's best block.

    python tools/bench_miwae_small.py [--out profiles/miwae_small.jsonl] [--batches 16,64] [--kinds reg,van] [--rounds 5]
    python tools/bench_miwae_small.py --trace STEPS   # STEPS small-path steps at B = 64 alone (for a kernel trace)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vpc_amd  # noqa: E402
from vpc_amd import miwae  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
D, LAT, S = 12, 10, 20
ALL_ROWS = str(1 << 30)
VARIANTS = [("chain", None), ("small_rb1", 1), ("small_rb2", 2), ("small_rb4", 4)]


def steps_for(B):
    """Steps of a timed block: a few tenths of a second at the step times of this family."""
    return 2000 if B <= 256 else 600 if B <= 1024 else 200


def make(kind, B):
    g = torch.Generator().manual_seed(0)
    x, m = torch.rand(B, D, generator=g).cuda(), (torch.rand(B, D, generator=g) < 0.5).cuda()
    torch.manual_seed(0)
    model = (vpc_amd.Reg_MIWAE if kind == "reg" else vpc_amd.MIWAE)(D, 500, 10, LAT, TP, S, 1).cuda()
    return vpc_amd.MIWTrainer(model, lr=1e-3, seed=1), x, m


def select(tr, rb):
    os.environ["VPC_MIW_SMALL"] = "0" if rb is None else ALL_ROWS
    tr.small_rb = rb


def block(tr, x, m, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(x, m, alpha=0.5, p_missingness=30)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def bench(kind, B, rounds, emit):
    tr, x, m = make(kind, B)
    steps = steps_for(B)
    times = {name: [] for name, _ in VARIANTS}
    for name, rb in VARIANTS:  # every variant's code objects, workspaces and first launches
        select(tr, rb)
        block(tr, x, m, 20)
        assert tr.last_path == ("chain" if rb is None else "small")
    for _ in range(rounds):
        for name, rb in VARIANTS:
            select(tr, rb)
            block(tr, x, m, max(5, steps // 20))
            times[name].append(block(tr, x, m, steps))
    P = 2 if kind == "reg" else 1
    for name, rb in VARIANTS:
        t = times[name]
        emit(dict(name=f"{name}_{kind}_b{B}", kind=kind, B=B, S=S, d=D, L=LAT, decoder_rows=P * B * S, variant=name,
                  steps_per_block=steps, us_per_step_blocks=[round(v, 2) for v in t],
                  us_median=round(statistics.median(t), 2), us_min=round(min(t), 2), us_max=round(max(t), 2)))
    best = min((n for n, rb in VARIANTS if rb), key=lambda n: statistics.median(times[n]))
    emit(dict(name=f"summary_{kind}_b{B}", kind=kind, B=B, decoder_rows=P * B * S, best_small=best,
              small_worst_us=round(max(times[best]), 2), chain_best_us=round(min(times["chain"]), 2),
              small_worst_beats_chain_best=max(times[best]) < min(times["chain"]), loss=tr.loss_value()))


def trace(steps):
    tr, x, m = make("reg", 64)
    os.environ.setdefault("VPC_MIW_SMALL", str(miwae.SMALL_ROWS_MEASURED))  # (VPC_MIW_SMALL=0 traces the chain)
    for _ in range(steps):
        tr.step(x, m, alpha=0.5, p_missingness=30)
    torch.cuda.synchronize()
    print(json.dumps(dict(name="trace", path=tr.last_path, steps=steps, loss=tr.loss_value())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="16,64,256,1024,4096")
    ap.add_argument("--kinds", default="reg,van")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_miwae_small.py measures on the GPU: no device found")
    if a.trace:
        return trace(a.trace)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for kind in a.kinds.split(","):
        for B in (int(b) for b in a.batches.split(",")):
            bench(kind, B, a.rounds, emit)


if __name__ == "__main__":
    main()
