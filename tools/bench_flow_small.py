"""Small-batch flow step (the few-row layer ops of csrc/vpc_rows.hip) against the launch chain of FlowTrainer.step, in one
process:

  * shapes d = 12, hid = 500, REG_VAEFlow and VAEFlow at B in {16, 64}, VAEFlow also at B = 128 (R = P * B <= 128 stacked rows),
  * variants: the chain (VPC_FLOW_SMALL=0) and the small path (VPC_FLOW_SMALL=128) on the SAME trainer,
  * five rounds; a round times one block of every variant in turn (alternating), a block is `steps` eager steps - device
    draws and Adam included - between two device synchronisations, after a warm-up of the variant,
  * one JSON line per (kind, B, variant): the five block times in us per step, their median, min and max; then one line
    per (kind, B) saying whether the small path's worst block beats the chain's best block.

    python tools/bench_flow_small.py [--out profiles/flow_small.jsonl] [--cells reg:16,reg:64,van:16,van:64,van:128] [--rounds 5]
    python tools/bench_flow_small.py --trace STEPS   # STEPS small-path steps of REG_VAEFlow at B = 64 alone (for a kernel trace)
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
from vpc_amd import flow  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
D, HID = 12, 500
VARIANTS = [("chain", "0"), ("small", str(flow.SMALL_MAX_ROWS))]
STEPS = 2000  # a few tenths of a second per block at the step times of this family


def make(kind, B):
    g = torch.Generator().manual_seed(0)
    x, m = torch.rand(B, D, generator=g).cuda(), (torch.rand(B, D, generator=g) < 0.5).cuda()
    torch.manual_seed(0)
    model = (vpc_amd.REG_VAEFlow if kind == "reg" else vpc_amd.VAEFlow)(D, HID, 10, 10, TP).cuda()
    return vpc_amd.FlowTrainer(model, lr=1e-3, seed=1), x, m


def block(tr, x, m, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(x, m, alpha=0.5, p_missingness=30)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def bench(kind, B, rounds, emit):
    tr, x, m = make(kind, B)
    times = {name: [] for name, _ in VARIANTS}
    for name, env in VARIANTS:  # every variant's code objects, workspaces and first launches
        os.environ["VPC_FLOW_SMALL"] = env
        block(tr, x, m, 20)
        assert tr.last_path == name
    for _ in range(rounds):
        for name, env in VARIANTS:
            os.environ["VPC_FLOW_SMALL"] = env
            block(tr, x, m, STEPS // 20)
            times[name].append(block(tr, x, m, STEPS))
    R = (2 if kind == "reg" else 1) * B
    for name, env in VARIANTS:
        t = times[name]
        emit(dict(name=f"{name}_{kind}_b{B}", kind=kind, B=B, d=D, hid=HID, stacked_rows=R, variant=name, VPC_FLOW_SMALL=env,
                  steps_per_block=STEPS, us_per_step_blocks=[round(v, 2) for v in t],
                  us_median=round(statistics.median(t), 2), us_min=round(min(t), 2), us_max=round(max(t), 2)))
    emit(dict(name=f"summary_{kind}_b{B}", kind=kind, B=B, stacked_rows=R, small_worst_us=round(max(times["small"]), 2),
              chain_best_us=round(min(times["chain"]), 2),
              small_worst_beats_chain_best=max(times["small"]) < min(times["chain"]), loss=tr.loss_value()))


def trace(steps):
    tr, x, m = make("reg", 64)
    os.environ.setdefault("VPC_FLOW_SMALL", str(flow.SMALL_MAX_ROWS))  # (VPC_FLOW_SMALL=0 traces the chain)
    for _ in range(steps):
        tr.step(x, m, alpha=0.5, p_missingness=30)
    torch.cuda.synchronize()
    print(json.dumps(dict(name="trace", path=tr.last_path, steps=steps, loss=tr.loss_value())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cells", default="reg:16,reg:64,van:16,van:64,van:128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow_small.py measures on the GPU: no device found")
    if a.trace:
        return trace(a.trace)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for cell in a.cells.split(","):
        kind, B = cell.split(":")
        bench(kind, int(B), a.rounds, emit)


if __name__ == "__main__":
    main()
