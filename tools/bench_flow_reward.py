"""Config 5 reward of the flow models: one reward matrix at n = 256, M = 50, hid = 500 for d = 12 and d = 128, both
classes, medians of 5 blocks -> profiles/flow_reward.jsonl.

    python tools/bench_flow_reward.py [--out profiles/flow_reward.jsonl] [--once D]

  fused_ms     vpc.flow_reward_matrix (device draws), all candidates
  api_ms       the same quantity through the only route without it: the drop-in chaini_I/II_ratio_version API-path loop
               (evaluate.py:653-661, 4 encoder calls per candidate and sample), TIMED ON `api_candidates` CANDIDATES AND
               SCALED to d - 1
  cpu_ms       the float64 restatement (tests/flow_reward_oracle.py) on 16 threads, timed on `cpu_candidates` candidates
               and scaled to d - 1
  trunk_tflops GEMM-equivalent rate of the b-row trunk (layers 2 and 3 of 2 n (d-1) M rows) over the WHOLE fused call;
               the per-kernel rate is in profiles/flow_reward_kernel_stats.csv
--once D runs a single fused call at width D (the command profiled under rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vpc_amd as vpc  # noqa: E402

N, M, HID = 256, 50, 500
TP = {"batch_size": 64, "patience": 100}


def inputs(d, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, d, generator=g)
    mask = (torch.rand(N, d, generator=g) < 0.3).float()
    mask[:, -1] = 0
    im = torch.rand(M, N, d, generator=g)
    return x.cuda(), mask.cuda(), im.cuda()


def timed(fn, blocks=5, reps=1):
    out = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return statistics.median(out), out


def api_loop(model, x, mask, im, cands):
    for u in cands:
        loc = torch.where(mask[:, u] == 0)[0]
        tx = x.clone()
        acc = torch.zeros(len(loc), device=x.device)
        for m in range(M):
            tx[loc, u] = im[m, loc, u]
            acc += vpc.chaini_I_ratio_version(tx[loc], mask[loc], u, model)
            tx[loc, -1] = im[m, loc, -1]
            acc -= vpc.chaini_II_ratio_version(tx[loc], mask[loc], u, model)
    return acc / M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_reward.jsonl"))
    ap.add_argument("--once", type=int, default=0)
    a = ap.parse_args()
    torch.manual_seed(0)
    if a.once:
        model = vpc.REG_VAEFlow(a.once, HID, 10, 10, TP).cuda()
        x, mask, im = inputs(a.once)
        vpc.flow_reward_matrix(model, x, mask, im, seed=1)
        torch.cuda.synchronize()
        return
    import flow_reward_oracle as FR
    torch.set_num_threads(16)
    rows = []
    for d in (12, 128):
        for kind, cls in (("reg", vpc.REG_VAEFlow), ("van", vpc.VAEFlow)):
            model = cls(d, HID, 10, 10, TP).cuda()
            x, mask, im = inputs(d)
            fused = lambda: vpc.flow_reward_matrix(model, x, mask, im, seed=1)
            fused()
            f_ms, f_all = timed(fused, reps=3 if d == 12 else 1)
            cands = [0, d // 2]
            api_loop(model, x, mask, im, cands[:1])
            a_ms, _ = timed(lambda: api_loop(model, x, mask, im, cands), blocks=5 if d == 12 else 3)
            a_ms *= (d - 1) / len(cands)
            P = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
            eps = np.random.default_rng(0).standard_normal((1, M, 4, N, 10))  # candidate 0 only
            t0 = time.perf_counter()
            FR.reward_matrix(P, x.cpu().numpy(), mask.cpu().numpy(), im.cpu().numpy(), eps, candidates=[0])
            c_ms = (time.perf_counter() - t0) * 1e3 * (d - 1)
            flops = 2.0 * (2 * N * (d - 1) * M) * (HID * HID + 100 * HID)
            row = dict(what="flow_reward", kind=kind, n=N, d=d, M=M, hid=HID, chunk=vpc.active.flow_reward_chunk(N, d, HID, M),
                       fused_ms=round(f_ms, 3), fused_blocks_ms=[round(v, 3) for v in f_all], api_ms=round(a_ms, 1),
                       api_candidates=len(cands), api_scaled=True, cpu_ms=round(c_ms, 1), cpu_candidates=1, cpu_threads=16,
                       trunk_tflops=round(flops / (f_ms * 1e-3) / 1e12, 2), speedup_vs_api=round(a_ms / f_ms, 1))
            print(json.dumps(row), flush=True)
            rows.append(row)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
