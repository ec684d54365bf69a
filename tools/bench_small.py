"""Small-batch / strong-scaling timings of the fused Reg_VAE step.

    python tools/bench_small.py [--batches 64,256,1024,8192,16384,32768] [--steps 300] [--graph]

For every batch size: us / step of FusedTrainer.step with the 16-row N-split kernel forced (VPC_TILE=16: csrc/vpc_small.hip,
one launch for the whole step), with the throughput shape forced (VPC_TILE=128: 128-row tiles, 8
waves, both passes looped in the workgroup) and with the small-batch shape forced (VPC_TILE=64: 64-row tiles, one wave
per SIMD, passes spread over blockIdx.y), device-side draws and Adam included, plus per-kernel HIP-event times.
Prints one JSON line per (B, shape).

    python tools/bench_small.py --mask-augm [--shapes 12x64,64x64,12x1024] [--steps 300] [--out profiles/small_augm.jsonl]

The mask-augmented classes (Reg_VAE_mask, vanilla_VAE_mask) instead: per (d, B), FusedTrainer.step (eager, device draws, Adam
included) on the N-split kernel against the row-tiled path (VPC_STEP_SMALL=0) in ONE process, five alternating timed blocks
per path, the median of each, and the C ABI launches of one step.  One JSON line per (class, d, B), appended to --out."""
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


def run(B, d, tile, steps, graph):
    os.environ["VPC_TILE"] = tile
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = vpc.Reg_VAE(d, 500, 10, 10, {"batch_size": B, "patience": 1}, "bench", "kl_reg").to(dev)
    tr = vpc.FusedTrainer(m, seed=1)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, d, generator=g).to(dev)
    mask = (torch.rand(B, d, generator=g) < 0.7).to(dev)
    fn = tr.step_graph if graph else tr.step
    for _ in range(60):
        fn(x, mask, alpha=1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn(x, mask, alpha=1.0)
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / steps * 1e6
    kern = {}
    if not graph:
        tr.timers, tr.timer_every = {}, 1
        for _ in range(20):
            tr.step(x, mask, alpha=1.0)
        torch.cuda.synchronize()
        kern = {k: round(statistics.median(a.elapsed_time(b) for a, b in v) * 1e3, 1) for k, v in tr.timers.items()}
    return dict(B=B, d=d, tile=int(tile), graph=graph, us_per_step=round(us, 1), blocks=tr.last_blocks, kernels_us=kern,
                loss=tr.loss_value())


class _Launches:
    """Stands in for the loaded library during one step: counts the vpc_* entries fetched that launch a kernel."""
    HOST_ONLY = ("vpc_step_small_max_rows", "vpc_step_fused_applicable", "vpc_step_workspace_floats")

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        if name.startswith("vpc_") and name not in self.HOST_ONLY:
            self.names.append(name)
        return getattr(self.real, name)


def run_mask_augm(cls, d, B, steps, blocks=5):
    from vpc_amd import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, d, generator=g).to(dev)
    mask = (torch.rand(B, d, generator=g) < 0.7).to(dev)
    paths = {"step_small": None, "row_tiled": "0"}  # value of VPC_STEP_SMALL
    trs, times, launches, dom = {}, {k: [] for k in paths}, {}, {}

    def select(env):
        os.environ.pop("VPC_STEP_SMALL", None)
        if env is not None:
            os.environ["VPC_STEP_SMALL"] = env

    for name, env in paths.items():
        select(env)
        torch.manual_seed(0)
        tp = {"batch_size": B, "patience": 1}
        m = (vpc.Reg_VAE_mask(d, 500, 10, 10, tp, "bench", "kl_reg") if cls == "Reg_VAE_mask" else
             vpc.vanilla_VAE_mask(d, 500, 10, 10, tp, "bench")).to(dev)
        tr = trs[name] = vpc.FusedTrainer(m, seed=1)
        for _ in range(60):
            tr.step(x, mask, alpha=1.0)
        rec = _Launches(_lib.lib())
        _lib._lib = rec
        tr.step(x, mask, alpha=1.0)
        _lib._lib = rec.real
        launches[name], dom[name] = rec.names, tr.dominant_launch()
    for _ in range(blocks):
        for name, env in paths.items():
            select(env)
            tr = trs[name]
            for _ in range(20):
                tr.step(x, mask, alpha=1.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(x, mask, alpha=1.0)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e6)
    select(None)
    out = dict(model=cls, d=d, B=B, steps=steps, blocks=blocks)
    for name in paths:
        out[name] = dict(us_per_step=round(statistics.median(times[name]), 1), all_us=[round(t, 1) for t in times[name]],
                         launches=len(launches[name]), entries=launches[name], dominant=dom[name])
    out["speedup"] = round(out["row_tiled"]["us_per_step"] / out["step_small"]["us_per_step"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256,1024,8192,16384,32768")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--mask-augm", action="store_true")
    ap.add_argument("--shapes", default="12x64,64x64,12x1024", help="--mask-augm: d x B pairs")
    ap.add_argument("--out", default=None, help="--mask-augm: also append the JSON lines to this file")
    a = ap.parse_args()
    if a.mask_augm:
        for cls in ("Reg_VAE_mask", "vanilla_VAE_mask"):
            for d, B in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
                line = json.dumps(run_mask_augm(cls, d, B, a.steps))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        return
    for B in [int(v) for v in a.batches.split(",")]:
        for tile in ("128", "64", "16"):  # 16 = the N-split kernel (csrc/vpc_small.hip)
            print(json.dumps(run(B, a.dim, tile, a.steps, False)), flush=True)
            if a.graph:
                print(json.dumps(run(B, a.dim, tile, a.steps, True)), flush=True)


if __name__ == "__main__":
    main()
