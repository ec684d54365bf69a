"""eval_vae(engine="batched") (flow.FlowEvaluator, csrc/vpc_floweval.hip) against eval_vae(engine="chain") for the flow models, in
one process:

  * cells kind:d:M - REG_VAEFlow / VAEFlow at d = 12, M = 5 and M = 50, and one d = 128 cell; hid 500, N = 1600 rows in batches of
    64 (25 batches per pass), the loader's batches resident on the device, save=False,
  * variants: "chain" and "batched" (eval_vae end to end: the gathering of the passes, the launches, one .cpu()), and
    "evaluate" (FlowEvaluator.evaluate on the gathered arrays + .cpu(): the launches alone),
  * five rounds; a round times one block of every variant in turn (alternating); a block is `calls` calls between two device
    synchronisations, after a warm-up of the variant,
  * one JSON line per (cell, variant): the five block times in ms per call, their median, min and max, and the C ABI calls of
    one call; then one line per cell saying whether the batched engine's worst block beats the chain's best block,
  * --max-rows: the "evaluate" variant of the M = 50 cells at several chunk sizes (what flow.EVAL_MAX_ROWS was chosen from).

    python tools/bench_flow_eval.py [--out profiles/flow_eval.jsonl] [--cells reg:12:5,..] [--rounds 5] [--max-rows 8192,..]
    python tools/bench_flow_eval.py --trace CALLS   # CALLS batched calls of reg:12:50 alone (for a kernel trace)
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
from vpc_amd import _lib, flow, harness  # noqa: E402

TP = {"batch_size": 64, "patience": 1}
HID, N, BATCH = 500, 1600, 64
CELLS = "reg:12:5,van:12:5,reg:12:50,van:12:50,reg:128:5"


class _Recorder:
    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        if name.startswith("vpc_"):
            self.names.append(name)
        return getattr(self.real, name)


def make(kind, d):
    g = torch.Generator().manual_seed(0)
    x, m = torch.rand(N, d, generator=g).cuda(), (torch.rand(N, d, generator=g) < 0.7).cuda()
    torch.manual_seed(0)
    model = (vpc_amd.REG_VAEFlow if kind == "reg" else vpc_amd.VAEFlow)(d, HID, 10, 10, TP).cuda()
    loader = [(x[lo:lo + BATCH], m[lo:lo + BATCH]) for lo in range(0, N, BATCH)]
    return model, loader


def eval_call(model, loader, kind, d, M, engine):
    vae_type = "reg_flow1" if kind == "reg" else "vanilla_flow1"
    return lambda: vpc_amd.eval_vae([(loader, "test")], 30, d, HID, 10, M, 10, "bench", TP, "bench", vae_type, 1, 1, 1,
                                    alpha=0.5, reg_type="kl_reg", model=model, save=False, engine=engine, seed=1)


def block(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def abi_calls(fn):
    rec = _Recorder(_lib.lib())
    _lib._lib = rec
    try:
        fn()
    finally:
        _lib._lib = rec.real
    return len(rec.names)


def bench(kind, d, M, rounds, emit, max_rows_list):
    model, loader = make(kind, d)
    with torch.no_grad():
        gx, gm, ranges = harness._gather_passes([loader], M, d, torch.device("cuda"))
        ev = flow.FlowEvaluator(model, seed=1)
        variants = [("chain", eval_call(model, loader, kind, d, M, "chain")),
                    ("batched", eval_call(model, loader, kind, d, M, "batched")),
                    ("evaluate", lambda: ev.evaluate(gx, gm, ranges).cpu())]
        for mr in max_rows_list:
            e = flow.FlowEvaluator(model, seed=1, max_rows=mr)
            variants.append((f"evaluate_max_rows_{mr}", lambda e=e: e.evaluate(gx, gm, ranges).cpu()))
        calls = max(2, 50 // M)
        times, ncalls = {name: [] for name, _ in variants}, {}
        for name, fn in variants:  # code objects, workspaces, first launches
            block(fn, 2)
            ncalls[name] = abi_calls(fn)
        for _ in range(rounds):
            for name, fn in variants:
                block(fn, 1)
                times[name].append(block(fn, calls))
    cell = f"{kind}_d{d}_M{M}"
    for name, _ in variants:
        t = times[name]
        emit(dict(name=f"{name}_{cell}", kind=kind, d=d, hid=HID, N=N, batch=BATCH, M=M, rows=M * N, variant=name,
                  calls_per_block=calls, ms_per_call_blocks=[round(v, 3) for v in t], ms_median=round(statistics.median(t), 3),
                  ms_min=round(min(t), 3), ms_max=round(max(t), 3), abi_calls_per_call=ncalls[name]))
    emit(dict(name=f"summary_{cell}", kind=kind, d=d, M=M, batched_worst_ms=round(max(times["batched"]), 3),
              chain_best_ms=round(min(times["chain"]), 3), batched_worst_beats_chain_best=max(times["batched"]) < min(times["chain"]),
              median_ratio=round(statistics.median(times["chain"]) / statistics.median(times["batched"]), 1)))


def trace(calls):
    model, loader = make("reg", 12)
    fn = eval_call(model, loader, "reg", 12, 50, "batched")
    for _ in range(calls):
        r = fn()
    torch.cuda.synchronize()
    print(json.dumps(dict(name="trace", calls=calls, elbo=float(r["test"]["elbo"]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cells", default=CELLS)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-rows", default="")
    ap.add_argument("--trace", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow_eval.py measures on the GPU: no device found")
    if a.trace:
        return trace(a.trace)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    mr = [int(v) for v in a.max_rows.split(",") if v]
    for cell in a.cells.split(","):
        kind, d, M = cell.split(":")
        bench(kind, int(d), int(M), a.rounds, emit, mr if int(M) >= 50 else [])


if __name__ == "__main__":
    main()
