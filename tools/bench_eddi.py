"""Step time of the EDDI family on the API path: model.forward -> model.loss -> backward ->
torch.optim.Adam on one MI355X, the front-end kernels timed separately, the CPU port timed beside it.

    python tools/bench_eddi.py [--batch 64] [--d 128] [--k 20] [--vanilla] [--no-cpu]

    python tools/bench_eddi.py --small [--shapes 12x64,12x1024,64x64] [--steps 300] [--out profiles/eddi_small.jsonl]

The small-batch one-kernel step instead (csrc/vpc_small.hip: step_small_eddi_kernel): per (d, B), for Reg_EDDI K = 10 and
vanilla_EDDI K = 20, EDDITrainer.step (eager, device draws, Adam included) on the small path against the launch chain
(VPC_STEP_SMALL=0) in ONE process, a trainer each, warm-up, five alternating timed blocks per path, the median of each, and
the C ABI launches of one step.  One JSON line per (class, d, B), appended to --out.  64 is the widest obs_dim instantiated.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpc_amd  # noqa: E402
from vpc_amd import eddi  # noqa: E402


class _Launches:
    """Stands in for the loaded library during one step: counts the vpc_* entries fetched that launch a kernel."""
    HOST_ONLY = ("vpc_step_small_max_rows", "vpc_eddi_front_scratch", "vpc_linear_wgrad_scratch")

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        if name.startswith("vpc_") and name not in self.HOST_ONLY:
            self.names.append(name)
        return getattr(self.real, name)


# kernels behind one call of an entry, where that is not one (csrc/vpc_eddi.hip: backward, reduction, chain rule)
_KERNELS_PER_ENTRY = {"vpc_eddi_front_bwd": 3}


def run_small(cls, d, K, B, steps, blocks=5):
    from vpc_amd import _lib
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, d, generator=g).cuda()
    mask = (torch.rand(B, d, generator=g) < 0.7).cuda()
    paths = {"small": None, "chain": "0"}  # value of VPC_STEP_SMALL
    trs, times, launches = {}, {k: [] for k in paths}, {}

    def select(env):
        os.environ.pop("VPC_STEP_SMALL", None)
        if env is not None:
            os.environ["VPC_STEP_SMALL"] = env

    def step(tr):
        tr.step(x, mask, epoch=1, alpha=0.5, p_missingness=30)

    for name, env in paths.items():
        select(env)
        torch.manual_seed(0)
        tp = {"batch_size": B, "patience": 1}
        m = (eddi.Reg_EDDI(d, 500, K, 10, tp, "bench", "kl_reg") if cls == "Reg_EDDI" else
             eddi.vanilla_EDDI(d, 500, K, 10, tp, "bench")).cuda()
        tr = trs[name] = eddi.EDDITrainer(m, seed=1)
        for _ in range(60):
            step(tr)
        rec = _Launches(_lib.lib())
        _lib._lib = rec
        step(tr)
        _lib._lib = rec.real
        launches[name] = rec.names
        assert tr.last_path == name, (tr.last_path, name)
    gc.collect()
    gc.disable()
    for _ in range(blocks):
        for name, env in paths.items():
            select(env)
            tr = trs[name]
            for _ in range(20):
                step(tr)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(tr)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e6)
    gc.enable()
    select(None)
    out = dict(model=cls, d=d, K=K, B=B, steps=steps, blocks=blocks)
    for name in paths:
        out[name] = dict(us_per_step=round(statistics.median(times[name]), 1), all_us=[round(t, 1) for t in times[name]],
                         entries=launches[name], launches=sum(_KERNELS_PER_ENTRY.get(n, 1) for n in launches[name]),
                         loss=trs[name].loss_value())
    chain = out["chain"]["all_us"]
    out["chain_spread_us"] = round(max(chain) - min(chain), 1)
    out["speedup"] = round(out["chain"]["us_per_step"] / out["small"]["us_per_step"], 2)
    # the routing rule of profiles/eddi_small_notes.md: the small path's median below the chain's by more than the chain's spread
    out["route_small"] = out["chain"]["us_per_step"] - out["small"]["us_per_step"] > out["chain_spread_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="the small-batch one-kernel step against the launch chain")
    ap.add_argument("--shapes", default="12x64,12x1024,64x64", help="--small: d x B pairs")
    ap.add_argument("--out", default=None, help="--small: also append the JSON lines to this file")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--latent", type=int, default=10)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (per block with --small): default 50, 300 with --small")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--vanilla", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--api", action="store_true", help="time the API path instead of the fused EDDITrainer step")
    a = ap.parse_args()
    if a.small:
        for cls, K in (("Reg_EDDI", 10), ("vanilla_EDDI", 20)):
            for d, B in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
                line = json.dumps(run_small(cls, d, K, B, a.steps or 300))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        return
    a.steps = a.steps or 50
    B, d, K, L = a.batch, a.d, a.k, a.latent
    torch.manual_seed(0)
    tp = {"batch_size": B, "patience": 1}
    model = (eddi.vanilla_EDDI(d, 500, K, L, tp, "bench") if a.vanilla else
             eddi.Reg_EDDI(d, 500, K, L, tp, "bench", "kl_reg")).cuda()
    model.flatten_parameters()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    x = torch.rand(B, d, device="cuda")
    m = torch.rand(B, d, device="cuda") < 0.7

    tr = None if a.api else eddi.EDDITrainer(model, seed=0)

    def step():
        if tr is not None:
            tr.step(x, m, epoch=1, alpha=0.5, p_missingness=30)
            return tr.out9[0]
        mp = None if a.vanilla else vpc_amd.create_missing_uci(x.shape, 30) * m
        _, (_, tl) = model.forward_loss(x, m, mp, epoch=1, alpha=0.5)
        opt.zero_grad()
        tl.backward()
        opt.step()
        return tl

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()  # a gen-2 collection inside the loop stalls the host for tens of ms (profiles/r01_notes.md)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        tl = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    gc.enable()
    # front-end kernels alone (HBM-bound: x fp32 + mask u8 in, agg out)
    mu8 = m.view(torch.uint8)
    AC = torch.empty(2, K, d, device="cuda")
    t = model.trainable()
    eddi.eddi_fold(t[12], t[13], t[14], t[15], AC, d, K)
    agg = torch.empty(B, K, device="cuda")
    dagg = torch.randn(B, K, device="cuda")
    g = [torch.empty_like(p) for p in t[12:]]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(3):
        eddi.eddi_front_fwd(x, mu8, AC, agg, B, d, K)
        eddi.eddi_front_bwd(x, mu8, AC, dagg, t[12], t[13], t[14], *g, B, d, K)
    ev[0].record()
    for _ in range(20):
        eddi.eddi_front_fwd(x, mu8, AC, agg, B, d, K)
    ev[1].record()
    for _ in range(20):
        eddi.eddi_front_bwd(x, mu8, AC, dagg, t[12], t[13], t[14], *g, B, d, K)
    ev[2].record()
    torch.cuda.synchronize()
    f_ms, b_ms = ev[0].elapsed_time(ev[1]) / 20, ev[1].elapsed_time(ev[2]) / 20
    out = {"metric": "EDDI training samples/sec (" + ("API path" if a.api else "fused EDDITrainer step") + ")", "value": B / dt,
           "unit": "samples/s", "ms_per_step": dt * 1e3, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"{'vanilla_EDDI' if a.vanilla else 'Reg_EDDI kl_reg'} B={B} d={d} K={K} L={L}"},
           "loss": float(tl),
           "front_end": {"fwd_ms": f_ms, "bwd_ms": b_ms, "fwd_GBps": B * d * 5 / f_ms / 1e6,
                         "bytes_model": "x fp32 + mask u8 per (row, feature); agg / dagg B*K*4"}}
    if not a.no_cpu:
        from oracle import eddi_oracle as O
        nthr = min(16, os.cpu_count() or 1)
        torch.set_num_threads(nthr)
        Bc = min(B, 4096)
        sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items() if k in O.EDDI_KEYS}
        port = O.EDDIPort(sd, L, "kl_reg")
        copt = torch.optim.Adam(list(sd.values()), lr=1e-3)
        xc, mc = x[:Bc].cpu(), m[:Bc].cpu()

        def cstep():
            if a.vanilla:
                mf = mc.float()
                o = port.vanilla_forward(xc, mf)
                _, l = port.vanilla_loss(xc, o[2], o[3], o[0], o[1], 1, mf)
            else:
                mp = mc & (torch.rand(Bc, d) < 0.7)
                o = port.reg_forward(xc, mc, mp)
                _, l = port.reg_loss(xc, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mc, mp, 1, alpha=0.5)
            copt.zero_grad()
            l.backward()
            copt.step()
        cstep()
        n, t1 = 0, time.perf_counter()
        while time.perf_counter() - t1 < 8.0:
            cstep()
            n += 1
        cdt = (time.perf_counter() - t1) / n
        out["cpu_baseline"] = {"value": Bc / cdt, "unit": "samples/s", "cores": nthr, "kind": "port",
                               "sample": f"{n} steps of the torch port at B={Bc}, ~8 s"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
