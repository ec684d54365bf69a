"""Config 5 (active variable selection) for every encoder family: one acquisition step's reward matrix R[n, d-1] at
n_test = 256, M = 50 (Data/imputation_args.json) - GPU (vpc.reward_matrix: vpc_reward_matrix for the plain model,
vpc_reward_matrix_ex for the others) and, unless --no-cpu, the oracle's op-for-op CPU port of the reference loop
(evaluate.py:424-433, 514-634) on a sample of 2 candidates, extrapolated.  One JSON line per configuration.

    python tools/bench_reward_families.py [--no-cpu] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpc_amd as vpc  # noqa: E402
from oracle import eddi_oracle as EO  # noqa: E402
from oracle import vae_oracle as O  # noqa: E402

n, M, L = 256, 50, 10
TP = {"batch_size": n, "patience": 1}
CONFIGS = [  # (label, model family, d, K)
    ("plain", "vae", 128, None),
    ("eddi_K10", "eddi", 128, 10),
    ("eddi_K32", "eddi", 128, 32),
    ("mask_augm", "vaemask", 64, None),
    ("wide", "vae", 129, None),
    ("wide", "vae", 256, None),
]


def model_and_port(family, d, K):
    torch.manual_seed(0)
    if family == "eddi":
        m = vpc.Reg_EDDI(d, 500, K, L, TP, "b", "kl_reg")
    elif family == "vaemask":
        m = vpc.Reg_VAE_mask(d, 500, 10, L, TP, "b", "kl_reg")
    else:
        m = vpc.Reg_VAE(d, 500, 10, L, TP, "b", "kl_reg")
    params = {k: v.detach().clone() for k, v in m.state_dict().items() if "prior" not in k}
    port = EO.EDDIPort(params, L) if family == "eddi" else O.TorchPort(params, L, mask_augm=family == "vaemask")
    return m.cuda(), port


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    for label, family, d, K in CONFIGS:
        m, port = model_and_port(family, d, K)
        g = torch.Generator().manual_seed(d)
        x = torch.rand(n, d, generator=g)
        mask = (torch.rand(n, d, generator=g) < 0.5).float()
        mask[:, -1] = 0
        im = torch.rand(M, n, d, generator=g)
        xd, md, imd = x.cuda(), mask.cuda(), im.cuda()
        for _ in range(3):
            vpc.reward_matrix(m, xd, md, imd)
        torch.cuda.synchronize()
        ts = []  # as tools/bench_reward.py: the mean of `iters` back-to-back calls, five times
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(a.iters):
                vpc.reward_matrix(m, xd, md, imd)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / a.iters * 1e3)
        rec = {"workload": f"reward matrix {label} n={n} d={d} M={M}" + (f" K={K}" if K else "") + " (one acquisition step)",
               "gpu_ms_median": float(np.median(ts)), "gpu_ms_min": float(np.min(ts)), "iters": a.iters}
        if not a.no_cpu:
            t0 = time.perf_counter()
            with torch.no_grad():
                for u in (0, d // 2):
                    loc = np.where(mask[:, u].numpy() == 0)[0]
                    O.R_lindley_chain(port, u, x, mask, M, im, loc)
            rec["cpu_port_ms_extrapolated_from_2_candidates"] = (time.perf_counter() - t0) / 2 * (d - 1) * 1e3
            rec["cpu_threads"] = torch.get_num_threads()
            rec["speedup"] = rec["cpu_port_ms_extrapolated_from_2_candidates"] / rec["gpu_ms_median"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
