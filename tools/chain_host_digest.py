"""Digest of what the host code of the three chain-backed families (notmiwae.py, miwae.py, flow.py) computes: one line
`case tensor sha256` per tensor, to compare two trees that load the same build of the library.  Only names that both
trees have are used.

  * trainers, 3 steps each with device draws, seed = 1, B = 16: NMTrainer f32 (both classes; d = 12, L = 10, K = 5), NMTrainer
    bf16 (d = 128, L = 10, K = 8; prints use_nmdec and whether the fused tail ran), NMTrainer.step_graph (f32, 3 calls),
    MIWTrainer chain and small path (both classes; d = 12, L = 10, S = 4; prints last_path), FlowTrainer (both classes; d = 12,
    hid_dim 64): model._flat, exp_avg, exp_avg_sq, tail, rng_offset, step_count,
  * eager, the six classes at those shapes: torch.manual_seed(0), forward_loss under grad, backward: the loss and every p.grad,
  * streaming imputation, the four MIWAE / MNAR classes at B = 5, S = 40: impute_stream(seed=7, return_lse=True): xm, lse.

    python tools/chain_host_digest.py > profiles/chain_host_digest_new.txt
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vpc_amd as vpc  # noqa: E402
from vpc_amd import miwae, notmiwae  # noqa: E402

TP = {"batch_size": 16, "patience": 1}
ALL_ROWS = str(1 << 30)


def emit(case, name, value):
    if torch.is_tensor(value):
        data = value.detach().contiguous().cpu().numpy().tobytes()
    else:
        data = repr(value).encode()
    print(f"{case} {name} {hashlib.sha256(data).hexdigest()}", flush=True)


def data(B, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    x, m = torch.rand(B, d, generator=g), (torch.rand(B, d, generator=g) < 0.7).float()
    mp = m * (torch.rand(B, d, generator=g) < 0.7).float()
    return x.cuda(), m.cuda(), mp.cuda()


def model_of(cls, d, S, hid=500):
    torch.manual_seed(0)
    if cls in (vpc.VAEFlow, vpc.REG_VAEFlow):
        return cls(d, hid, 10, 10, TP).cuda()
    return cls(d, hid, 10, 10, TP, S, 1).cuda()


def trainer_case(case, tr, step, note=None):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    if note is not None:
        print(f"{case} note {note()}", flush=True)
    for name in ("exp_avg", "exp_avg_sq", "tail", "rng_offset", "step_count"):
        emit(case, name, getattr(tr, name))
    emit(case, "flat", tr.model._flat)


def trainers():
    for cls in (vpc.REG_notMIWAE_v2, vpc.notMIWAE_myversion):
        x, m, _ = data(16, 12)
        tr = vpc.NMTrainer(model_of(cls, 12, 5), seed=1)
        trainer_case(f"nm_f32_{cls.__name__}", tr, lambda: tr.step(x, m, alpha=0.5, p_missingness=30))
    x, m, _ = data(16, 128)
    tr = vpc.NMTrainer(model_of(vpc.REG_notMIWAE_v2, 128, 8), seed=1, precision="bf16")
    trainer_case("nm_bf16_REG_notMIWAE_v2", tr, lambda: tr.step(x, m, alpha=0.5, p_missingness=30),
                 lambda: f"use_nmdec={tr.use_nmdec} fused_tail={bool(tr._repacked)}")
    x, m, _ = data(16, 12)
    tr = vpc.NMTrainer(model_of(vpc.REG_notMIWAE_v2, 12, 5), seed=1)
    trainer_case("nm_graph_REG_notMIWAE_v2", tr, lambda: tr.step_graph(x, m, alpha=0.5, p_missingness=30))
    for path, rows in (("chain", "0"), ("small", ALL_ROWS)):
        os.environ["VPC_MIW_SMALL"] = rows
        for cls in (vpc.Reg_MIWAE, vpc.MIWAE):
            tr = vpc.MIWTrainer(model_of(cls, 12, 4), seed=1)
            trainer_case(f"miw_{path}_{cls.__name__}", tr, lambda: tr.step(x, m, alpha=0.5, p_missingness=30),
                         lambda: f"last_path={tr.last_path}")
    del os.environ["VPC_MIW_SMALL"]
    for cls in (vpc.REG_VAEFlow, vpc.VAEFlow):
        tr = vpc.FlowTrainer(model_of(cls, 12, 1, 64), seed=1)
        trainer_case(f"flow_{cls.__name__}", tr, lambda: tr.step(x, m, alpha=0.5, p_missingness=30))


def eager():
    x, m, mp = data(16, 12)
    for cls, S, hid in ((vpc.REG_notMIWAE_v2, 5, 500), (vpc.notMIWAE_myversion, 5, 500), (vpc.Reg_MIWAE, 4, 500),
                        (vpc.MIWAE, 4, 500), (vpc.REG_VAEFlow, 1, 64), (vpc.VAEFlow, 1, 64)):
        model = model_of(cls, 12, S, hid)
        torch.manual_seed(0)
        _, ret = model.forward_loss(x, m, mp if model.regularised else None, epoch=1, alpha=0.5)
        ret[1].backward()
        torch.cuda.synchronize()
        case = f"eager_{cls.__name__}"
        emit(case, "loss", ret[1])
        for name, p in model.named_parameters():
            if p.grad is not None:
                emit(case, f"grad:{name}", p.grad)


def stream():
    x, m, _ = data(5, 12, 3)
    for mod, cls in ((notmiwae, vpc.REG_notMIWAE_v2), (notmiwae, vpc.notMIWAE_myversion), (miwae, vpc.Reg_MIWAE),
                     (miwae, vpc.MIWAE)):
        xm, lse = mod.impute_stream(model_of(cls, 12, 40), x, m, seed=7, return_lse=True)
        torch.cuda.synchronize()
        emit(f"stream_{cls.__name__}", "xm", xm)
        emit(f"stream_{cls.__name__}", "lse", lse)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("chain_host_digest.py runs on the GPU: no device found")
    trainers()
    eager()
    stream()
