"""The tile / pass loops of the fp32 step's MFMA kernels (csrc/vpc_enc.hip, csrc/vpc_dec8.hip) at the smallest shapes where
state carried from one (tile, pass) of a workgroup to the next can go wrong - written for a prefetch across tile-passes
(measured and not kept, profiles/fp32_scalar_ownership_notes.md), kept because the existing tests never run a batch where
SOME workgroups have two tiles and others one.  C = the CU count (a grid is at most C workgroups of 128-row tiles):
    B = 128 (C + 1) + 37   a few workgroups run two tiles, the rest one; the last tile is ragged; a request past the last
                           tile would show (its rows would enter the gradients);
    the same B, 64-row tiles   the 4-wave kernels' tile loop (2 C + 3 tiles over C workgroups x passes on blockIdx.y);
    vanilla_VAE (one pass)     the next pair is always the next tile;
    d = 100                    columns past d in the last feature tiles;
    B = 300, 128-row tiles     three workgroups, one tile each: "no next tile" in every pass.
Tolerances are those of tests/test_gpu_parity.py (loss 2e-5 relative, gradients 2e-4 of the tensor's max against
oracle/vae_oracle.py; the two decoder kernels 2e-6 / 2e-5 against each other); the same step run twice gives the same bits.
"""
import functools

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from oracle import vae_oracle as O

pytestmark = pytest.mark.gpu
L = 10
TP = {"batch_size": 64, "patience": 100}
DEV = "cuda"
ALPHA, BETA = 0.8, 0.9


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def make_model(kind, d, params):
    if kind == "reg":
        m = vpc.Reg_VAE(d, 500, 10, L, TP, "exp", "kl_reg")
    else:
        m = vpc.vanilla_VAE(d, 500, 10, L, TP, "exp")
    sd = m.state_dict()
    for k, v in params.items():
        sd[k] = v.clone()
    m.load_state_dict(sd)
    return m.to(DEV)


def cus():
    return vpc._lib.max_blocks() // 2


@functools.lru_cache(maxsize=None)
def case(kind, d, B):
    """Inputs and the oracle's loss / gradients of one shape: computed once, shared by the tests, never modified."""
    g = torch.Generator().manual_seed(B + d)
    x = torch.rand(B, d, generator=g)
    mask = torch.rand(B, d, generator=g) < 0.7
    mask_p = mask & (torch.rand(B, d, generator=g) < 0.7)
    eq, ep = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    params = O.init_params(d, L, seed=7)
    if kind == "reg":
        loss, grads, _ = O.torch_reg_step(params, L, x, mask, mask_p, eq, ep, alpha=ALPHA, beta=BETA)
    else:
        loss, grads, _ = O.torch_vanilla_step(params, L, x, mask, eq)
    return params, (x, mask, mask_p, eq, ep), loss.item(), {k: v.numpy() for k, v in grads.items()}


def run_step(kind, d, params, inputs):
    x, mask, mask_p, eq, ep = (t.to(DEV) for t in inputs)
    m = make_model(kind, d, params)
    tr = vpc.FusedTrainer(m)
    out = []
    for _ in range(2):
        if kind == "reg":
            tr.step(x, mask, mask_p, eq, ep, alpha=ALPHA, beta=BETA, update=False)
        else:
            tr.step(x, mask, eps_q=eq, update=False)
        out.append((tr.loss_value(), tr.grad.clone()))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])  # the same step twice: the same bits
    return m, out[0][0], out[0][1].cpu().numpy()


def check_vs_oracle(kind, d, B):
    params, inputs, loss_ref, grads_ref = case(kind, d, B)
    m, loss, flat = run_step(kind, d, params, inputs)
    print(f"{kind} d={d} B={B}: loss {loss!r} oracle {loss_ref!r} rel {abs(loss - loss_ref) / abs(loss_ref):.3g}")
    errs, off = {}, 0
    for k, p in zip(O.PARAM_KEYS, m.trainable()):
        errs[k] = rel(flat[off:off + p.numel()].reshape(p.shape), grads_ref[k])
        off += p.numel()
    print("   gradient errors (of max):", {k: f"{v:.3g}" for k, v in errs.items()})
    assert abs(loss - loss_ref) <= 2e-5 * abs(loss_ref)
    for k, v in errs.items():
        assert v < 2e-4, k


@pytest.mark.parametrize("tile", ["128", "64"])
def test_two_tiles_in_some_workgroups_ragged_last_tile(tile, monkeypatch):
    monkeypatch.setenv("VPC_TILE", tile)
    check_vs_oracle("reg", 128, 128 * (cus() + 1) + 37)


def test_one_pass_next_pair_is_next_tile(monkeypatch):
    monkeypatch.setenv("VPC_TILE", "128")
    check_vs_oracle("vanilla", 128, 128 * (cus() + 1) + 37)


def test_columns_past_d(monkeypatch):
    monkeypatch.setenv("VPC_TILE", "128")
    check_vs_oracle("reg", 100, 128 * (cus() + 1) + 5)


def test_no_next_tile_in_any_pass(monkeypatch):
    monkeypatch.setenv("VPC_TILE", "128")
    check_vs_oracle("reg", 128, 300)


def test_decoder_kernel_variants_agree_across_tiles(monkeypatch):
    """The 8-wave decoder against the 4-wave one (VPC_DEC8=0) where some workgroups run two tiles."""
    monkeypatch.setenv("VPC_TILE", "128")
    params, inputs, _, _ = case("reg", 128, 128 * (cus() + 1) + 37)
    res = []
    for v in ("1", "0"):
        monkeypatch.setenv("VPC_DEC8", v)
        _, loss, flat = run_step("reg", 128, params, inputs)
        res.append((loss, flat))
    print(f"dec8 vs dec: loss rel {abs(res[0][0] - res[1][0]) / abs(res[1][0]):.3g}, grad {rel(res[0][1], res[1][1]):.3g}")
    assert abs(res[0][0] - res[1][0]) <= 2e-6 * abs(res[1][0])
    assert rel(res[0][1], res[1][1]) < 2e-5
