"""Small-batch one-kernel step of the mask-augmented classes on the MI355X: Reg_VAE_mask / vanilla_VAE_mask at
B <= ops.step_small_max_rows() run step_small_aug_kernel (csrc/vpc_small.hip: the N-split tile body with an input stage that
builds [x*mask | mask]) instead of the row-tiled sequence draw -> encoder_fwd -> decoder_fused -> encoder_bwd.

Tolerances are the project's own for a fused fp32 step against a float32 reference (tests/test_mask_augm.py): loss 2e-5
relative, every gradient tensor 2e-4 of its maximum.  The row-tiled path (VPC_STEP_SMALL=0) is held to the same goldens here,
since tests/test_mask_augm.py now runs the new path."""
import ctypes
import os

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from conftest import load_golden
from oracle import vae_oracle as O
from vpc_amd import fused, ops

pytestmark = pytest.mark.gpu
L = 10
DEV = "cuda"
TP = {"batch_size": 64, "patience": 1}
LOSS_TOL, GRAD_TOL = 2e-5, 2e-4


def need_rows(B):
    if ops.step_small_max_rows() < B:
        pytest.skip(f"the small-batch step is off for {B} rows (VPC_STEP_SMALL / VPC_TILE)")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def make_model(kind, d, params, reg_type="kl_reg"):
    m = vpc.Reg_VAE_mask(d, 500, 10, L, TP, "exp", reg_type) if kind == "reg" else vpc.vanilla_VAE_mask(d, 500, 10, L, TP, "exp")
    sd = m.state_dict()
    sd.update({k: v.clone() for k, v in params.items()})
    m.load_state_dict(sd)
    return m.to(DEV)


def synth(B, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, d, generator=g)
    mask = torch.rand(B, d, generator=g) < 0.7
    mask_p = mask & (torch.rand(B, d, generator=g) < 0.7)
    return x, mask, mask_p, torch.randn(B, L, generator=g), torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)


def check_step(tr, model, loss_ref, grads_ref, what):
    """loss and the 12 gradient tensors of the trainer's last step against a reference {key: array}"""
    loss = tr.loss_value()
    flat = tr.grad.cpu().numpy()
    assert np.isfinite(loss) and np.all(np.isfinite(flat)), what
    print(what, "loss", loss, "ref", loss_ref, "rel", abs(loss - loss_ref) / abs(loss_ref))
    assert abs(loss - loss_ref) <= LOSS_TOL * abs(loss_ref), (what, loss, loss_ref)
    off = 0
    for k, p in zip(O.PARAM_KEYS, model.trainable()):
        err = rel(flat[off:off + p.numel()].reshape(p.shape), grads_ref[k])
        print(what, k, err)
        assert err < GRAD_TOL, (what, k, err)
        off += p.numel()
    assert off == flat.size


# ------------------------------------------------------------------ 1. reference vectors, both paths
def _golden_params(g, kind):
    pre = f"{kind}.param."
    return {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(pre) and "prior" not in k}


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@pytest.mark.parametrize("path", ["step_small", "decoder_fused"])
def test_reference_vectors(path, monkeypatch):
    """maskaugm_d14.npz (B = 48, d = 14: pitch 16, the mask half straddles tiles 0 and 1) through FusedTrainer on the N-split
    kernel - this case fails before the mask-augmented instantiations exist: the step reports "decoder_fused" - and on the
    row-tiled path."""
    g = load_golden("maskaugm_d14.npz")
    if path == "decoder_fused":
        monkeypatch.setenv("VPC_STEP_SMALL", "0")
    else:
        need_rows(48)
    x, mk, mp = _t(g["x"]), _t(g["mask"]), _t(g["mask_p"])
    m = make_model("reg", 14, _golden_params(g, "reg"))
    tr = vpc.FusedTrainer(m)
    tr.step(x, mk, mp, _t(g["reg.eps_q"]), _t(g["reg.eps_p"]), alpha=0.7, beta=0.9, update=False)
    assert tr.dominant_launch() == path
    check_step(tr, m, float(g["reg.loss"]), {k: g[f"reg.grad.{k}"] for k in O.PARAM_KEYS}, f"reg {path}")
    m = make_model("vanilla", 14, _golden_params(g, "vanilla"))
    tr = vpc.FusedTrainer(m)
    tr.step(x, mk, eps_q=_t(g["vanilla.eps_q"]), beta=0.9, update=False)
    assert tr.dominant_launch() == path
    check_step(tr, m, float(g["vanilla.loss"]), {k: g[f"vanilla.grad.{k}"] for k in O.PARAM_KEYS}, f"vanilla {path}")


# ------------------------------------------------------------------ 2. shape grid against the oracle
def oracle_step(kind, reg_type, d, B, seed):
    params = O.init_params(d, L, seed=seed, mask_augm=True)
    x, mask, mask_p, eq, ep, eml = synth(B, d, seed + 100)
    if kind == "vanilla":
        loss, grads, _ = O.torch_vanilla_step(params, L, x, mask * torch.ones(x.shape), eq, beta=0.9, mask_augm=True)
    elif reg_type == "ml_reg":
        loss, grads, _ = O.torch_reg_step(params, L, x, mask, mask_p, eq, ep, reg_type="ml_reg", alpha=0.7, beta=0.9, epoch=1400,
                                          eps_ml=eml, mask_augm=True)
    else:
        loss, grads, _ = O.torch_reg_step(params, L, x, mask, mask_p, eq, ep, alpha=0.7, beta=0.9, mask_augm=True)
    return params, (x, mask, mask_p, eq, ep, eml), loss.item(), {k: v.numpy() for k, v in grads.items()}


def fused_step(kind, reg_type, d, params, data):
    x, mask, mask_p, eq, ep, eml = (t.to(DEV) for t in data)
    m = make_model(kind, d, params, reg_type)
    tr = vpc.FusedTrainer(m)
    if kind == "vanilla":
        tr.step(x, mask, eps_q=eq, beta=0.9, update=False)
    elif reg_type == "ml_reg":
        tr.step(x, mask, mask_p, eq, ep, eml, epoch=1400, alpha=0.7, beta=0.9, update=False)
    else:
        tr.step(x, mask, mask_p, eq, ep, alpha=0.7, beta=0.9, update=False)
    return m, tr


# d = 3: pitch 4, one tile, zero fill from column 6; d = 8, 16: the mask half ends on a tile edge; d = 14: it straddles a tile;
# d = 20: pitch 20, (4, 2) tiles; d = 33: pitch 36, 8 input against 4 output tiles; d = 64: the limit, no zero columns;
# B = 5, 33, 37: a last tile of 5, 1 and 5 rows
GRID = ([("reg", "kl_reg", d, B) for d, B in [(3, 5), (8, 16), (12, 64), (14, 37), (16, 33), (20, 37), (33, 5), (64, 64)]] +
        [("reg", "ml_reg", 14, 37), ("reg", "ml_reg", 64, 64), ("vanilla", None, 12, 64), ("vanilla", None, 33, 5)])


@pytest.mark.parametrize("kind,reg_type,d,B", GRID, ids=[f"{k}-{r}-d{d}-B{B}" for k, r, d, B in GRID])
def test_shape_grid_vs_oracle(kind, reg_type, d, B):
    need_rows(B)
    params, data, loss_ref, grads_ref = oracle_step(kind, reg_type, d, B, seed=7 * d + B)
    m, tr = fused_step(kind, reg_type, d, params, data)
    assert tr.dominant_launch() == "step_small"
    check_step(tr, m, loss_ref, grads_ref, f"{kind} {reg_type} d={d} B={B}")


# ------------------------------------------------------------------ 3. zero fill
def test_zero_fill_after_a_wider_model():
    """d = 3 (input columns 6 .. 15 of the one tile must be written as zeros) right after a step of a d = 64 model, whose input
    buffers filled all 128 columns of the same LDS.  Order-dependent by construction: both steps run here, in this order."""
    need_rows(64)
    params, data, _, _ = oracle_step("reg", "kl_reg", 64, 64, seed=1)
    fused_step("reg", "kl_reg", 64, params, data)
    torch.cuda.synchronize()
    params, data, loss_ref, grads_ref = oracle_step("reg", "kl_reg", 3, 16, seed=2)
    m, tr = fused_step("reg", "kl_reg", 3, params, data)
    assert tr.dominant_launch() == "step_small"
    check_step(tr, m, loss_ref, grads_ref, "zero fill d=3 B=16")


# ------------------------------------------------------------------ 4. same draws on both paths
def _drawn_step(d, B, env, monkeypatch, seed=11, **kw):
    if env is None:
        monkeypatch.delenv("VPC_STEP_SMALL", raising=False)
    else:
        monkeypatch.setenv("VPC_STEP_SMALL", env)
    params = O.init_params(d, L, seed=3, mask_augm=True)
    x, mask = (t.to(DEV) for t in synth(B, d, 5)[:2])
    m = make_model("reg", d, params)
    tr = vpc.FusedTrainer(m, seed=seed)
    tr.step(x, mask, alpha=0.7, beta=0.9, update=False, **kw)
    return m, tr


@pytest.mark.parametrize("d", [12, 64])
def test_same_draws_on_both_paths(d, monkeypatch):
    """d % 4 == 0: the pitch of the new path is d, so one seed gives both paths the same mask_p bytes and eps planes."""
    B = 64
    need_rows(B)
    m1, t1 = _drawn_step(d, B, None, monkeypatch)
    m0, t0 = _drawn_step(d, B, "0", monkeypatch)
    assert t1.dominant_launch() == "step_small" and t0.dominant_launch() == "decoder_fused"
    assert torch.equal(t1.mask_p_buf, t0.mask_p_buf)
    assert torch.equal(t1.eps_buf[:2].view(torch.int32), t0.eps_buf[:2].view(torch.int32))
    assert t1.rng_offset == t0.rng_offset
    l1, l0 = t1.loss_value(), t0.loss_value()
    assert abs(l1 - l0) <= LOSS_TOL * abs(l0), (l1, l0)
    g1, g0 = t1.grad.cpu().numpy(), t0.grad.cpu().numpy()
    off = 0
    for k, p in zip(O.PARAM_KEYS, m1.trainable()):
        assert rel(g1[off:off + p.numel()], g0[off:off + p.numel()]) < GRAD_TOL, k
        off += p.numel()


# ------------------------------------------------------------------ 5. five Adam steps
def test_adam_trajectory_matches_row_tiled(monkeypatch):
    """d = 14, B = 48, injected draws: five updates on the new path against five on the row-tiled one, at the bounds of
    test_fused_adam_trajectory_matches_golden (loss 3e-5 relative, final parameters 1e-4 of their maximum)."""
    d, B = 14, 48
    need_rows(B)
    params = O.init_params(d, L, seed=4, mask_augm=True)
    steps = [tuple(t.to(DEV) for t in synth(B, d, 40 + i)) for i in range(5)]
    out = {}
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("VPC_STEP_SMALL", raising=False)
        else:
            monkeypatch.setenv("VPC_STEP_SMALL", env)
        m = make_model("reg", d, params)
        tr = vpc.FusedTrainer(m)
        losses = []
        for x, mask, mask_p, eq, ep, _ in steps:
            tr.step(x, mask, mask_p, eq, ep, alpha=0.7, beta=0.9)
            losses.append(tr.loss_value())
        out[env] = (tr.dominant_launch(), losses, [p.detach().cpu().numpy() for p in m.trainable()])
    assert out[None][0] == "step_small" and out["0"][0] == "decoder_fused"
    for i, (a, b) in enumerate(zip(out[None][1], out["0"][1])):
        assert abs(a - b) <= 3e-5 * abs(b), (i, a, b)
    for k, a, b in zip(O.PARAM_KEYS, out[None][2], out["0"][2]):
        assert rel(a, b) < 1e-4, k


# ------------------------------------------------------------------ 6. shards
def test_shards_draw_the_rows_of_the_whole_batch(monkeypatch):
    d, B = 12, 64
    need_rows(B)
    monkeypatch.delenv("VPC_STEP_SMALL", raising=False)
    params = O.init_params(d, L, seed=3, mask_augm=True)
    x, mask = (t.to(DEV) for t in synth(B, d, 5)[:2])
    whole = vpc.FusedTrainer(make_model("reg", d, params), seed=11)
    whole.step(x, mask, alpha=0.7, update=False)
    assert whole.dominant_launch() == "step_small"
    for lo in (0, 32):
        tr = vpc.FusedTrainer(make_model("reg", d, params), seed=11)
        tr.step(x[lo:lo + 32], mask[lo:lo + 32], alpha=0.7, update=False, global_batch=B, row_lo=lo)
        assert tr.dominant_launch() == "step_small"
        assert torch.equal(tr.mask_p_buf, whole.mask_p_buf[lo:lo + 32]), lo
        assert torch.equal(tr.eps_buf[:2].view(torch.int32), whole.eps_buf[:2, lo:lo + 32].contiguous().view(torch.int32)), lo
        assert tr.rng_offset == whole.rng_offset


# ------------------------------------------------------------------ 7. graph replay
def test_graph_replay_matches_eager_steps(monkeypatch):
    d, B = 12, 64
    need_rows(B)
    monkeypatch.delenv("VPC_STEP_SMALL", raising=False)
    params = O.init_params(d, L, seed=9, mask_augm=True)
    x, mask = (t.to(DEV) for t in synth(B, d, 4)[:2])
    m1, m2 = make_model("reg", d, params), make_model("reg", d, params)
    t1, t2 = vpc.FusedTrainer(m1, seed=3), vpc.FusedTrainer(m2, seed=3)
    t2.step_graph(x, mask, alpha=0.9, beta=0.8)  # the eager warm-up step and the capture
    t1.step(x, mask, alpha=0.9, beta=0.8)
    for i in range(3):
        t1.step(x, mask, alpha=0.9, beta=0.8)
        t2.step_graph(x, mask, alpha=0.9, beta=0.8)
        assert torch.equal(t1.out9, t2.out9), i
        assert torch.equal(m1._flat, m2._flat), i
    assert t1.dominant_launch() == t2.dominant_launch() == "step_small"


# ------------------------------------------------------------------ 8. C entries
def test_c_entries_refuse_before_any_launch():
    """Every buffer is one zeroed device array that holds no model: a launch would leave partial blocks behind."""
    l = vpc._lib.lib()
    buf = torch.zeros(1 << 20, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    ptrs = (ctypes.c_void_p * 2)(p.value, p.value)
    co = vpc._lib.VpcLossCoef([1.0], [0.0], 1.0)
    nbv = ctypes.c_int(-1)
    nb = ctypes.byref(nbv)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def both(d, d_real, x=p):
        head = (x, p, p, 1, ptrs, None, co, ptrs, None, 1.0, 0.0, p, p, p, nb, 16, d, d_real, L)
        a = l.vpc_step_small_aug_f32(*head, stream)
        b = l.vpc_step_small_aug_draw_f32(*head, None, 0.7, p, 256, 0, 0, 0, None, 0, 16, 16, 0, 16, stream)
        assert a == b
        return a

    assert both(12, 13) == 2   # d_real > d
    assert both(16, 12) == 2   # d - d_real > 3
    assert both(14, 14) == 2   # d % 4 != 0
    assert both(68, 65) == 2   # 2 * d_real > 128
    assert both(16, 14, x=ctypes.c_void_p(p.value + 4)) == 1   # misaligned x
    torch.cuda.synchronize()
    assert nbv.value == -1 and not bool(buf.any())


# ------------------------------------------------------------------ 9. harness.train
@pytest.mark.parametrize("vae_type", ["vanilla_vae_with_drop_mask_augm1", "reg_vae_mask_augm1"])
def test_harness_train(vae_type, tmp_path, monkeypatch):
    d, B = 12, 16
    need_rows(B)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("VPC_STEP_SMALL", raising=False)
    used = []
    real_step = fused.FusedTrainer.step

    def step(self, *a, **k):
        used.append(self)
        return real_step(self, *a, **k)

    monkeypatch.setattr(fused.FusedTrainer, "step", step)
    x, mask = synth(2 * B, d, 8)[:2]
    loader = [(x[i:i + B], mask[i:i + B]) for i in range(0, 2 * B, B)]
    torch.manual_seed(1)
    m0 = vpc.model_loader("train", d, 500, 10, L, 30, "synth", TP, 1, 20, 10, "exp", "kl_reg", vae_type, alpha=0.5, p_missingness=30)
    before = [p.detach().clone() for p in m0.trainable()]
    m = vpc.train((loader, None), 30, d, 500, 10, 1, L, "synth", TP, "exp", vae_type, 20, 10, max_epochs=1,
                  device=torch.device(DEV), alpha=0.5, p_missingness=30, reg_type="kl_reg", verbose=False, model=m0)
    assert len(used) == 2 and used[0] is used[1]
    assert used[0].dominant_launch() == "step_small"
    assert os.path.exists(vpc.checkpoint_path("exp", "synth", vae_type, 30, alpha=0.5, p_missingness=30, reg_type="kl_reg"))
    after = [p.detach().cpu() for p in m.trainable()]
    assert all(torch.isfinite(a).all() for a in after)
    assert all(not torch.equal(a, b.cpu()) for a, b in zip(after, before))
