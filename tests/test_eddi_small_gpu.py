"""Small-batch one-kernel step of the point-net classes on the MI355X: Reg_EDDI / vanilla_EDDI at B <= ops.step_small_max_rows(),
K <= 32, obs_dim <= 64 run step_small_eddi_kernel (csrc/vpc_small.hip: the N-split tile body with the folded front-end as its input
stage and the front-end's backward behind the encoder backward) and one tail launch instead of the chain of about twenty.

Bounds are the project's own for EDDITrainer against the reference (tests/test_eddi_gpu.py): loss 1e-4 relative, each of the 16
gradient tensors 2e-4 of its maximum; trajectories 1e-4 on the losses and 5e-5 on the final parameters."""
import ctypes

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from conftest import load_golden
from oracle import eddi_oracle as EO
from vpc_amd import eddi, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TP = {"batch_size": 64, "patience": 1}
LOSS_TOL, GRAD_TOL = 1e-4, 2e-4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _close(a, b, tol, what):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    print(what, "max abs err", err, "scale", scale)
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} (scale {scale:.3e})"


def _load(g, cls, *extra, prefix="param."):
    d = g["x"].shape[1]
    model = cls(d, 500, int(g["K"]), int(g["L"]), TP, "exp", *extra)
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(prefix)})
    return model.to(DEV)


def _check_loss(tr, ref, what):
    loss = tr.loss_value()
    print(what, "loss", loss, "ref", ref, "rel", abs(loss - ref) / abs(ref))
    assert np.isfinite(loss) and abs(loss - ref) <= LOSS_TOL * abs(ref), (what, loss, ref)


def _check_grads(model, ref, what):
    """all 16 gradient tensors of the last step against {state_dict key: array or tensor}"""
    n = 0
    for k, p in model.named_parameters():
        if k in ref:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            _close(p.grad, ref[k], GRAD_TOL, f"{what} grad {k}")
            n += 1
    assert n == 16, n


def _golden_grads(g, tag):
    pre = f"grad.{tag}."
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


# ------------------------------------------------------------------ 1. vectors captured from the reference
@pytest.mark.parametrize("name", ["eddi_reg_d14.npz", "eddi_reg_d40.npz"])
def test_reg_reference_vectors(name):
    """eddi_reg_d14: B = 32, d = 14 (pitch 16), K = 10 - two row tiles, one input tile; eddi_reg_d40: B = 48, d = 40, K = 20,
    L = 6 - three row tiles, two input tiles, DT = 4.  Injected draws, update included (the gradients are those of the step).
    Fails before the small-batch step exists: the trainer has no last_path."""
    g = load_golden(name)
    x, m, mp = _dev(g["x"]), _dev(g["mask"]), _dev(g["mask_p"])
    for tag, rt, alpha in (("kl0.5", "kl_reg", 0.5), ("kl1.0", "kl_reg", 1.0), ("ml0.8", "ml_reg", 0.8)):
        model = _load(g, eddi.Reg_EDDI, rt)
        tr = eddi.EDDITrainer(model)
        tr.step(x, m, mask_p=mp, eps_q=_dev(g["eps_q"]), eps_p=_dev(g["eps_p"]), eps_ml=_dev(g["eps_ml"]), epoch=1400, beta=0.9,
                alpha=alpha, beta_annealing=(tag == "kl1.0"))
        assert tr.last_path == "small"
        _check_loss(tr, float(g[f"loss.{tag}"]), f"{name} {tag}")
        _check_grads(model, _golden_grads(g, tag), f"{name} {tag}")


def test_vanilla_reference_vectors():
    """eddi_van_d14: K = 20, two input tiles, one pass."""
    g = load_golden("eddi_van_d14.npz")
    model = _load(g, eddi.vanilla_EDDI)
    tr = eddi.EDDITrainer(model)
    tr.step(_dev(g["x"]), _dev(g["mask"]), eps_q=_dev(g["eps_q"]), epoch=3, beta=0.8)
    assert tr.last_path == "small"
    _check_loss(tr, float(g["loss"]), "eddi_van_d14")
    _check_grads(model, _golden_grads(g, "v"), "eddi_van_d14")


# ------------------------------------------------------------------ 2. trajectories
@pytest.mark.parametrize("kind", ["reg", "van"])
def test_adam_trajectory(kind):
    """Five Adam steps of the reference; afterwards model.decoder (its own packed image) follows the state dict."""
    g = load_golden(f"eddi_traj_{kind}_d14.npz")
    model = (_load(g, eddi.Reg_EDDI, "kl_reg", prefix="param0.") if kind == "reg" else
             _load(g, eddi.vanilla_EDDI, prefix="param0."))
    tr = eddi.EDDITrainer(model, lr=1e-3)
    x, m = _dev(g["x"]), _dev(g["mask"])
    for s in range(len(g["losses"])):
        eps = _dev(g["eps"][s])
        if kind == "reg":
            tr.step(x, m, mask_p=_dev(g["mask_p"][s]), eps_q=eps[0], eps_p=eps[1], epoch=s + 1, alpha=0.5)
        else:
            tr.step(x, m, eps_q=eps[0], epoch=s + 1)
        assert tr.last_path == "small"
        ref = float(g["losses"][s])
        print(kind, s, tr.loss_value(), ref)
        assert abs(tr.loss_value() - ref) <= 1e-4 * abs(ref), (s, tr.loss_value(), ref)
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith("param5."):
            _close(sd[k[7:]], torch.from_numpy(v), 5e-5, k)
    F = torch.nn.functional
    with torch.no_grad():
        z = torch.linspace(-1, 1, 4 * int(g["L"]), device=DEV).reshape(4, -1)
        xhat, _ = model.decoder(z)
        ref = torch.sigmoid(F.linear(torch.relu(F.linear(torch.relu(F.linear(z, sd["seq_decoder.0.weight"], sd["seq_decoder.0.bias"])),
                                                         sd["seq_decoder.2.weight"], sd["seq_decoder.2.bias"])),
                                     sd["seq_decoder.4.weight"], sd["seq_decoder.4.bias"]))
    _close(xhat, ref, 2e-5, "decoder after the small-batch steps")


# ------------------------------------------------------------------ 3. ragged and edge shapes against the oracle's port
def _oracle_step(kind, d, K, B, Ld, seed, zero_row=None):
    torch.manual_seed(seed)
    model = (eddi.Reg_EDDI(d, 500, K, Ld, TP, "exp", "kl_reg") if kind == "reg" else eddi.vanilla_EDDI(d, 500, K, Ld, TP, "exp"))
    p = {k: v.detach().clone().float().requires_grad_(True) for k, v in model.state_dict().items() if k in EO.EDDI_KEYS}
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(B, d, generator=g)
    m = torch.rand(B, d, generator=g) < 0.7
    if zero_row is not None:
        m[zero_row] = False
    mp = m & (torch.rand(B, d, generator=g) < 0.7)
    eq, ep = torch.randn(B, Ld, generator=g), torch.randn(B, Ld, generator=g)
    port = EO.EDDIPort(p, Ld, "kl_reg")
    if kind == "reg":
        o = port.reg_forward(x, m, mp, eq, ep)
        _, ref = port.reg_loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], m, mp, 1, alpha=0.5, beta=1.0)
    else:
        o = port.vanilla_forward(x, m, eq)
        _, ref = port.vanilla_loss(x, o[2], o[3], o[0], o[1], 1, m)
    ref.backward()
    model = model.to(DEV)
    tr = eddi.EDDITrainer(model)
    if kind == "reg":
        tr.step(x.to(DEV), m.to(DEV), mask_p=mp.to(DEV), eps_q=eq.to(DEV), eps_p=ep.to(DEV), epoch=1, alpha=0.5)
    else:
        tr.step(x.to(DEV), m.to(DEV), eps_q=eq.to(DEV), epoch=1)
    return tr, model, ref.item(), {k: v.grad for k, v in p.items()}


# B = 1 and 21: a single row, a last tile with 5 valid rows; K = 10, 16, 17, 32: below, at and above one input tile, the limit;
# the 21-row cases carry a row with an all-zero mask (agg = 0, no front-end gradient from it)
EDGE = [("reg", 12, 10, 1, None), ("reg", 12, 10, 21, 3), ("van", 12, 16, 21, 20), ("reg", 12, 17, 21, 0), ("reg", 12, 32, 21, 7),
        ("van", 12, 32, 1, None), ("reg", 64, 32, 21, 18)]


@pytest.mark.parametrize("kind,d,K,B,zero_row", EDGE, ids=[f"{k}-d{d}-K{K}-B{B}" for k, d, K, B, _ in EDGE])
def test_edge_shapes_vs_oracle(kind, d, K, B, zero_row):
    tr, model, loss_ref, grads_ref = _oracle_step(kind, d, K, B, 10, seed=100 * K + B, zero_row=zero_row)
    assert tr.last_path == "small"
    what = f"{kind} d={d} K={K} B={B}"
    _check_loss(tr, loss_ref, what)
    _check_grads(model, grads_ref, what)


# ------------------------------------------------------------------ 4. draws
def _drawn(kind, env, monkeypatch, steps, d=12, B=64, seed=9):
    if env is None:
        monkeypatch.delenv("VPC_STEP_SMALL", raising=False)
    else:
        monkeypatch.setenv("VPC_STEP_SMALL", env)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, d, generator=g).to(DEV)
    m = (torch.rand(B, d, generator=g) < 0.7).to(DEV)
    torch.manual_seed(3)
    model = (eddi.Reg_EDDI(d, 500, 10, 10, TP, "exp", "kl_reg") if kind == "reg" else eddi.vanilla_EDDI(d, 500, 20, 10, TP, "exp")).to(DEV)
    tr = eddi.EDDITrainer(model, seed=seed)
    losses = []
    for s in range(steps):
        tr.step(x, m, epoch=s + 1, alpha=0.5, p_missingness=30)
        losses.append(tr.loss_value())
    return tr, model, losses


@pytest.mark.parametrize("d", [12, 14])
def test_same_draws_on_both_paths(d, monkeypatch):
    """B = 64, seed 9.  d = 12: the kernel's pitch is d and it makes the draws itself; d = 14: the kernel's rows are 16 wide and
    the draws are made on the unpadded rows in front of it.  Either way mask_p bytes and eps planes are the chain's."""
    t1, _, _ = _drawn("reg", None, monkeypatch, 1, d=d)
    t0, _, _ = _drawn("reg", "0", monkeypatch, 1, d=d)
    assert t1.last_path == "small" and t0.last_path == "chain"
    assert torch.equal(t1.mask_p_buf, t0.mask_p_buf)
    assert torch.equal(t1.eps_buf[:2], t0.eps_buf[:2])
    assert t1.rng_offset == t0.rng_offset


def test_device_draw_runs_repeat_bitwise(monkeypatch):
    runs = [_drawn("reg", None, monkeypatch, 8) for _ in range(2)]
    assert runs[0][0].last_path == "small"
    assert runs[0][2][-1] < runs[0][2][0]
    assert runs[0][2] == runs[1][2] and torch.equal(runs[0][1]._flat, runs[1][1]._flat)


# ------------------------------------------------------------------ 5. the two paths agree
@pytest.mark.parametrize("kind", ["reg", "van"])
def test_paths_agree_over_five_steps(kind, monkeypatch):
    """Reg K = 10 and vanilla K = 20 at d = 12, B = 64, device draws (the same on both paths)."""
    t1, m1, l1 = _drawn(kind, None, monkeypatch, 5)
    t0, m0, l0 = _drawn(kind, "0", monkeypatch, 5)
    assert t1.last_path == "small" and t0.last_path == "chain"
    for i, (a, b) in enumerate(zip(l1, l0)):
        print(kind, i, a, b)
        assert abs(a - b) <= 1e-4 * abs(b), (i, a, b)
    for (k, a), b in zip(m1.named_parameters(), m0.parameters()):
        _close(a, b, 5e-5, f"{kind} final {k}")


# ------------------------------------------------------------------ 6. refusals and fall-back
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

    def both(d, d_real, K, x=p, front=p):
        head = (x, p, p, 1, ptrs, None, co, ptrs, None, 1.0, 0.0, p, p, p, nb, 16, d, d_real, 10, K, front, p, p)
        a = l.vpc_step_small_eddi_f32(*head, stream)
        b = l.vpc_step_small_eddi_draw_f32(*head, None, 0.7, p, 256, 0, 0, 0, None, 0, 16, 16, 0, 16, stream)
        assert a == b
        return a

    assert both(12, 12, 33) == 2   # K = 33
    assert both(12, 12, 0) == 2
    assert both(14, 14, 10) == 2   # d not a multiple of 4
    assert both(12, 13, 10) == 2   # d_real > d
    assert both(16, 12, 10) == 2   # d - d_real > 3
    assert both(12, 0, 10) == 2
    assert both(68, 68, 10) == 2   # no instantiation past obs_dim 64
    assert both(16, 14, 10, x=ctypes.c_void_p(p.value + 4)) == 1       # misaligned x
    assert both(16, 14, 10, front=ctypes.c_void_p(p.value + 2)) == 1   # misaligned front-end parameters
    assert both(16, 14, 10, front=None) == 1
    torch.cuda.synchronize()
    assert nbv.value == -1 and not bool(buf.any())


def test_larger_batches_and_ranks_keep_the_chain(monkeypatch):
    monkeypatch.setenv("VPC_STEP_SMALL", "32")  # the row limit
    g = torch.Generator().manual_seed(2)
    x = torch.rand(48, 12, generator=g).to(DEV)
    m = (torch.rand(48, 12, generator=g) < 0.7).to(DEV)
    torch.manual_seed(1)
    model = eddi.Reg_EDDI(12, 500, 10, 10, TP, "exp", "kl_reg").to(DEV)
    tr = eddi.EDDITrainer(model, seed=1)
    tr.step(x, m, epoch=1, alpha=0.5)
    assert tr.last_path == "chain" and np.isfinite(tr.loss_value())
    tr.step(x[:32], m[:32], epoch=1, alpha=0.5)
    assert tr.last_path == "small" and np.isfinite(tr.loss_value())
    tr.step(x, m, epoch=1, alpha=0.5)  # and back, on the same trainer
    assert tr.last_path == "chain" and np.isfinite(tr.loss_value())
    assert not eddi.small_step_route(12, 10, 32, 2, ops.step_small_max_rows())  # world_size > 1: the predicate alone
