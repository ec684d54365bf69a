"""The small-batch step of FlowTrainer (flow.py: _step_small on the few-row layer ops of csrc/vpc_rows.hip), switched on with
VPC_FLOW_SMALL=128 through monkeypatch:
  * at hid 500 against the float64 closed form (tests/flow_oracle.py::step), loss 2e-5 relative and every gradient 2e-4 of
    its max - the bounds of test_flow_gpu.py::test_trainer_hid500_vs_oracle - with seeds at which no spline decision of any
    pass is within FLAG_BIN / FLAG_GATE of a knot in float64 (asserted before the launch), so no element is excluded,
  * the per-pass flag, the golden trajectories, the launch sequence, the routing, device draws, harness.train(model=...)."""
import os

import numpy as np
import pytest
import torch

import flow_oracle as FO
from conftest import load_golden

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 1}
NO_GRAD = ["flow.flows.0.unnormalized_pdf", "flow.flows.1.unnormalized_pdf", "flow.flows.2.unnormalized_pdf",
           "encoder_mean.weight", "encoder_mean.bias", "encoder_logvar.weight", "encoder_logvar.bias",
           "decoder_logvar.0.weight", "decoder_logvar.0.bias"]
SMALL_CALLS = (["vpc_flow_prep"] + ["vpc_rows_fwd"] * 3 + ["vpc_flow_fwd"] + ["vpc_rows_fwd"] * 5 + ["vpc_flow_loss"] +
               ["vpc_rows_bwd"] * 5 + ["vpc_flow_bwd"] + ["vpc_rows_bwd"] * 3 + ["vpc_adam_step"])


@pytest.fixture(scope="module")
def fl():
    import vpc_amd
    from vpc_amd import flow
    return flow


@pytest.fixture
def small(monkeypatch):
    monkeypatch.setenv("VPC_FLOW_SMALL", "128")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, ref, tol, what):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    err = float((got - ref).abs().max() / (ref.abs().max() + 1e-30))
    print(what, f"err {err:.3e} tol {tol:.1e}")
    assert err <= tol, (what, err)


def _rel(got, ref, tol, what):
    print(what, f"got {float(got)!r} ref {float(ref)!r} tol {tol:.1e}")
    assert abs(float(got) - float(ref)) <= tol * abs(float(ref)), (what, float(got), float(ref))


def _load_model(fl, g, cls, prefix="param."):
    model = cls(g["x"].shape[1], int(g["hid"]), 10, 10, TP)
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(prefix)})
    return model.cuda()


# ------------------------------------------------------------------------------------------------ float64 closed form
def _oracle_case(B, d, reg, seed, p_outside=False):
    rng = np.random.default_rng(seed)
    x = rng.random((B, d)).astype(np.float32)
    mask = rng.random((B, d)) < 0.7
    mask_p = mask & (rng.random((B, d)) < 0.7) if reg else None
    eps = rng.standard_normal((2 if reg else 1, B, FO.L)).astype(np.float32)
    if p_outside:
        eps[1] = np.sign(eps[1] + 1e-3) * (1.05 + np.abs(eps[1]))
    return x, mask, mask_p, eps


def _n_flagged(P, x, mask, mask_p, eps):
    """Spline decisions, over every pass, that fp32 may take the other way (the caches as tests/flow_cases.py obtains them:
    flow_fwd on the float64 contexts of the pass)."""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    n = 0
    for k, mk in enumerate([mask] + ([mask_p] if mask_p is not None else [])):
        mk = np.asarray(mk, np.float64)
        ecache, _ = FO.mlp(P, FO.ENC, np.concatenate([np.asarray(x, np.float64) * mk, mk], 1))
        cache = FO.flow_fwd(ecache[-1], np.asarray(eps[k], np.float64))[2]
        if cache is not None:  # (None: a pass without an inside draw takes no decision)
            n += int(FO.flagged(FO.flow_flags(cache)).sum())
    return n


def _small_vs_oracle(fl, d, B, reg, alpha, seed, p_outside=False):
    H = 500
    P = FO.init_params(d, H, seed=seed)
    x, mask, mask_p, eps = _oracle_case(B, d, reg, seed + 1, p_outside)
    assert _n_flagged(P, x, mask, mask_p, eps) == 0, "pick another seed: a spline decision sits on a knot in float64"
    model = (fl.REG_VAEFlow if reg else fl.VAEFlow)(d, H, 10, 10, TP)
    sd = model.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in P.items()})
    model.load_state_dict(sd)
    model.cuda()
    tr = fl.FlowTrainer(model, lr=1e-3)
    tr.grad.fill_(float("nan"))  # (every gradient is written by a rows_bwd launch: nothing is accumulated)
    tr.step(_dev(x), _dev(mask), mask_p=None if mask_p is None else _dev(mask_p), eps=_dev(eps), alpha=alpha)
    assert tr.last_path == "small"
    r = FO.step(P, x, mask, mask_p, eps, alpha=alpha)
    _rel(tr.loss_value(), r["loss"], 2e-5, (d, B, reg))
    flat, off = tr.grad.cpu(), 0
    for k in FO.TRAINABLE:
        n = P[k].size
        _close(flat[off:off + n].view(P[k].shape), torch.from_numpy(r["grads"][k]), 2e-4, (d, B, reg, k))
        off += n
    return tr, r


@pytest.mark.parametrize("d,B", [(12, 1), (12, 37), (12, 64), (128, 64)])
def test_reg_hid500_vs_oracle(fl, small, d, B):
    _small_vs_oracle(fl, d, B, True, 0.5, 100 + d + B)


@pytest.mark.parametrize("d,B", [(12, 37), (12, 128), (128, 100)])
def test_vanilla_hid500_vs_oracle(fl, small, d, B):
    _small_vs_oracle(fl, d, B, False, 0.0, 200 + d + B)


def test_flag_is_per_pass(fl, small):
    """q pass with inside draws, p pass with none: the p pass of the SAME launch is the identity (z = eps exactly,
    z_log_prob = log N(eps)), the q pass is splined; gradients match the oracle."""
    tr, r = _small_vs_oracle(fl, 12, 37, True, 1.0, 7, p_outside=True)
    B = 37
    eps_p = tr.eps[B:].cpu()
    assert bool((eps_p.abs() > 1).all()) and bool((tr.eps[:B].abs() <= 1).any())
    assert torch.equal(tr.z[B:].cpu(), eps_p)
    _close(tr.zlp[B:], -eps_p.double() ** 2 / 2 - FO.HL, 1e-6, "zlp_p")
    assert not torch.equal(tr.z[:B].cpu(), tr.eps[:B].cpu())
    _close(tr.z[:B], torch.from_numpy(r["fwd"]["z_q"]), 2e-5, "z_q")


# ------------------------------------------------------------------------------------------------ golden trajectories
@pytest.mark.parametrize("kind", ["reg", "van"])
def test_trajectory(fl, small, kind):
    """hid 64, B = 37, five Adam steps recorded from the reference; the 9 tensors that never get a gradient are bitwise
    unchanged."""
    g = load_golden(f"flow_traj_{kind}_d12.npz")
    model = _load_model(fl, g, fl.REG_VAEFlow if kind == "reg" else fl.VAEFlow, "param0.")
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if k in NO_GRAD}
    tr = fl.FlowTrainer(model, lr=1e-3)
    x, m = _dev(g["x"]), _dev(g["mask"]).bool()
    total = 0.0
    for s in range(len(g["losses"])):
        tr.step(x, m, mask_p=_dev(g["mask_p"][s]) if kind == "reg" else None, eps=_dev(g["eps"][s]),
                alpha=float(g["alpha"]))
        assert tr.last_path == "small"
        _rel(tr.loss_value(), g["losses"][s], 2e-5, s)
        total += g["losses"][s]
    _rel(tr.epoch_total(), total, 2e-5, "epoch_total")
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith("param5."):
            _close(sd[k[7:]], torch.from_numpy(v), 5e-5, k)
    for k, v in before.items():
        assert torch.equal(sd[k], v), k
        assert torch.equal(v.cpu(), torch.from_numpy(g["param5." + k])), k


# ------------------------------------------------------------------------------------------------ launches, routing
class _Recorder:
    """Stands in for the loaded library: records every vpc_* symbol fetched, hands out the real one."""

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        if name.startswith("vpc_"):
            self.names.append(name)
        return getattr(self.real, name)


def _wine(fl, cls, B, seed=1):
    torch.manual_seed(0)
    model = cls(12, 500, 10, 10, TP).cuda()
    g = torch.Generator().manual_seed(3)
    x, m = torch.rand(B, 12, generator=g).cuda(), (torch.rand(B, 12, generator=g) < 0.6).cuda()
    return fl.FlowTrainer(model, lr=1e-3, seed=seed), x, m


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_launch_sequence(fl, small, kind, monkeypatch):
    """The third step at the wine shape (B = 64, hid 500) is the small path's sequence: prep, 3 rows_fwd, the flow, 5 rows_fwd,
    the loss, 5 rows_bwd, the flow backward, 3 rows_bwd, Adam - 21 calls, 22 launches (vpc_flow_loss is two), against the
    chain's 29 calls; a trainer that only took the small path never allocated the weight-gradient partials."""
    from vpc_amd import _lib
    tr, x, m = _wine(fl, fl.REG_VAEFlow if kind == "reg" else fl.VAEFlow, 64)
    step = lambda: tr.step(x, m, alpha=0.5, p_missingness=30)
    step()
    step()
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    step()
    monkeypatch.setattr(_lib, "_lib", rec.real)
    assert rec.names == SMALL_CALLS and len(SMALL_CALLS) == 21
    assert tr.last_path == "small" and tr._wg is None


def test_routing(fl, monkeypatch):
    monkeypatch.delenv("VPC_FLOW_SMALL", raising=False)
    tr, x, m = _wine(fl, fl.REG_VAEFlow, 64)
    tr.step(x, m, alpha=0.5)
    assert tr.last_path == "chain"
    monkeypatch.setenv("VPC_FLOW_SMALL", "0")
    tr.step(x, m, alpha=0.5)
    assert tr.last_path == "chain"
    monkeypatch.setenv("VPC_FLOW_SMALL", "128")
    tr.step(x, m, alpha=0.5)
    assert tr.last_path == "small"
    monkeypatch.setenv("VPC_FLOW_SMALL", "127")  # R = 128 stacked rows is over this limit
    tr.step(x, m, alpha=0.5)
    assert tr.last_path == "chain"
    monkeypatch.setenv("VPC_FLOW_SMALL", "100000")  # REG at B = 65: R = 130 > the kernels' 128 rows
    tr65, x65, m65 = _wine(fl, fl.REG_VAEFlow, 65)
    tr65.step(x65, m65, alpha=0.5)
    assert tr65.last_path == "chain"
    trv, xv, mv = _wine(fl, fl.VAEFlow, 65)  # (one pass: R = 65)
    trv.step(xv, mv)
    assert trv.last_path == "small"
    import vpc_amd
    monkeypatch.setenv("VPC_FLOW_SMALL", "abc")
    with pytest.raises(vpc_amd.VpcError, match="VPC_FLOW_SMALL"):
        tr.step(x, m, alpha=0.5)


def test_both_paths_draw_the_same(fl, monkeypatch):
    """Same seed and step index: the chain step and the small step read bit-equal eps and mask_p, also when the small step
    follows a chain step on the same trainer."""
    draws = {}
    for order in (("chain", "chain"), ("chain", "small"), ("small", "small")):
        tr, x, m = _wine(fl, fl.REG_VAEFlow, 37, seed=5)
        for s, path in enumerate(order):
            monkeypatch.setenv("VPC_FLOW_SMALL", "128" if path == "small" else "0")
            tr.step(x, m, alpha=0.5, p_missingness=30)
            assert tr.last_path == path
            draws.setdefault(s, []).append((tr.eps.clone(), tr.mask_p.clone()))
    for s, runs in draws.items():
        for eps, mp in runs[1:]:
            assert torch.equal(eps, runs[0][0]) and torch.equal(mp, runs[0][1]), s
    assert not torch.equal(draws[0][0][0], draws[1][0][0])


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_device_draws_reproduce(fl, small, kind):
    """Same seed, two runs of 10 steps: losses and final flat parameters bitwise equal."""
    runs = []
    for _ in range(2):
        tr, x, m = _wine(fl, fl.REG_VAEFlow if kind == "reg" else fl.VAEFlow, 64, seed=11)
        losses = []
        for _s in range(10):
            tr.step(x, m, alpha=0.5, p_missingness=30)
            losses.append(tr.tail[0].clone())
        assert tr.last_path == "small"
        runs.append((torch.stack(losses), tr.model._flat.clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    assert bool(torch.isfinite(runs[0][0]).all())


def test_step_timers_keep_their_names(fl, small):
    tr, x, m = _wine(fl, fl.REG_VAEFlow, 16)
    tr.timers = {}
    tr.step(x, m, alpha=0.5)
    torch.cuda.synchronize()
    assert tr.last_path == "small"
    assert {k: len(v) for k, v in tr.timers.items()} == {"prep": 1, "enc_fwd": 3, "flow": 1, "dec_fwd": 5, "loss": 1,
                                                         "dec_bwd": 5, "flow_bwd": 1, "enc_bwd": 3, "adam": 1}


def test_harness_train(fl, small, tmp_path, monkeypatch):
    """train(model=...) on a 96-row loader with batch 64: the full batch and the shorter last one both take the small path,
    and the checkpoint loads back."""
    import vpc_amd
    from torch.utils.data import DataLoader, TensorDataset
    monkeypatch.chdir(tmp_path)
    paths, step = [], fl.FlowTrainer.step

    def recording_step(self, *a, **kw):
        step(self, *a, **kw)
        paths.append((a[0].shape[0], self.last_path))

    monkeypatch.setattr(fl.FlowTrainer, "step", recording_step)
    torch.manual_seed(0)
    x = torch.rand(96, 12)
    m = torch.rand(96, 12) < 0.7
    loader = DataLoader(TensorDataset(x, m), batch_size=64, shuffle=False)
    for vae_type, cls in (("reg_flow1", fl.REG_VAEFlow), ("vanilla_flow2", fl.VAEFlow)):
        del paths[:]
        torch.manual_seed(1)
        model = cls(12, 64, 10, 10, TP)
        before = {k: v.clone() for k, v in model.state_dict().items()}
        out = vpc_amd.train((loader, None), 50, 12, 64, 10, 1, 10, "toy", TP, "exp", vae_type, 1, 1, max_epochs=1, alpha=0.5,
                            p_missingness=30, reg_type="kl_reg", fused=True, verbose=False, model=model)
        assert out is model
        assert paths == [(64, "small"), (32, "small")]
        ck = vpc_amd.checkpoint_path("exp", "toy", vae_type, 50, 0.5, 30, "kl_reg")
        assert os.path.exists(ck)
        saved = torch.load(ck, weights_only=True)
        assert list(saved) == list(before)
        again = cls(12, 64, 10, 10, TP)
        again.load_state_dict(saved)
        for k, v in again.state_dict().items():
            assert torch.equal(v, model.state_dict()[k].cpu()), (vae_type, k)
            if k in NO_GRAD:
                assert torch.equal(v, before[k]), (vae_type, k)
        assert any(not torch.equal(saved[k], before[k]) for k in FO.TRAINABLE)
