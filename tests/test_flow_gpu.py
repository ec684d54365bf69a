"""GPU parity of the flow path (VAEFlow / REG_VAEFlow, csrc/vpc_flow.hip) through the C ABI:
  * API forward, loss (train and evaluate stages, alpha 1 / 0.5 / 0), every parameter gradient and the llh_eval values
    against vectors recorded from the reference (tests/golden/flow_*.npz), hid 64 and a ragged 72, d 12 and 40,
  * the per-pass torch.any(inside) flag (a p pass with no inside draw), 5-step Adam trajectories on the API path and
    on FlowTrainer (the 9 gradient-free tensors bitwise unchanged),
  * FlowTrainer at hid 500 (d 12 / 128, B 1 / 37 / 64 / 4096) against the float64 oracle (tests/flow_oracle.py),
  * device draws, train(model=...) and eval_vae(model=...) with the reference's file names, the guards.
Tolerances: loss 2e-5 relative, gradients 2e-4 of the tensor's max."""
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


@pytest.fixture(scope="module")
def fl():
    import vpc_amd
    from vpc_amd import flow
    return flow


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, ref, tol, what):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    err = float((got - ref).abs().max() / (ref.abs().max() + 1e-30))
    assert err <= tol, (what, err)


def _rel(got, ref, tol, what):
    assert abs(float(got) - float(ref)) <= tol * abs(float(ref)), (what, float(got), float(ref))


def _load_model(fl, g, cls, prefix="param."):
    model = cls(g["x"].shape[1], int(g["hid"]), 10, 10, TP)
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(prefix)})
    return model.cuda()


def _api(model, x, m, mp, eps, alpha=1.0, stage="train", llh=False):
    """forward with the recorded draws injected + loss, as train.py:77-85 / evaluate.py:189-200."""
    if mp is not None:
        z_q, zlp_q = model._encode(x, m, eps=eps[0])
        z_p, zlp_p = model._encode(x, mp, eps=eps[1])
        xm_q, lv_q = model.decoder(z_q)
        xm_p, lv_p = model.decoder(z_p)
        o = (z_p, zlp_p, xm_p, lv_p, z_q, zlp_q, xm_q, lv_q)
        r = model.loss(x, o[6], o[7], o[4], o[5], o[2], o[3], o[0], o[1], m, mp, alpha, llh_eval=llh, stage=stage)
        return r, o
    z, zlp = model._encode(x, m, eps=eps[0])
    xm, lv = model.decoder(z)
    o = (z, zlp, xm, lv)
    return model.loss(x, o[2], o[3], o[0], o[1], m, llh_eval=llh), o


def _check_grads(model, g, tag):
    pre = f"grad.{tag}."
    names = {k[len(pre):] for k in g if k.startswith(pre)}
    assert names == set(FO.TRAINABLE)
    for k, p in model.named_parameters():
        if k in names:
            _close(p.grad, torch.from_numpy(g[pre + k]), 2e-4, (tag, k))
        else:
            assert p.grad is None, k


@pytest.mark.parametrize("d", [12, 40])
def test_api_reg_vs_reference(fl, d):
    g = load_golden(f"flow_reg_d{d}.npz")
    model = _load_model(fl, g, fl.REG_VAEFlow)
    assert list(model.state_dict()) == list(g["keys"])
    x, m, mp, eps = _dev(g["x"]), _dev(g["mask"]), _dev(g["mask_p"]), _dev(g["eps"])
    stages = [(a, "train", f"a{a}") for a in (1.0, 0.5, 0.0)]
    if "loss.eval" in g:
        stages.append((0.5, "evaluate", "eval"))
    for alpha, stage, tag in stages:
        model.zero_grad(set_to_none=True)
        (pl, tl), o = _api(model, x, m, mp, eps, alpha, stage)
        _rel(tl.item(), g["loss." + tag], 2e-5, tag)
        assert pl is tl or abs(pl.item() - tl.item()) == 0
        tl.backward()
        _check_grads(model, g, tag)
    for n, t in zip(["z_p", "z_log_prob_p", "x_mean_p", "x_logvar_p", "z_q", "z_log_prob_q", "x_mean_q", "x_logvar_q"],
                    o):
        _close(t, torch.from_numpy(g["fwd." + n]), 2e-5, n)
    assert bool((o[3] == -8).all()) and o[3].shape == o[2].shape
    with torch.no_grad():
        for stage in ("train", "evaluate"):
            r, _ = _api(model, x, m, mp, eps, 0.5, stage, llh=True)
            ref = g[f"llh.{stage}"]
            for i in range(4):
                if ref[i] == 0:
                    assert float(r[i]) == 0.0, (stage, i)
                else:
                    _rel(float(r[i]), ref[i], 2e-5, (stage, i))


@pytest.mark.parametrize("d", [12, 40])
def test_api_vanilla_vs_reference(fl, d):
    g = load_golden(f"flow_van_d{d}.npz")
    model = _load_model(fl, g, fl.VAEFlow)
    x, m, eps = _dev(g["x"]), _dev(g["mask"]), _dev(g["eps"])
    (pl, tl), o = _api(model, x, m, None, eps)
    _rel(tl.item(), g["loss"], 2e-5, "train_loss")
    _rel(pl.item(), g["print_loss"], 2e-5, "print_loss")
    tl.backward()
    _check_grads(model, g, "v")
    for n, t in zip(["z", "z_log_prob", "x_mean", "x_logvar"], o):
        _close(t, torch.from_numpy(g["fwd." + n]), 2e-5, n)
    with torch.no_grad():
        r, _ = _api(model, x, m, None, eps, llh=True)
        for i in range(4):
            _rel(float(r[i]), g["llh"][i], 2e-5, i)


def test_api_quirk_pass_without_inside_draw(fl):
    """B = 1, the q pass holds inside and outside draws (and the boundary values +-1), the p pass none: the p pass is
    the identity (z_p = eps_p bit for bit), no gradient reaches its context."""
    g = load_golden("flow_quirk_reg.npz")
    model = _load_model(fl, g, fl.REG_VAEFlow)
    x, m, mp, eps = _dev(g["x"]), _dev(g["mask"]), _dev(g["mask_p"]), _dev(g["eps"])
    for alpha in (1.0, 0.5):
        model.zero_grad(set_to_none=True)
        (_, tl), o = _api(model, x, m, mp, eps, alpha)
        _rel(tl.item(), g[f"loss.a{alpha}"], 2e-5, alpha)
        tl.backward()
        _check_grads(model, g, f"a{alpha}")
    assert torch.equal(o[0].cpu(), torch.from_numpy(g["eps"][1]))
    _close(o[4], torch.from_numpy(g["fwd.z_q"]), 2e-5, "z_q")


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_api_adam_trajectory(fl, kind):
    """model.forward / loss / backward + optim.Adam as train.py:77-117, draws and mask_p injected."""
    g = load_golden(f"flow_traj_{kind}_d12.npz")
    model = _load_model(fl, g, fl.REG_VAEFlow if kind == "reg" else fl.VAEFlow, "param0.")
    model.flatten_parameters()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    x, m = _dev(g["x"]), _dev(g["mask"])
    for s in range(len(g["losses"])):
        mp = _dev(g["mask_p"][s]) if kind == "reg" else None
        (_, tl), _ = _api(model, x, m, mp, _dev(g["eps"][s]), float(g["alpha"]))
        opt.zero_grad()
        tl.backward()
        opt.step()
        _rel(tl.item(), g["losses"][s], 2e-5, s)
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith("param5."):
            _close(sd[k[7:]], torch.from_numpy(v), 5e-5, k)


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_trainer_trajectory(fl, kind):
    """FlowTrainer (stacked q/p GEMMs, gated loss, one wgrad reduction, flat Adam) reproduces the reference's
    trajectory; the 9 tensors that never get a gradient are bitwise unchanged."""
    g = load_golden(f"flow_traj_{kind}_d12.npz")
    model = _load_model(fl, g, fl.REG_VAEFlow if kind == "reg" else fl.VAEFlow, "param0.")
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if k in NO_GRAD}
    tr = fl.FlowTrainer(model, lr=1e-3)
    x, m = _dev(g["x"]), _dev(g["mask"]).bool()
    total = 0.0
    for s in range(len(g["losses"])):
        tr.step(x, m, mask_p=_dev(g["mask_p"][s]) if kind == "reg" else None, eps=_dev(g["eps"][s]),
                alpha=float(g["alpha"]))
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


def _oracle_case(B, d, reg, seed, p_outside=False):
    rng = np.random.default_rng(seed)
    x = rng.random((B, d)).astype(np.float32)
    mask = rng.random((B, d)) < 0.7
    mask_p = mask & (rng.random((B, d)) < 0.7) if reg else None
    eps = rng.standard_normal((2 if reg else 1, B, FO.L)).astype(np.float32)
    if p_outside:
        eps[1] = np.sign(eps[1] + 1e-3) * (1.05 + np.abs(eps[1]))
    return x, mask, mask_p, eps


def _trainer_vs_oracle(fl, d, B, reg, alpha, seed, p_outside=False):
    H = 500
    P = FO.init_params(d, H, seed=seed)
    x, mask, mask_p, eps = _oracle_case(B, d, reg, seed + 1, p_outside)
    model = (fl.REG_VAEFlow if reg else fl.VAEFlow)(d, H, 10, 10, TP)
    sd = model.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in P.items()})
    model.load_state_dict(sd)
    model.cuda()
    tr = fl.FlowTrainer(model, lr=1e-3)
    tr.step(_dev(x), _dev(mask), mask_p=None if mask_p is None else _dev(mask_p), eps=_dev(eps), alpha=alpha)
    r = FO.step(P, x, mask, mask_p, eps, alpha=alpha)
    _rel(tr.loss_value(), r["loss"], 2e-5, (d, B, reg))
    flat, off = tr.grad.cpu(), 0
    for k in FO.TRAINABLE:
        n = P[k].size
        _close(flat[off:off + n].view(P[k].shape), torch.from_numpy(r["grads"][k]), 2e-4, (d, B, reg, k))
        off += n
    return tr, r


@pytest.mark.parametrize("d", [12, 128])
@pytest.mark.parametrize("B", [1, 37, 64, 4096])
def test_trainer_hid500_vs_oracle(fl, d, B):
    _trainer_vs_oracle(fl, d, B, True, 0.5, 100 + d + B)
    if B in (37, 4096):
        _trainer_vs_oracle(fl, d, B, False, 0.0, 200 + d + B)


def test_flag_is_per_pass(fl):
    """q pass with inside draws, p pass with none: the p pass of the SAME launch is the identity (z = eps exactly,
    z_log_prob = log N(eps)), the q pass is splined; gradients match the oracle."""
    tr, r = _trainer_vs_oracle(fl, 12, 37, True, 1.0, 7, p_outside=True)
    B = 37
    eps_p = tr.eps[B:].cpu()
    assert bool((eps_p.abs() > 1).all()) and bool((tr.eps[:B].abs() <= 1).any())
    assert torch.equal(tr.z[B:].cpu(), eps_p)
    _close(tr.zlp[B:], -eps_p.double() ** 2 / 2 - FO.HL, 1e-6, "zlp_p")
    assert not torch.equal(tr.z[:B].cpu(), tr.eps[:B].cpu())
    _close(tr.z[:B], torch.from_numpy(r["fwd"]["z_q"]), 2e-5, "z_q")


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_trainer_device_draws(fl, kind):
    """Device draws: eps ~ N(0, 1) moments, mask_p a sub-mask of mask with P(keep) = 0.7, a seed reproduces the run
    bit for bit, and the loss goes down."""
    cls = fl.REG_VAEFlow if kind == "reg" else fl.VAEFlow
    B, d = 4096, 12
    gen = torch.Generator(device="cuda").manual_seed(2)
    x = torch.rand(B, d, device="cuda", generator=gen)
    m = torch.rand(B, d, device="cuda", generator=gen) < 0.6
    runs = []
    for _ in range(2):
        torch.manual_seed(7)
        model = cls(d, 64, 10, 10, TP).cuda()
        tr = fl.FlowTrainer(model, lr=3e-3, seed=11)
        losses = []
        for s in range(30):
            tr.step(x, m, alpha=0.5, p_missingness=30)
            if s == 0:
                e = tr.eps.double()
                assert abs(float(e.mean())) < 0.02 and abs(float(e.var()) - 1) < 0.03, (float(e.mean()), float(e.var()))
                assert abs(float((e.abs() <= 1).double().mean()) - 0.6827) < 0.01
                if kind == "reg":
                    mp = tr.mask_p != 0
                    assert bool((mp <= m).all())
                    keep = float(mp.sum()) / float(m.sum())
                    assert abs(keep - 0.7) < 0.02, keep
            losses.append(tr.loss_value())
        runs.append((losses, model._flat.clone(), tr.eps.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    ls = runs[0][0]
    assert np.mean(ls[-5:]) < np.mean(ls[:5]), ls


def test_guards(fl):
    import vpc_amd
    with pytest.raises(vpc_amd.VpcError):
        fl.VAEFlow(12, 64, 10, 11, TP)
    with pytest.raises(vpc_amd.VpcError):
        fl.REG_VAEFlow(12, 64, 10, 11, TP)
    cpu = fl.VAEFlow(12, 64, 10, 10, TP)
    with pytest.raises(vpc_amd.VpcError):
        cpu.forward(torch.rand(4, 12), torch.ones(4, 12))
    model = fl.REG_VAEFlow(12, 64, 10, 10, TP).cuda()
    x, m = torch.rand(4, 12, device="cuda"), torch.ones(4, 12, device="cuda")
    with pytest.raises(vpc_amd.VpcError):
        model.forward(x.cpu(), m.cpu(), m.cpu())
    with pytest.raises(NotImplementedError):
        model.encoder(x, m, sample=False)
    with pytest.raises(NotImplementedError):
        model.backward(torch.zeros(4, 10, device="cuda"), x, m)
    with pytest.raises(vpc_amd.VpcError):
        fl.FlowTrainer(model, world_size=2, rank=0)
    with pytest.raises(NotImplementedError):
        vpc_amd.active_learning_func(None, x, m.bool(), 50, 12, 64, 10, 2, 10, "toy", TP, "exp", "reg_flow1", 1, 1, 1,
                                     model=model, save=False)


def test_harness_train_flow(fl, tmp_path, monkeypatch):
    """train(model=...) for both flow names, fused (FlowTrainer) and API path: reference-named checkpoints that load
    back into the reference's classes' state_dict layout."""
    import vpc_amd
    from torch.utils.data import DataLoader, TensorDataset
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    x = torch.rand(96, 12)
    m = torch.rand(96, 12) < 0.7
    loader = DataLoader(TensorDataset(x, m), batch_size=32, shuffle=False)
    for vae_type, cls in (("reg_flow1", fl.REG_VAEFlow), ("vanilla_flow2", fl.VAEFlow)):
        for fused in (True, False):
            torch.manual_seed(1)
            model = cls(12, 64, 10, 10, TP)
            before = {k: v.clone() for k, v in model.state_dict().items()}
            out = vpc_amd.train((loader, None), 50, 12, 64, 10, 1, 10, "toy", TP, "exp", vae_type, 1, 1,
                                max_epochs=2, alpha=0.5, p_missingness=30, reg_type="kl_reg", fused=fused,
                                verbose=False, model=model)
            assert out is model
            ck = vpc_amd.checkpoint_path("exp", "toy", vae_type, 50, 0.5, 30, "kl_reg")
            fam = "reg_flow" if vae_type.startswith("reg") else "vanilla_flow"
            assert ck.split(os.sep)[-2] == fam and os.path.exists(ck)
            saved = torch.load(ck, weights_only=True)
            assert list(saved) == list(before)
            again = cls(12, 64, 10, 10, TP)
            again.load_state_dict(saved)
            for k, v in again.state_dict().items():
                assert torch.equal(v, model.state_dict()[k].cpu()), (vae_type, fused, k)
                if k in NO_GRAD:
                    assert torch.equal(v, before[k]), (vae_type, fused, k)
            assert any(not torch.equal(saved[k], before[k]) for k in FO.TRAINABLE)


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_eval_vae_flow_interop(fl, kind, tmp_path, monkeypatch):
    """eval_vae(model=...) (evaluate.py:189-200) on the reference's checkpoint: the four result files under the
    reference's names, each value within the spread of what the reference wrote over six seeds."""
    import vpc_amd
    g = load_golden(f"flow_eval_{kind}_d12.npz")
    vae_type = "reg_flow1" if kind == "reg" else "vanilla_flow1"
    monkeypatch.chdir(tmp_path)
    model = _load_model(fl, g, fl.REG_VAEFlow if kind == "reg" else fl.VAEFlow)
    x, mask = torch.from_numpy(g["x"]), torch.from_numpy(g["mask"])
    loaders = [([(x[:24], mask[:24]), (x[24:], mask[24:])], "test")]
    torch.manual_seed(0)
    res = vpc_amd.eval_vae(loaders, 40, 12, int(g["hid"]), 10, int(g["M"]), 10, "toy", TP, "exp", vae_type, 100, 1, 1,
                           alpha=0.5, p_missingness=30, reg_type="kl_reg", model=model)["test"]
    files = sorted(os.path.join(sub, f) for sub in ("rest", "elbos")
                   for f in os.listdir(os.path.join("experiments", "exp", "toy", sub, "".join(
                       c for c in vae_type if not c.isdigit()))))
    assert [os.path.basename(f) for f in files] == [str(s) for s in g["result_files"]]
    # result_files order: sorted (rest/..., elbos/...) paths as the fixture generator lists them
    by_name = {"vae_elbo": "elbo", "negative_llh_q_imputed": "negll_imp", "negative_llh_imputed": "negll_imp",
               "negative_llh_q": "negll", "negative_llh": "negll", "rmse": "rmse"}
    for i, name in enumerate(g["result_files"]):
        key = next(v for k, v in by_name.items() if f"_{k}_" in str(name))
        ref = g["values"][:, i]
        lo, hi = ref.min() - 3 * ref.std() - 1e-3 * abs(ref.mean()), ref.max() + 3 * ref.std() + 1e-3 * abs(ref.mean())
        got = float(res[key])
        assert lo <= got <= hi, (str(name), got, ref)
