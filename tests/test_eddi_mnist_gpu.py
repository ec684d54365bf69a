"""GPU parity of the MNIST point-net pair (Reg_EDDI_mnist / vanilla_EDDI_mnist, eddi_mnist.py + the vpc_eddiw_* kernels of csrc/vpc_eddi.hip) against
vectors captured from the reference itself (tests/golden/eddi_mnist_*.npz) and the float64 closed form of
tests/eddi_mnist_oracle.py.

Tolerances are the project's existing ones for fp32 against reference goldens (README, row "loss / gradient parity"): loss
2e-5 relative, gradients 2e-4 of the tensor's maximum (the goldens store that maximum beside the strided sample of the five
large matrices), forward outputs 2e-5 of max(1, max).  The front end alone is held to the bounds tests/test_eddi_gpu.py holds
the d <= 128 kernels to (agg 1e-5, gradients 2e-5 of max(1, max)) at every width: a blocked fp32 sum of n terms has a relative
error of about sqrt(n) 2^-24 (6e-6 at the n = 4096 x 1024 terms of the largest case) against the float64 oracle.
"""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

TP = {"batch_size": 64, "patience": 1}
LOSS_TOL, GRAD_TOL, FWD_TOL = 2e-5, 2e-4, 2e-5
TAGS = (("kl0.5", "kl_reg", 0.5), ("kl1.0", "kl_reg", 1.0), ("ml0.8", "ml_reg", 0.8))


@pytest.fixture(scope="module")
def em():
    import vpc_amd
    from vpc_amd import eddi_mnist
    return eddi_mnist


@pytest.fixture(scope="module")
def MO():
    import eddi_mnist_oracle
    return eddi_mnist_oracle


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(a, b, tol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    print(f"{what}: max abs err {err:.3e} (scale {scale:.3e}, tol {tol:.1e})")
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} (scale {scale:.3e})"


def _model(em, g, reg_type=None, seed_key="seed"):
    d = g["x"].shape[1]
    torch.manual_seed(int(g[seed_key]))
    if reg_type is not None:
        return em.Reg_EDDI_mnist(d, 500, int(g["K"]), int(g["L"]), TP, "exp", reg_type).cuda()
    return em.vanilla_EDDI_mnist(d, 500, int(g["K"]), int(g["L"]), TP, "exp").cuda()


def _grad_check(MO, named_grads, g, tag):
    for k, gr in named_grads:
        ref = g.get(f"grad.{tag}.{k}")
        if ref is None:
            continue
        assert gr is not None, k
        got = MO.stored(k, gr.detach().cpu().numpy())
        gmax = float(g[f"gmax.{tag}.{k}"])
        err = float(np.max(np.abs(got.astype(np.float64) - ref)))
        print(f"grad {tag} {k}: max abs err {err:.3e} of max {gmax:.3e} = {err / max(gmax, 1e-30):.2e}")
        assert err <= GRAD_TOL * gmax, (tag, k, err, gmax)


def _loss_close(got, ref, what):
    got, ref = float(got.detach() if torch.is_tensor(got) else got), float(ref)
    print(f"{what}: {got!r} vs {ref!r} rel {abs(got - ref) / max(abs(ref), 1e-30):.2e}")
    assert abs(got - ref) <= LOSS_TOL * abs(ref), (what, got, ref)


def _with_randn(draws, fn):
    it = iter(draws)
    orig = torch.randn
    torch.randn = lambda *a, **k: next(it)
    try:
        return fn()
    finally:
        torch.randn = orig


# ------------------------------------------------------------------------------------------------ front end alone
def _front_case(em, MO, B, d, K, two):
    rng = np.random.default_rng(1000 * d + 10 * K + B + int(two))
    x = rng.random((B, d), dtype=np.float32)
    m = rng.random((B, d)) < 0.6
    E, tb = rng.normal(size=(d, K)).astype(np.float32), rng.normal(size=(d, 1)).astype(np.float32)
    Wp, cp = rng.normal(size=(K, 2 + K)).astype(np.float32) * 0.3, rng.normal(size=K).astype(np.float32) * 0.3
    # entries within 1e-4 of a ReLU kink are unobserved in this data (0.3 % of them): fp32 and float64 may gate them
    # differently, and the derivative is not defined there
    m &= ~MO.front_near_kink(x, E, tb, Wp, cp)
    m[0] = False  # an all-zero mask row: agg = 0, no gradient from it
    if B > 1:
        m[1] = True  # an all-one mask row
    m2 = m & (rng.random((B, d)) < 0.7)
    R = 2 * B if two else B
    dagg = rng.normal(size=(R, K)).astype(np.float32)
    agg_ref, gr = MO.front_chunked(x, m, E, tb, Wp, cp, dagg[:B])
    if two:
        a2, g2 = MO.front_chunked(x, m2, E, tb, Wp, cp, dagg[B:])
        agg_ref = np.concatenate([agg_ref, a2], 0)
        gr = {k: gr[k] + g2[k] for k in gr}
    xd, mu8 = _dev(x), _dev(m.astype(np.uint8))
    m2u8 = _dev(m2.astype(np.uint8)) if two else None
    Ed, tbd, Wpd, cpd = _dev(E), _dev(tb), _dev(Wp), _dev(cp)
    AC = torch.empty(2, K, d, device="cuda")
    em.eddiw_fold(Ed, tbd, Wpd, cpd, AC, d, K)
    agg = torch.full((R, K), float("nan"), device="cuda")
    em.eddiw_front_fwd(xd, mu8, AC, agg, B, d, K, mask2_u8=m2u8)
    what = f"B={B} d={d} K={K} masks={2 if two else 1}"
    _close(agg, torch.from_numpy(agg_ref), 1e-5, f"agg {what}")
    assert float(agg[0].abs().max()) == 0.0
    outs = []
    for _ in range(2):
        gs = [torch.full(s, float("nan"), device="cuda") for s in ((d, K), (d, 1), (K, 2 + K), (K,))]
        em.eddiw_front_bwd(xd, mu8, AC, _dev(dagg), Ed, tbd, Wpd, *gs, B, d, K, mask2_u8=m2u8)
        outs.append(gs)
    for a, b in zip(*outs):
        assert torch.equal(a, b), "front_bwd is not bitwise reproducible"
    for got, key in zip(outs[0], ("type_pars1", "type_bias1", "pnp_encoder1.0.weight", "pnp_encoder1.0.bias")):
        _close(got, torch.from_numpy(gr[key]), 2e-5, f"{key} {what}")


@pytest.mark.parametrize("K", [1, 7, 20, 32])
@pytest.mark.parametrize("d", [1, 127, 128, 129, 200, 784, 1024])
def test_front_end_vs_closed_form(em, MO, d, K):
    for B in (1, 37, 4096):
        for two in (False, True):
            _front_case(em, MO, B, d, K, two)


def test_front_end_all_zero_mask(em):
    B, d, K = 37, 784, 20
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, d, generator=g).cuda()
    E, tb = torch.randn(d, K, generator=g).cuda(), torch.randn(d, 1, generator=g).cuda()
    Wp, cp = torch.randn(K, 2 + K, generator=g).cuda(), torch.randn(K, generator=g).cuda()
    m = torch.zeros(B, d, dtype=torch.uint8, device="cuda")
    AC = torch.empty(2, K, d, device="cuda")
    em.eddiw_fold(E, tb, Wp, cp, AC, d, K)
    agg = torch.full((B, K), float("nan"), device="cuda")
    em.eddiw_front_fwd(x, m, AC, agg, B, d, K)
    assert float(agg.abs().max()) == 0.0
    gs = [torch.full(s, float("nan"), device="cuda") for s in ((d, K), (d, 1), (K, 2 + K), (K,))]
    em.eddiw_front_bwd(x, m, AC, torch.randn(B, K, device="cuda"), E, tb, Wp, *gs, B, d, K)
    for t in gs:
        assert float(t.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ API path against the reference
@pytest.mark.parametrize("d", [784, 200])
def test_reg_against_reference(em, MO, d):
    g = load_golden(f"eddi_mnist_reg_d{d}.npz")
    B = g["x"].shape[0]
    # d = 784: given as images, [B, 28, 28] - forward and loss reshape (VAE.py:97-99, 188-190)
    shp = (B, 28, 28) if d == 784 else (B, d)
    x, m, mp = _dev(g["x"]).reshape(shp), _dev(g["mask"]).reshape(shp), _dev(g["mask_p"]).reshape(shp)
    names = ["mean_p", "logvar_p", "x_mean_p", "x_logvar_p", "mean_q", "logvar_q", "x_mean_q", "x_logvar_q"]
    for tag, rt, alpha in TAGS:
        model = _model(em, g, rt)

        def run():
            o = model.forward(x, m, mp, "train")
            r = model.loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], m, mp, 1400, beta=0.9, alpha=alpha,
                           beta_annealing=(tag == "kl1.0"), llh_eval=True)
            return o, r
        o, r = _with_randn([_dev(g["eps_q"]), _dev(g["eps_p"]), _dev(g["eps_ml"])], run)
        for n, t in zip(names, o):
            _close(t.reshape(g["fwd." + n].shape), torch.from_numpy(g["fwd." + n]), FWD_TOL, f"{tag} {n}")
        assert o[3].shape == (1,)
        _loss_close(r[1], g[f"loss.{tag}"], f"loss {tag}")
        _loss_close(r[2], g[f"re.{tag}"], f"RE_q {tag}")
        assert float(r[3]) == float(g[f"re_imp.{tag}"]) == 0.0  # VAE.py:148
        r[1].backward()
        _grad_check(MO, [(k, p.grad) for k, p in model.named_parameters()], g, tag)
        assert model.prior_mean.grad is None and model.prior_std.grad is None
    with torch.no_grad():
        r = model.loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], m, mp, 7, llh_eval=True, stage="evaluate")
    for got, key in zip(r[1:], ("eval_loss", "eval_re", "eval_re_imp")):
        _loss_close(got, g[key], key)


def test_vanilla_against_reference(em, MO):
    g = load_golden("eddi_mnist_van_d784.npz")
    model = _model(em, g)
    B = g["x"].shape[0]
    x, m = _dev(g["x"]).reshape(B, 1, 28, 28), _dev(g["mask"]).float().reshape(B, 1, 28, 28)
    o = _with_randn([_dev(g["eps_q"])], lambda: model.forward(x, m))
    for n, t in zip(["mean", "logvar", "x_mean", "x_logvar"], o):
        _close(t.reshape(g["fwd." + n].shape), torch.from_numpy(g["fwd." + n]), FWD_TOL, n)
    r = model.loss(x, o[2], o[3], o[0], o[1], 3, m, beta=0.8, llh_eval=True)
    for got, key in zip(r[1:], ("loss", "re", "re_imp")):  # re_imp in the 'train' stage too: VAE.py:294-295
        _loss_close(got, g[key], key)
    r[1].backward()
    _grad_check(MO, [(k, p.grad) for k, p in model.named_parameters()], g, "v")
    # a bool mask gives the same numbers (the vanilla class takes both, VAE.py:294)
    r2 = model.loss(x, o[2].detach(), o[3], o[0].detach(), o[1].detach(), 3, m.bool(), beta=0.8, llh_eval=True)
    assert abs(float(r2[1]) - float(r[1])) <= 1e-6 * abs(float(r[1])) and abs(float(r2[3]) - float(r[3])) <= 1e-6 * abs(float(r[3]))


def test_empty_batch_and_encoder_decoder_shapes(em):
    model = em.Reg_EDDI_mnist(784, 500, 20, 6, TP, "exp", "kl_reg").cuda()
    z, mean, lv = model.encoder(torch.empty(0, 784, device="cuda"), torch.empty(0, 784, device="cuda"))
    assert z.shape == mean.shape == lv.shape == (0, 10) and not z.is_cuda  # VAE.py:66-67: ten columns, CPU
    x, m = torch.rand(5, 784, device="cuda"), torch.rand(5, 784, device="cuda") < 0.5
    z, mean, lv = model.encoder(x, m, sample=False)
    assert torch.equal(z, mean) and mean.shape == lv.shape == (5, 6)
    xm, xlv = model.decoder(z)
    assert xm.shape == (5, 784) and xlv.shape == (1,) and abs(float(xlv) - np.log(0.02)) < 1e-6


# ------------------------------------------------------------------------------------------------ trajectories
def _traj_check(MO, model, g):
    sd = model.state_dict()
    for k in MO.KEYS:
        ref = g["param5." + k]
        got = MO.stored(k, sd[k].detach().cpu().numpy())
        err = float(np.max(np.abs(got - ref)))
        print(f"final {k}: max abs err {err:.3e}")
        assert err <= 5e-5 * max(1.0, float(np.abs(ref).max())), (k, err)  # tests/test_eddi_gpu.py's trajectory bound
    assert torch.equal(sd["prior_mean"].cpu(), torch.zeros(int(g["L"])))
    assert torch.equal(sd["prior_std"].cpu(), torch.ones(int(g["L"])))


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_adam_trajectory_api_path(em, MO, kind):
    g = load_golden(f"eddi_mnist_traj_{kind}_d784.npz")
    model = _model(em, g, "kl_reg" if kind == "reg" else None)
    model.flatten_parameters()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    x, m = _dev(g["x"]), _dev(g["mask"])
    for s in range(len(g["losses"])):
        def run():
            if kind == "reg":
                mp = _dev(g["mask_p"][s])
                o = model.forward(x, m, mp, stage="train")
                return model.loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], m, mp, s + 1, alpha=0.5)[1]
            mf = m.float()
            o = model.forward(x, mf)
            return model.loss(x, o[2], o[3], o[0], o[1], s + 1, mf)[1]
        tl = _with_randn([_dev(e) for e in g["eps"][s]], run)
        opt.zero_grad()
        tl.backward()
        opt.step()
        _loss_close(tl, g["losses"][s], f"step {s}")
    _traj_check(MO, model, g)


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_trainer_trajectory(em, MO, kind):
    g = load_golden(f"eddi_mnist_traj_{kind}_d784.npz")
    model = _model(em, g, "kl_reg" if kind == "reg" else None)
    tr = em.EDDIMnistTrainer(model, lr=1e-3)
    x, m = _dev(g["x"]).reshape(-1, 28, 28), _dev(g["mask"]).reshape(-1, 28, 28)
    for s in range(len(g["losses"])):
        eps = _dev(g["eps"][s])
        tr.step(x, m, mask_p=_dev(g["mask_p"][s]) if kind == "reg" else None, eps=eps, epoch=s + 1, alpha=0.5)
        _loss_close(tr.loss_value(), g["losses"][s], f"step {s}")
    _traj_check(MO, model, g)
    # the API path sees the updated weights
    with torch.no_grad():
        sd = model.state_dict()
        z = torch.randn(4, int(g["L"]), device="cuda")
        h = z
        for i in (0, 2, 4):
            h = torch.relu(torch.nn.functional.linear(h, sd[f"seq_decoder.{i}.weight"], sd[f"seq_decoder.{i}.bias"]))
        ref = torch.sigmoid(torch.nn.functional.linear(h, sd["seq_decoder.6.weight"], sd["seq_decoder.6.bias"]))
        _close(model.decoder(z)[0], ref, FWD_TOL, "decoder after trainer steps")


@pytest.mark.parametrize("tag,rt,alpha", TAGS)
def test_trainer_step_against_reference_gradients(em, MO, tag, rt, alpha):
    """One trainer step on the d = 784 golden: loss and every gradient (read from the flat bucket) against the reference."""
    g = load_golden("eddi_mnist_reg_d784.npz")
    model = _model(em, g, rt)
    tr = em.EDDIMnistTrainer(model, lr=1e-3)
    eps = _dev(np.stack([g["eps_q"], g["eps_p"]]))
    tr.step(_dev(g["x"]), _dev(g["mask"]), mask_p=_dev(g["mask_p"]), eps=eps, eps_ml=_dev(g["eps_ml"]), epoch=1400, beta=0.9,
            alpha=alpha, beta_annealing=(tag == "kl1.0"))
    _loss_close(tr.loss_value(), g[f"loss.{tag}"], f"trainer loss {tag}")
    _grad_check(MO, [(k, p.grad) for k, p in model.named_parameters() if p.requires_grad], g, tag)


@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("B", [1, 37, 64, 4096])
def test_trainer_vs_float64_oracle(em, MO, B, kind):
    """One trainer step against the float64 closed form: loss 2e-5 relative, every gradient 2e-4 of the tensor's maximum.
    ReLU has no derivative at 0, and at B = 4096 a step evaluates 2 x 10^7 hidden units: a few pre-activations lie closer to 0
    than fp32 can resolve (measured on the reg inputs: float64 pre-activation 2.2e-7 at row 3326, unit 308 of seq_decoder.4,
    whose pre-activations average 0.078; 2.7e-8 at row 3914, unit 453 of seq_decoder.2 in the p pass, which the fp32 CPU port
    gates the same way as the device), and a unit gated the other way moves one row of a weight gradient by that batch row's
    whole term (5.079e-4 of a maximum 0.9383 in seq_decoder.4.weight row 308, 1.5e-7 in all its other rows) - a comparison
    against float64 is not defined there.  So the oracle takes the gate the step itself took for the units whose float64
    pre-activation lies inside MO.kink_band() (2 sqrt(n) 2^-24 of the dot product's magnitude sum) and its own pre > 0
    everywhere else; the number of units in the band and of gates taken over is printed and bounded.  The front end's gates
    stay the oracle's own."""
    d, K, Ld = 784, 20, 10
    torch.manual_seed(5)
    model = (em.Reg_EDDI_mnist(d, 500, K, Ld, TP, "exp", "kl_reg") if kind == "reg" else
             em.vanilla_EDDI_mnist(d, 500, K, Ld, TP, "exp"))
    p = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.cuda()
    gen = torch.Generator().manual_seed(B)
    x = torch.rand(B, d, generator=gen)
    m = torch.rand(B, d, generator=gen) < 0.7
    mp = m & (torch.rand(B, d, generator=gen) < 0.7) if kind == "reg" else None
    eps = torch.randn(2 if kind == "reg" else 1, B, Ld, generator=gen)
    tr = em.EDDIMnistTrainer(model, lr=1e-3)
    tr.step(x.cuda(), m.cuda(), mask_p=None if mp is None else mp.cuda(), eps=eps.cuda(), epoch=1, alpha=0.5)
    gates = {}
    for p_ in range(eps.shape[0]):
        rows = slice(p_ * B, (p_ + 1) * B)
        for i, name in enumerate(("pnp_encoder2.0", "pnp_encoder2.2", "pnp_encoder2.4")):
            gates[(p_, name)] = (tr.enc[i + 1][rows] > 0).cpu().numpy()
        for i, name in enumerate(("seq_decoder.0", "seq_decoder.2", "seq_decoder.4")):
            gates[(p_, name)] = (tr.dec[i + 1][rows] > 0).cpu().numpy()
    stats = {}
    ref, gr = MO.closed_form_step(p, Ld, x.numpy(), m.numpy(), None if mp is None else mp.numpy(), eps.numpy(), alpha=0.5,
                                  device_gates=gates, stats=stats)
    units = eps.shape[0] * B * 2400  # hidden ReLU units of one step: 500 + 500 + 200 + 200 + 500 + 500 per row and pass
    print(f"B={B} {kind}: {stats['in_band']} of {units} units inside the kink band, {stats['taken_from_device']} gated as the step did")
    assert stats["in_band"] <= 1e-4 * units + 2 and stats["taken_from_device"] <= stats["in_band"]
    _loss_close(tr.loss_value(), ref, f"loss B={B}")
    for k, prm in model.named_parameters():
        if k in gr:
            r = gr[k].reshape(prm.shape)
            gmax = float(np.abs(r).max())
            err = float(np.max(np.abs(prm.grad.detach().cpu().numpy().astype(np.float64) - r)))
            print(f"grad {k} B={B}: err {err:.3e} of max {gmax:.3e} = {err / max(gmax, 1e-30):.2e}")
            assert err <= GRAD_TOL * gmax, (k, err, gmax)


def test_trainer_device_draws(em):
    torch.manual_seed(2)
    B, d, K = 64, 784, 20
    x = torch.rand(B, 28, 28, device="cuda")
    m = torch.rand(B, 28, 28, device="cuda") < 0.7
    finals = []
    for rep in range(2):
        torch.manual_seed(3)
        model = em.Reg_EDDI_mnist(d, 500, K, 10, TP, "exp", "kl_reg").cuda()
        tr = em.EDDIMnistTrainer(model, seed=9)
        losses = []
        for s in range(8):
            tr.step(x, m, epoch=s + 1, alpha=0.5, p_missingness=30)
            losses.append(tr.loss_value())
        assert losses[-1] < losses[0]
        finals.append((losses, model._flat.clone()))
        mpb, mu = tr.mask_p_buf.bool(), m.reshape(B, d)
        assert not bool((mpb & ~mu).any())  # mask_p <= mask
        n = int(mu.sum())
        keep = int(mpb.sum()) / n
        assert abs(keep - 0.7) <= 3.0 * np.sqrt(0.7 * 0.3 / n), keep  # binomial 3-sigma band
    assert finals[0][0] == finals[1][0] and torch.equal(finals[0][1], finals[1][1])


# ------------------------------------------------------------------------------------------------ harness
def test_harness_train_and_eval_mnist(em, tmp_path, monkeypatch, capsys):
    """train() (train.py:13-133, data_type == 'mnist') fused and on the API path, checkpoint under the reference's name,
    model_loader('test', ...) and eval_vae (evaluate.py:136-297) for both classes; the UCI EDDI path beside it is untouched."""
    import re
    import vpc_amd
    from torch.utils.data import DataLoader, TensorDataset
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    x = torch.rand(96, 28, 28)
    m = torch.rand(96, 28, 28) < 0.7
    loader = DataLoader(TensorDataset(x, m), batch_size=32, shuffle=False)
    tp = {"batch_size": 32, "patience": 1}
    for vae_type in ("reg_EDDI1", "vanilla_EDDI1", "vanilla_EDDI_with_drop1"):
        cls = vpc_amd.Reg_EDDI_mnist if "reg" in vae_type else vpc_amd.vanilla_EDDI_mnist
        for fused in (True, False):
            torch.manual_seed(1)
            capsys.readouterr()
            model = vpc_amd.train((loader, None), 30, 784, 500, 20, 1, 10, "mnist", tp, "exp", vae_type, 1, 1, max_epochs=2,
                                  alpha=0.5, p_missingness=30, reg_type="kl_reg", fused=fused)
            totals = [float(v) for v in re.findall(r"Total Loss: ([-0-9.e+]+)", capsys.readouterr().out)]
            assert type(model) is cls and len(totals) == 2 and totals[1] < totals[0], (vae_type, fused, totals)
            ck = vpc_amd.checkpoint_path("exp", "mnist", vae_type, 30, alpha=0.5, p_missingness=30, reg_type="kl_reg")
            assert os.path.exists(ck)
            if "vanilla" in vae_type:
                assert os.path.basename(ck) == f"checkpoint_{vae_type}_30_missing_rate_test.pt"
            else:
                assert os.path.basename(ck) == f"checkpoint_{vae_type}_0.5_30_kl_reg_30_missing_rate_full_reg_test.pt"
            loaded = vpc_amd.model_loader("test", 784, 500, 20, 10, 30, "mnist", tp, 2, 1, 1, "exp", "kl_reg", vae_type,
                                          alpha=0.5, p_missingness=30)
            assert type(loaded) is cls
            for k, v in model.state_dict().items():
                assert torch.equal(loaded.state_dict()[k], v.cpu()), k
            res = vpc_amd.eval_vae([(loader, "test")], 30, 784, 500, 20, 2, 10, "mnist", tp, "exp", vae_type, 2, 1, 1,
                                   alpha=0.5, p_missingness=30, reg_type="kl_reg")
            r = res["test"]
            assert all(torch.isfinite(v) for v in r.values()) and 0.05 < float(r["rmse"]) < 0.7
            paths = vpc_amd.result_paths("exp", "mnist", vae_type, "test", 30, 0.5, 30, "kl_reg")
            assert len(paths) == 4 and all(os.path.exists(p) for p in paths.values())
            os.remove(ck)
    x14, m14 = torch.rand(96, 14), torch.rand(96, 14) < 0.7
    l14 = DataLoader(TensorDataset(x14, m14), batch_size=32, shuffle=False)
    uci = vpc_amd.train((l14, None), 30, 14, 500, 10, 1, 10, "toy", tp, "exp", "reg_EDDI1", 1, 1, max_epochs=1, alpha=0.5,
                        reg_type="kl_reg", verbose=False, save=False)
    assert type(uci) is vpc_amd.Reg_EDDI


def test_guards(em):
    import vpc_amd
    model = em.Reg_EDDI_mnist(784, 500, 20, 10, TP, "exp", "kl_reg").cuda()
    x, m = torch.rand(4, 784, device="cuda"), torch.rand(4, 784, device="cuda") < 0.5
    with pytest.raises(vpc_amd.VpcError, match="not supported"):
        vpc_amd.reward_matrix(model, x, m, torch.rand(3, 4, 784, device="cuda"))
    with pytest.raises(vpc_amd.VpcError):
        model.forward(x.cpu(), m.cpu(), m.cpu())
    with pytest.raises(vpc_amd.VpcError):
        em.EDDIMnistTrainer(model).step(x.cpu(), m.cpu())
    with pytest.raises(vpc_amd.VpcError, match="world_size"):
        em.EDDIMnistTrainer(model, world_size=2, rank=0)
    with pytest.raises(TypeError):
        em.EDDIMnistTrainer(vpc_amd.Reg_EDDI(14, 500, 10, 10, TP, "exp", "kl_reg").cuda())
    for bad in ((1025, 20, 10), (784, 33, 10), (784, 20, 16)):
        with pytest.raises(vpc_amd.VpcError):
            em.Reg_EDDI_mnist(bad[0], 500, bad[1], bad[2], TP, "exp", "kl_reg")
    AC = torch.empty(2, 33, 8, device="cuda")
    with pytest.raises(vpc_amd.VpcError):
        em.eddiw_front_fwd(x, m.view(torch.uint8), AC, torch.empty(4, 33, device="cuda"), 4, 1025, 20)
