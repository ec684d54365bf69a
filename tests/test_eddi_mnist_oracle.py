"""CPU checks of the MNIST point-net pair (Reg_EDDI_mnist / vanilla_EDDI_mnist): the oracle port and the float64 closed form
against vectors captured from the reference itself (tests/golden/eddi_mnist_*.npz), bitwise initialisation under the recorded
seed, state_dict layout, model_loader dispatch and the stated limits.  Runs anywhere (no GPU)."""
import zlib

import numpy as np
import pytest
import torch

from conftest import load_golden

import eddi_mnist_oracle as MO

TP = {"batch_size": 64, "patience": 1}
GOLD = ["eddi_mnist_reg_d784.npz", "eddi_mnist_van_d784.npz", "eddi_mnist_reg_d200.npz"]
TAGS = (("kl0.5", "kl_reg", 0.5), ("kl1.0", "kl_reg", 1.0), ("ml0.8", "ml_reg", 0.8))


def _model(g, seed_key="seed"):
    """The package's class built under the golden's seed (the goldens store no weights)."""
    import vpc_amd
    d = g["x"].shape[1]
    torch.manual_seed(int(g[seed_key]))
    if "mask_p" in g or "fwd.mean_p" in g:
        return vpc_amd.Reg_EDDI_mnist(d, 500, int(g["K"]), int(g["L"]), TP, "exp", "kl_reg")
    return vpc_amd.vanilla_EDDI_mnist(d, 500, int(g["K"]), int(g["L"]), TP, "exp")


def _params(g):
    return {k: v.detach().clone() for k, v in _model(g).state_dict().items()}


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


@pytest.mark.parametrize("name", GOLD + ["eddi_mnist_traj_reg_d784.npz", "eddi_mnist_traj_van_d784.npz"])
def test_constructor_reproduces_reference_init_bitwise(name):
    g = load_golden(name)
    model = _model(g)
    sd = model.state_dict()
    assert tuple(sd.keys()) == MO.STATE_KEYS
    if "keys" in g:
        assert [str(k) for k in g["keys"]] == list(sd.keys())
    crc = 0
    for k, v in sd.items():
        crc = zlib.crc32(np.ascontiguousarray(v.numpy()).tobytes(), crc)
    assert crc == int(g["param_crc"])  # CRC-32 over every tensor's bytes in state_dict order: bitwise the reference's
    prefix = "param." if "param.type_pars1" in g else "param0."
    for k, v in sd.items():
        assert np.array_equal(MO.stored(k, v.numpy()), g[prefix + k]), k
    assert model.max_epoch == 2800 and model.emb_dim == int(g["K"]) and model.latent_dim == int(g["L"])
    assert model.x_logvar.shape == (1,) and abs(float(model.x_logvar) - MO.X_LOGVAR) < 1e-6


def test_reference_state_dict_loads_strict():
    """The reference's state_dict (bitwise ours under the seed, see above) in the reference's key order loads with strict=True,
    and a freshly built model takes its values."""
    import vpc_amd
    g = load_golden(GOLD[0])
    ref = {str(k): v for k, v in zip(g["keys"], [_params(g)[str(k)] for k in g["keys"]])}
    torch.manual_seed(1)
    model = vpc_amd.Reg_EDDI_mnist(784, 500, 20, 10, TP, "exp", "kl_reg")
    res = model.load_state_dict(ref, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref[k]), k
    van = vpc_amd.vanilla_EDDI_mnist(784, 500, 20, 10, TP, "exp")
    van.load_state_dict(ref, strict=True)  # both classes share the layout (VAE.py:27-56, 220-250)


def test_model_loader_dispatch():
    import vpc_amd
    args = ("train", 784, 500, 20, 10, 30, "mnist", TP, 10, 1, 1, "exp", "kl_reg")
    m = vpc_amd.model_loader(*args, "reg_EDDI1")
    assert type(m) is vpc_amd.Reg_EDDI_mnist and tuple(m.state_dict().keys()) == MO.STATE_KEYS and m.reg_type == "kl_reg"
    m = vpc_amd.model_loader(*args, "vanilla_EDDI1")
    assert type(m) is vpc_amd.vanilla_EDDI_mnist and tuple(m.state_dict().keys()) == MO.STATE_KEYS
    m = vpc_amd.model_loader(*args, "vanilla_EDDI_with_drop1")
    assert type(m) is vpc_amd.vanilla_EDDI_mnist
    wine = ("train", 12, 500, 10, 10, 30, "wine", TP, 10, 1, 1, "exp", "kl_reg")
    assert type(vpc_amd.model_loader(*wine, "reg_EDDI1")) is vpc_amd.Reg_EDDI
    assert type(vpc_amd.model_loader(*wine, "vanilla_EDDI1")) is vpc_amd.vanilla_EDDI
    with pytest.raises(NotImplementedError):
        vpc_amd.model_loader(*args, "reg_flow1")


def test_limits_and_cpu_tensors_raise():
    import vpc_amd
    for bad in ((1025, 20, 10), (784, 33, 10), (784, 20, 16)):
        with pytest.raises(vpc_amd.VpcError):
            vpc_amd.Reg_EDDI_mnist(bad[0], 500, bad[1], bad[2], TP, "exp", "kl_reg")
        with pytest.raises(vpc_amd.VpcError):
            vpc_amd.vanilla_EDDI_mnist(bad[0], 500, bad[1], bad[2], TP, "exp")
    m = vpc_amd.vanilla_EDDI_mnist(64, 500, 4, 3, TP, "exp")
    x, mask = torch.rand(2, 64), torch.ones(2, 64, dtype=torch.bool)
    with pytest.raises(vpc_amd.VpcError):
        m.forward(x, mask)
    with pytest.raises(vpc_amd.VpcError):
        m.decoder(torch.zeros(2, 3))
    with pytest.raises(vpc_amd.VpcError):
        vpc_amd.reward_matrix(m, x, mask, torch.rand(3, 2, 64))


@pytest.mark.parametrize("name", ["eddi_mnist_reg_d784.npz", "eddi_mnist_reg_d200.npz"])
def test_port_reg_against_reference(name):
    g = load_golden(name)
    p, Ld = _params(g), int(g["L"])
    x, m, mp = (torch.from_numpy(g[k]) for k in ("x", "mask", "mask_p"))
    eps = torch.from_numpy(np.stack([g["eps_q"], g["eps_p"]]))
    port = MO.EDDIMnistPort(p, Ld, "kl_reg")
    with torch.no_grad():
        o = port.reg_forward(x, m, mp, eps[0], eps[1])
        names = ["mean_p", "logvar_p", "x_mean_p", "x_logvar_p", "mean_q", "logvar_q", "x_mean_q", "x_logvar_q"]
        for n, t in zip(names, o):
            ref = g["fwd." + n]
            assert np.max(np.abs(t.numpy().reshape(ref.shape) - ref)) <= 1e-6 * max(1.0, np.abs(ref).max()), n
        r = port.reg_loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], m, mp, 7, llh_eval=True, stage="evaluate")
        for got, key in zip(r[1:], ("eval_loss", "eval_re", "eval_re_imp")):
            assert _rel(got, g[key]) <= 1e-6, key
    for tag, rt, alpha in TAGS:
        kw = dict(reg_type=rt, alpha=alpha, beta=0.9, beta_annealing=(tag == "kl1.0"), epoch=1400,
                  eps_ml=torch.from_numpy(g["eps_ml"]))
        tl, gr = MO.port_step(p, Ld, x, m, mp, eps, **kw)
        assert _rel(tl, g[f"loss.{tag}"]) <= 1e-6, tag
        for k in MO.KEYS:
            ref = g.get(f"grad.{tag}.{k}")
            if ref is None:  # ml_reg gives the p decoder no gradient path of its own but every tensor still has one
                continue
            err = np.max(np.abs(MO.stored(k, gr[k].numpy()) - ref))
            assert err <= 1e-5 * float(g[f"gmax.{tag}.{k}"]) + 1e-12, (tag, k, err)
        # float64: closed form against autograd of the port (gradient 1e-9 of max), and against the reference's fp32 loss
        tl64, gr64 = MO.port_step(p, Ld, x, m, mp, eps, dtype=torch.float64, **kw)
        cl, cg = MO.closed_form_step(p, Ld, g["x"], g["mask"], g["mask_p"], eps.numpy(), **{**kw, "eps_ml": g["eps_ml"]})
        assert _rel(cl, tl64) <= 1e-12 and _rel(cl, g[f"loss.{tag}"]) <= 1e-6, tag
        for k in MO.KEYS:
            a, b = cg[k].reshape(-1), gr64[k].numpy().reshape(-1)
            assert np.max(np.abs(a - b)) <= 1e-9 * max(np.abs(b).max(), 1e-30), (tag, k)


def test_port_vanilla_against_reference():
    g = load_golden("eddi_mnist_van_d784.npz")
    p, Ld = _params(g), int(g["L"])
    x, m = torch.from_numpy(g["x"]), torch.from_numpy(g["mask"])
    mf = m * torch.ones(m.shape)
    eps = torch.from_numpy(g["eps_q"])[None]
    port = MO.EDDIMnistPort(p, Ld)
    with torch.no_grad():
        o = port.vanilla_forward(x, mf, eps[0])
        for n, t in zip(["mean", "logvar", "x_mean", "x_logvar"], o):
            ref = g["fwd." + n]
            assert np.max(np.abs(t.numpy().reshape(ref.shape) - ref)) <= 1e-6 * max(1.0, np.abs(ref).max()), n
        r = port.vanilla_loss(x, o[2], o[3], o[0], o[1], 3, mf, beta=0.8, llh_eval=True)  # 'train' stage: RE_imputed all the same
        for got, key in zip(r[1:], ("loss", "re", "re_imp")):
            assert _rel(got, g[key]) <= 1e-6, key
    tl, gr = MO.port_step(p, Ld, x, mf, None, eps, beta=0.8, epoch=3)
    assert _rel(tl, g["loss"]) <= 1e-6
    for k in MO.KEYS:
        err = np.max(np.abs(MO.stored(k, gr[k].numpy()) - g[f"grad.v.{k}"]))
        assert err <= 1e-5 * float(g[f"gmax.v.{k}"]) + 1e-12, (k, err)
    tl64, gr64 = MO.port_step(p, Ld, x, mf, None, eps, beta=0.8, epoch=3, dtype=torch.float64)
    cl, cg = MO.closed_form_step(p, Ld, g["x"], g["mask"], None, eps.numpy(), beta=0.8, epoch=3)
    assert _rel(cl, tl64) <= 1e-12 and _rel(cl, g["loss"]) <= 1e-6
    for k in MO.KEYS:
        a, b = cg[k].reshape(-1), gr64[k].numpy().reshape(-1)
        assert np.max(np.abs(a - b)) <= 1e-9 * max(np.abs(b).max(), 1e-30), k


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_port_trajectory_against_reference(kind):
    g = load_golden(f"eddi_mnist_traj_{kind}_d784.npz")
    model = _model(g)
    tr = MO.TorchTrainer({k: v for k, v in model.state_dict().items()}, int(g["L"]), vanilla=(kind == "van"))
    x, m = torch.from_numpy(g["x"]), torch.from_numpy(g["mask"])
    for s in range(len(g["losses"])):
        eps = torch.from_numpy(g["eps"][s])
        if kind == "reg":
            loss = tr.step(x, m, torch.from_numpy(g["mask_p"][s]), eps, epoch=s + 1, alpha=0.5)
        else:
            loss = tr.step(x, m * torch.ones(m.shape), None, eps, epoch=s + 1)
        assert _rel(loss, g["losses"][s]) <= 1e-6, (s, loss)
    for k in MO.KEYS:
        ref = g["param5." + k]
        got = MO.stored(k, tr.p[k].detach().numpy())
        assert np.max(np.abs(got - ref)) <= 1e-5 * max(1.0, np.abs(ref).max()), k
