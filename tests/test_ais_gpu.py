"""GPU: the persistent AIS kernel (csrc/vpc_ais.hip through vpc_amd.ais) against the goldens recorded from the reference's
own ais_trajectory, against the float64 CPU restatement (tests/ais_oracle.py) on the shapes of tests/ais_cases.py, and the
kernel's own draws.

Bounds (the project's parity bounds): per-chain logw within 2e-5 of max |logw|, z within 2e-4 of max |z|; epsilon and
accept_hist equal to the oracle's wherever every decision of the chain agrees.  Accept decisions must equal the float64
oracle's for every (step, chain) whose oracle |prob - u| is at least the case's margin (ais_cases.CASES: four times the
measured fp32-vs-fp64 difference of the CPU restatement), with at most 1 % of the decisions excluded; the seeds are
chosen so that the float64 oracle excludes none.
"""
import os

import numpy as np
import pytest
import torch

import ais_cases as AC
import ais_oracle as AO
from conftest import load_golden
from ais_cases import GOLDENS, golden_chain_inputs, golden_chain_logw

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 1}


@pytest.fixture(scope="module")
def vpc():
    import vpc_amd
    return vpc_amd


def _model(vpc, params, d, L, cls="Reg_VAE"):
    torch.manual_seed(0)
    args = (d, 500, 10, L, TP, "exp") + (("kl_reg",) if cls.startswith("Reg") else ())
    m = getattr(vpc, cls)(*args)
    sd = m.state_dict()
    sd.update({k: v.clone() for k, v in params.items()})
    m.load_state_dict(sd)
    return m.cuda()


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


# ---------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("name", GOLDENS)
def test_chains_vs_reference_golden(vpc, name):
    g = load_golden(name)
    i = golden_chain_inputs(g)
    d, L = g["x"].shape[1], int(g["L"])
    model = _model(vpc, i["params"], d, L, "Reg_VAE" if "reg_vae" in str(g["vae_type"]) else "vanilla_VAE")
    draws = (i["z0"].cuda() if i["mode"] == "forward" else None, i["v"].cuda(), i["u"].cuda())
    logw, z, eps, hist = vpc.ais_chains(model, i["x"].cuda(), g["schedule"], i["n_sample"], mode=i["mode"],
                                        post_z=torch.from_numpy(g["post_z"]).cuda() if i["mode"] == "backward" else None,
                                        likelihood="corrected" if i["sign"] < 0 else "reference", draws=draws)
    e_logw = _rel(logw, golden_chain_logw(g))
    e_z = _rel(z, torch.from_numpy(g["saved_latents"]).reshape(-1, L))
    print(f"{name}: logw err {e_logw:.2e}, z err {e_z:.2e}")
    assert e_logw <= 2e-5 and e_z <= 2e-4
    np.testing.assert_allclose(eps.cpu().numpy(), g["epsilon"], rtol=1e-6)
    np.testing.assert_array_equal(hist.cpu().numpy(), g["accept_hist"])


def test_ais_trajectory_files_and_means(vpc, tmp_path, monkeypatch):
    g = load_golden("ais_reg_d14.npz")
    i = golden_chain_inputs(g)
    d, L = g["x"].shape[1], int(g["L"])
    model = _model(vpc, i["params"], d, L)
    monkeypatch.chdir(tmp_path)
    draws = [(i["z0"].cuda(), i["v"].cuda(), i["u"].cuda())]
    means = vpc.ais_trajectory([(i["x"], torch.from_numpy(g["post_z"]))], d, 500, 10, L, int(g["missing_rate"]),
                               str(g["data_type"]), TP, int(g["max_epochs"]), str(g["vae_type"]), str(g["stage"]), 1, 1,
                               schedule=g["schedule"], n_sample=i["n_sample"], model=model, draws=draws)
    assert len(means) == 1 and abs(means[0].item() - g["means"][0]) <= 2e-5 * abs(g["means"][0])
    assert os.path.isfile(str(g["file_ais"])) and os.path.isfile(str(g["file_latents"]))
    ais = torch.load(str(g["file_ais"]))
    lat = torch.load(str(g["file_latents"]))
    assert ais.shape == torch.Size(g["saved_ais"].shape) and abs(ais.item() - float(g["saved_ais"])) <= 2e-5 * abs(float(g["saved_ais"]))
    assert lat.shape == torch.Size(g["saved_latents"].shape)
    assert _rel(lat, torch.from_numpy(g["saved_latents"])) <= 2e-4


# ---------------------------------------------------------------------------------------------- float64 oracle
def _check_case(vpc, name, sign, grad_clip=1e4):
    i = AC.inputs(name)
    o = AC.oracle(name, sign, torch.float64, grad_clip)
    model = _model(vpc, i["params"], i["d"], i["L"])
    B, T = i["z0"].shape[0], AC.T
    draws = (i["z0"].cuda(), i["v"].cuda(), i["u"].cuda())
    kw = dict(likelihood="corrected" if sign < 0 else "reference", draws=draws, init_step_size=i["step"],
              grad_clip=grad_clip)
    logw, z, eps, hist = vpc.ais_chains(model, i["x"].cuda(), i["schedule"], i["n_sample"], **kw)
    # the kernel's decisions: accept_hist after each prefix of the schedule (same draws, the state is bit-equal however the
    # schedule is split), differenced
    prefix = [vpc.ais_chains(model, i["x"].cuda(), i["schedule"][:k + 1], i["n_sample"],
                             **dict(kw, draws=(draws[0], draws[1][:k], draws[2][:k])))[3].cpu() for k in range(1, T - 1)]
    prefix.append(hist.cpu())
    acc = torch.stack([prefix[0]] + [prefix[k] - prefix[k - 1] for k in range(1, T - 1)]) > 0.5
    margin = i["margin"]
    assert o["margin"].min().item() >= margin, "the seed of this case must leave the float64 oracle no excluded decision"
    decisive = o["margin"] >= margin
    excluded = 1.0 - decisive.double().mean().item()
    same = acc == o["accept"]
    print(f"case {name} sign {sign:+.0f}: decisions {same.numel()}, accept rate {o['accept'].double().mean():.3f}, "
          f"excluded {excluded:.4f}, disagreeing {int((~same).sum())}, min oracle margin {o['margin'].min():.2e}")
    assert excluded <= 0.01
    assert bool(same[decisive].all())
    agree = same.all(0)
    e_logw, e_z = _rel(logw.cpu()[agree], o["logw"][agree]), _rel(z.cpu()[agree], o["z"][agree])
    print(f"   logw err {e_logw:.2e}, z err {e_z:.2e}")
    assert e_logw <= 2e-5 and e_z <= 2e-4
    np.testing.assert_allclose(eps.cpu().numpy()[agree], o["epsilon"].numpy()[agree], rtol=1e-6)
    np.testing.assert_array_equal(hist.cpu().numpy()[agree], o["accept_hist"].numpy()[agree])
    return o


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("name", list(AC.CASES))
def test_chains_vs_float64_oracle(vpc, name, sign):
    o = _check_case(vpc, name, sign)
    rate = o["accept"].double().mean().item()
    assert 0.0 < rate < 1.0  # both branches of accept / reject ran


def test_grad_clip_is_taken(vpc):
    o = _check_case(vpc, "a_clip", 1.0, grad_clip=1.0)
    assert o["clamped"] >= 1


# ---------------------------------------------------------------------------------------------- device draws
def _seeded(vpc, name="a", seed=1234, **kw):
    i = AC.inputs(name)
    model = _model(vpc, i["params"], i["d"], i["L"])
    return model, i, vpc.ais_chains(model, i["x"].cuda(), i["schedule"], i["n_sample"], seed=seed,
                                    init_step_size=i["step"], **kw)


def test_draws_entry_point_matches_seeded_run(vpc):
    model, i, got = _seeded(vpc)
    B = i["z0"].shape[0]
    draws = vpc.ais.ais_draws(B, i["L"], AC.T, 1234)
    inj = vpc.ais_chains(model, i["x"].cuda(), i["schedule"], i["n_sample"], draws=draws, init_step_size=i["step"])
    for a, b in zip(got, inj):
        assert torch.equal(a, b)


def test_seed_reproducible_and_distinct(vpc):
    _, _, r1 = _seeded(vpc, seed=77)
    _, _, r2 = _seeded(vpc, seed=77)
    _, _, r3 = _seeded(vpc, seed=78)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    assert not torch.equal(r1[0], r3[0]) and not torch.equal(r1[1], r3[1])


@pytest.mark.parametrize("name", ["a", "c"])
def test_launch_split_is_bit_equal(vpc, name):
    _, _, whole = _seeded(vpc, name, temps_per_launch=AC.T - 1)
    for tpl in (1, 2):
        _, _, part = _seeded(vpc, name, temps_per_launch=tpl)
        for a, b in zip(whole, part):
            assert torch.equal(a, b)


def test_draw_statistics(vpc):
    B, L, T = 2000, 10, 11  # 2e5 v normals, 2e4 z0 normals; uniforms: a second call with 2e5 values
    z0, v, _ = vpc.ais.ais_draws(B, L, T, 5)
    _, _, u = vpc.ais.ais_draws(20000, 1, T, 6)
    n = v.numel()
    assert n == 200000 and u.numel() == 200000
    vd, ud = v.double().flatten(), u.double().flatten()
    assert abs(vd.mean().item()) <= 5 / np.sqrt(n)
    assert abs(vd.var().item() - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert abs(ud.mean().item() - 0.5) <= 5 * np.sqrt(1 / 12 / n)
    assert abs(ud.var().item() - 1 / 12) <= 5 * np.sqrt(1 / 180 / n)  # var of (U - 1/2)^2 is 1/180
    assert abs(z0.double().mean().item()) <= 5 / np.sqrt(z0.numel())
    assert 0.0 < ud.min().item() and ud.max().item() < 1.0


# ---------------------------------------------------------------------------------------------- entry points
def test_unsupported_raise(vpc):
    i = AC.inputs("a")
    x = i["x"].cuda()
    sched = i["schedule"]
    model = _model(vpc, i["params"], i["d"], i["L"])
    with pytest.raises(vpc.VpcError):  # CPU tensors
        vpc.ais_chains(model, i["x"], sched, 2)
    with pytest.raises(vpc.VpcError):  # another family: its decoder is no Gaussian (mean, logvar) chain of this shape
        vpc.ais_chains(vpc.MIWAE(14, 500, 10, 10, TP, 5, 1).cuda(), x, sched, 2)
    with pytest.raises(vpc.VpcError):  # wide model (generic GEMM path): obs_dim > 128
        vpc.ais_chains(vpc.Reg_VAE(200, 500, 10, 10, TP, "exp", "kl_reg").cuda(), torch.rand(4, 200).cuda(), sched, 2)
    with pytest.raises(vpc.VpcError):  # latent_dim > 15
        vpc.ais_chains(vpc.vanilla_VAE(14, 500, 10, 20, TP, "exp").cuda(), x, sched, 2)
    lib = vpc._lib.lib()
    assert lib.vpc_ais_applicable(100, 128, 15) == 1
    assert lib.vpc_ais_applicable(100, 129, 10) == 0 and lib.vpc_ais_applicable(100, 14, 16) == 0
    st = torch.empty(int(lib.vpc_ais_state_floats(16)), device="cuda")
    img = torch.zeros(4096 * 8, device="cuda")
    s = torch.zeros(4, device="cuda")
    P = vpc._lib.ptr
    assert lib.vpc_ais_run(P(x), P(img), P(s), 4, 1, 3, 1, P(st), None, None, None, 0, 1.0, 10, 0.01, 1e4, -3.9, 16, 4,
                           129, 10, None) == 2
    assert lib.vpc_ais_run(P(x), P(img), P(s), 4, 1, 3, 1, P(st), None, None, None, 0, 1.0, 10, 0.01, 1e4, -3.9, 16, 4,
                           14, 16, None) == 2


def test_eddi_decoder_is_supported(vpc):
    """Reg_EDDI's seq_decoder is the same latent -> 50 -> 100 -> d sigmoid chain (VAE.py:701-709)."""
    i = AC.inputs("a")
    torch.manual_seed(0)
    m = vpc.Reg_EDDI(i["d"], 500, 10, i["L"], TP, "exp", "kl_reg")
    sd = m.state_dict()
    sd.update({k: v.clone() for k, v in i["params"].items()})
    m.load_state_dict(sd)
    m.cuda()
    ref, _, got = _seeded(vpc, "a", seed=9)
    out = vpc.ais_chains(m, i["x"].cuda(), i["schedule"], i["n_sample"], seed=9, init_step_size=i["step"])
    for a, b in zip(got, out):
        assert torch.equal(a, b)


def test_mask_variant_and_its_limit(vpc):
    """Reg_VAE_mask has the same decoder chain: same parameters, same seed -> the same chains as Reg_VAE.  Past obs_dim = 64
    its encoder input (2 d) leaves the register-chained kernels and with it the packed decoder image: VpcError."""
    i = AC.inputs("a")
    _, _, got = _seeded(vpc, "a", seed=9)
    m = _model(vpc, i["params"], i["d"], i["L"], "Reg_VAE_mask")
    out = vpc.ais_chains(m, i["x"].cuda(), i["schedule"], i["n_sample"], seed=9, init_step_size=i["step"])
    for a, b in zip(got, out):
        assert torch.equal(a, b)
    with pytest.raises(vpc.VpcError):
        vpc.ais_chains(vpc.Reg_VAE_mask(72, 500, 10, 3, TP, "exp", "kl_reg").cuda(), torch.rand(4, 72).cuda(),
                       i["schedule"], 2)


def test_eval_ais_writes_every_stage(vpc, tmp_path, monkeypatch):
    g = load_golden("ais_reg_d14.npz")
    i = golden_chain_inputs(g)
    d, L = g["x"].shape[1], int(g["L"])
    model = _model(vpc, i["params"], d, L)
    monkeypatch.chdir(tmp_path)
    loaders = [([(i["x"], torch.from_numpy(g["post_z"]))], st) for st in ("train", "valid", "test")]
    vpc.eval_ais(*loaders, d, 500, 10, L, 40, "toy", TP, 7, "reg_vae1", 1, 1, schedule=g["schedule"],
                 n_sample=i["n_sample"], model=model, seed=3)
    vals = []
    for st in ("train", "valid", "test"):
        f_ais = f"experiments/reg_vae1/toy/elbos/40_missing/7_epochs/{st}_ais.pt"
        f_lat = f"experiments/reg_vae1/toy/latents/40_missing/7_epochs/{st}_ais_true_latents.pt"
        vals.append(torch.load(f_ais).item())
        assert torch.load(f_lat).shape == (g["x"].shape[0], i["n_sample"], L)
    assert vals[0] == vals[1] == vals[2] and np.isfinite(vals[0])  # same data, same seed
