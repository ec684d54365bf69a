"""GPU: the GEMM-backed AIS engine (csrc/vpc_aisg.hip through vpc_amd.ais, engine="gemm") against the goldens recorded from
the reference's own ais_trajectory on its MNAR, flow, wide and latent-20 models, against the float64 CPU restatement
(tests/ais_family_oracle.py) on the shapes of tests/ais_family_cases.py, with a mask, and the engine's own properties.

Bounds (the project's parity bounds, as tests/test_ais_gpu.py): per-chain logw within 2e-5 of max |logw|, z within 2e-4 of
max |z|; epsilon at rtol 1e-6 and accept_hist equal wherever every decision of the chain agrees.  Accept decisions must
equal the float64 oracle's for every (step, chain) whose oracle |prob - u| is at least the case's margin (four times the
measured fp32-vs-fp64 difference of the CPU restatement, recorded next to the case), with at most 1 % of the decisions
excluded; the seeds are chosen so that the float64 oracle excludes none.  mnar14_ref (MNAR under the reference's sign)
carries its own logw / z bounds: 4 x what the fp32 CPU restatement measures against float64 on it (ais_family_cases).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ais_cases as AC
import ais_family_cases as FC
import ais_family_oracle as FO
import ais_oracle as AO
from conftest import load_golden

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 1}


@pytest.fixture(scope="module")
def vpc():
    import vpc_amd
    return vpc_amd


def _model(vpc, family, params, d, L, kind=""):
    torch.manual_seed(0)
    if family == "mnar":
        m = (vpc.notMIWAE_myversion if kind == "nm_van" else vpc.REG_notMIWAE_v2)(d, 500, 10, L, TP, 1, 1)
    elif family == "flow":
        m = vpc.VAEFlow(d, params["seq_decoder.0.weight"].shape[0], 10, L, TP)
    elif family == "mnist":
        m = vpc.vanilla_EDDI_mnist(d, 500, 10, L, TP, "exp")
    elif kind == "van":
        m = vpc.vanilla_VAE(d, 500, 10, L, TP, "exp")
    else:
        m = vpc.Reg_VAE(d, 500, 10, L, TP, "exp", "kl_reg")
    sd = m.state_dict()
    for k, v in params.items():
        assert k in sd and sd[k].shape == v.shape, k
    sd.update({k: v.clone() for k, v in params.items()})
    m.load_state_dict(sd)
    return m.cuda()


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _cuda(t):
    return None if t is None else t.cuda()


# ---------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("name", FC.GOLDENS)
def test_chains_vs_reference_golden(vpc, name):
    g = load_golden(name)
    i = FC.golden_chain_inputs(g)
    d, L = g["x"].shape[1], int(g["L"])
    model = _model(vpc, i["family"], i["params"], d, L, str(g["kind"]))
    draws = (i["z0"].cuda() if i["mode"] == "forward" else None, i["v"].cuda(), i["u"].cuda())
    logw, z, eps, hist = vpc.ais_chains(model, i["x"].cuda(), g["schedule"], i["n_sample"], mode=i["mode"],
                                        post_z=torch.from_numpy(g["post_z"]).cuda() if i["mode"] == "backward" else None,
                                        likelihood="corrected" if i["sign"] < 0 else "reference", draws=draws,
                                        engine="gemm")
    e_logw = _rel(logw, FC.golden_chain_logw(g))
    e_z = _rel(z, torch.from_numpy(g["saved_latents"]).reshape(-1, L))
    print(f"{name}: logw err {e_logw:.2e}, z err {e_z:.2e}")
    assert e_logw <= 2e-5 and e_z <= 2e-4
    np.testing.assert_allclose(eps.cpu().numpy(), g["epsilon"], rtol=1e-6)
    np.testing.assert_array_equal(hist.cpu().numpy(), g["accept_hist"])


# ---------------------------------------------------------------------------------------------- float64 oracle
def _check(vpc, label, model, i, o, sign, margin, bounds=(2e-5, 2e-4), grad_clip=1e4, mask=None):
    """i: x, schedule, n_sample, z0, v, u, step; o: the float64 oracle's run of the same chain."""
    T = len(i["schedule"])
    draws = (i["z0"].cuda(), i["v"].cuda(), i["u"].cuda())
    kw = dict(likelihood="corrected" if sign < 0 else "reference", draws=draws, init_step_size=i["step"],
              grad_clip=grad_clip, engine="gemm", mask=_cuda(mask))
    x = i["x"].cuda()
    logw, z, eps, hist = vpc.ais_chains(model, x, i["schedule"], i["n_sample"], **kw)
    # the engine's decisions: accept_hist after each prefix of the schedule (same draws, the state is bit-equal however the
    # schedule is split), differenced
    prefix = [vpc.ais_chains(model, x, i["schedule"][:k + 1], i["n_sample"],
                             **dict(kw, draws=(draws[0], draws[1][:k], draws[2][:k])))[3].cpu() for k in range(1, T - 1)]
    prefix.append(hist.cpu())
    acc = torch.stack([prefix[0]] + [prefix[k] - prefix[k - 1] for k in range(1, T - 1)]) > 0.5
    assert o["margin"].min().item() >= margin, "the seed of this case must leave the float64 oracle no excluded decision"
    decisive = o["margin"] >= margin
    excluded = 1.0 - decisive.double().mean().item()
    same = acc == o["accept"]
    print(f"case {label} sign {sign:+.0f}: decisions {same.numel()}, accept rate {o['accept'].double().mean():.3f}, "
          f"excluded {excluded:.4f}, disagreeing {int((~same).sum())}, min oracle margin {o['margin'].min():.2e}")
    agree = same.all(0)
    e_logw, e_z = _rel(logw.cpu()[agree], o["logw"][agree]), _rel(z.cpu()[agree], o["z"][agree])
    print(f"   logw err {e_logw:.2e} (bound {bounds[0]:.2e}), z err {e_z:.2e} (bound {bounds[1]:.2e})")
    assert excluded <= 0.01
    assert bool(same[decisive].all())
    assert e_logw <= bounds[0] and e_z <= bounds[1]
    np.testing.assert_allclose(eps.cpu().numpy()[agree], o["epsilon"].numpy()[agree], rtol=1e-6)
    np.testing.assert_array_equal(hist.cpu().numpy()[agree], o["accept_hist"].numpy()[agree])


def _check_case(vpc, name):
    i = FC.inputs(name)
    o = FC.oracle(name)
    model = _model(vpc, i["family"], i["params"], i["d"], i["L"])
    _check(vpc, name, model, i, o, i["sign"], i["margin"], i.get("bounds", (2e-5, 2e-4)), i["grad_clip"], i["mask"])
    return o


PLAIN = [n for n, c in FC.CASES.items() if "mask" not in c and "grad_clip" not in c]


@pytest.mark.parametrize("name", PLAIN)
def test_chains_vs_float64_oracle(vpc, name):
    o = _check_case(vpc, name)
    rate = o["accept"].double().mean().item()
    assert 0.0 < rate < 1.0  # both branches of accept / reject ran


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("name", ["a", "d"])
def test_persistent_kernel_cases_through_gemm(vpc, name, sign):
    """Cases a and d of tests/ais_cases.py (inside the persistent kernel's limits): the same check through engine="gemm"."""
    i = AC.inputs(name)
    o = AC.oracle(name, sign, torch.float64, 1e4)
    model = _model(vpc, "dense", i["params"], i["d"], i["L"])
    _check(vpc, name, model, i, o, sign, i["margin"])


def test_grad_clip_is_taken(vpc):
    o = _check_case(vpc, "mnar14_clip")
    assert o["clamped"] >= 1


# ---------------------------------------------------------------------------------------------- mask
@pytest.mark.parametrize("name", ["mnar14_mask", "dense129_mask"])
def test_masked_chains_vs_float64_oracle(vpc, name):
    i = FC.inputs(name)
    assert 0.5 < i["mask"].mean().item() < 0.9 and not bool((i["mask"].sum(1) == 0).any())
    _check_case(vpc, name)


def _seeded(vpc, name, seed=1234, **kw):
    i = FC.inputs(name)
    model = _model(vpc, i["family"], i["params"], i["d"], i["L"])
    kw.setdefault("engine", "gemm")
    return model, i, vpc.ais_chains(model, i["x"].cuda(), i["schedule"], i["n_sample"], seed=seed,
                                    init_step_size=i["step"], likelihood="corrected", **kw)


@pytest.mark.parametrize("name", ["mnar14", "mnist200"])
def test_all_ones_mask_is_bit_equal_to_no_mask(vpc, name):
    _, i, plain = _seeded(vpc, name)
    _, _, ones = _seeded(vpc, name, mask=torch.ones_like(i["x"]).cuda())
    for a, b in zip(plain, ones):
        assert torch.equal(a, b)


def test_mask_with_the_persistent_engine_raises(vpc):
    i = AC.inputs("a")
    model = _model(vpc, "dense", i["params"], i["d"], i["L"])
    with pytest.raises(vpc.VpcError):
        vpc.ais_chains(model, i["x"].cuda(), i["schedule"], 2, mask=torch.ones_like(i["x"]).cuda())
    with pytest.raises(vpc.VpcError):
        vpc.ais_chains(model, i["x"].cuda(), i["schedule"], 2, engine="persistent", mask=torch.ones_like(i["x"]).cuda())


# ---------------------------------------------------------------------------------------------- engine properties
@pytest.mark.parametrize("name", ["mnar14", "dense129"])  # dense129: latent_dim 20, the counter groups past the fourth
def test_draws_entry_point_matches_seeded_run(vpc, name):
    model, i, got = _seeded(vpc, name)
    B = i["z0"].shape[0]
    draws = vpc.ais.ais_draws(B, i["L"], FC.T, 1234)
    inj = vpc.ais_chains(model, i["x"].cuda(), i["schedule"], i["n_sample"], draws=draws, init_step_size=i["step"],
                         likelihood="corrected", engine="gemm")
    for a, b in zip(got, inj):
        assert torch.equal(a, b)
    if i["L"] > 16:  # the groups past the fourth are draws of their own
        v = draws[1]
        assert not torch.equal(v[:, :, 0:4], v[:, :, 16:20])
        assert abs(v.double().mean().item()) <= 5 / np.sqrt(v.numel())
        assert abs(v.double().var().item() - 1.0) <= 5 * np.sqrt(2.0 / v.numel())


@pytest.mark.parametrize("name", ["mnar14", "dense129", "flow12"])
def test_launch_split_is_bit_equal(vpc, name):
    _, _, whole = _seeded(vpc, name, temps_per_launch=FC.T - 1)
    for tpl in (1, 2):
        _, _, part = _seeded(vpc, name, temps_per_launch=tpl)
        for a, b in zip(whole, part):
            assert torch.equal(a, b)


def test_seed_reproducible_and_distinct(vpc):
    _, _, r1 = _seeded(vpc, "mnar40", seed=77)
    _, _, r2 = _seeded(vpc, "mnar40", seed=77)
    _, _, r3 = _seeded(vpc, "mnar40", seed=78)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    assert not torch.equal(r1[0], r3[0]) and not torch.equal(r1[1], r3[1])


def test_engine_auto(vpc):
    """auto = the persistent kernel where it applies (dense d = 14), the GEMM engine elsewhere (d = 129) and with a mask."""
    i = AC.inputs("a")
    model = _model(vpc, "dense", i["params"], i["d"], i["L"])
    kw = dict(seed=5, init_step_size=i["step"])
    run = lambda m, x, n, **k: vpc.ais_chains(m, x.cuda(), i["schedule"], n, **kw, **k)
    for a, b in zip(run(model, i["x"], i["n_sample"], engine="auto"), run(model, i["x"], i["n_sample"], engine="persistent")):
        assert torch.equal(a, b)
    ones = torch.ones_like(i["x"]).cuda()
    for a, b in zip(run(model, i["x"], i["n_sample"], engine="auto", mask=ones),
                    run(model, i["x"], i["n_sample"], engine="gemm", mask=ones)):
        assert torch.equal(a, b)
    w = FC.inputs("dense129")
    wide = _model(vpc, "dense", w["params"], w["d"], w["L"])
    for a, b in zip(run(wide, w["x"], w["n_sample"], engine="auto"), run(wide, w["x"], w["n_sample"], engine="gemm")):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        run(model, i["x"], 2, engine="fused")


# ---------------------------------------------------------------------------------------------- refusals
def test_miwae_raises_under_every_engine(vpc):
    i = AC.inputs("a")
    m = vpc.MIWAE(14, 500, 10, 10, TP, 5, 1).cuda()
    for engine in ("persistent", "gemm", "auto"):
        with pytest.raises(vpc.VpcError):
            vpc.ais_chains(m, i["x"].cuda(), i["schedule"], 2, engine=engine)


def test_default_engine_still_refuses(vpc):
    """What tests/test_ais_gpu.py::test_unsupported_raise lists, under the default engine; engine="gemm" takes the two wide ones."""
    i = AC.inputs("a")
    x, sched = i["x"].cuda(), i["schedule"]
    wide = vpc.Reg_VAE(200, 500, 10, 10, TP, "exp", "kl_reg").cuda()
    deep = vpc.vanilla_VAE(14, 500, 10, 20, TP, "exp").cuda()
    with pytest.raises(vpc.VpcError):
        vpc.ais_chains(_model(vpc, "dense", i["params"], i["d"], i["L"]), i["x"], sched, 2)  # CPU tensors
    with pytest.raises(vpc.VpcError):
        vpc.ais_chains(vpc.MIWAE(14, 500, 10, 10, TP, 5, 1).cuda(), x, sched, 2)
    with pytest.raises(vpc.VpcError):
        vpc.ais_chains(wide, torch.rand(4, 200).cuda(), sched, 2)
    with pytest.raises(vpc.VpcError):
        vpc.ais_chains(deep, x, sched, 2)
    for m, xx in ((wide, torch.rand(4, 200).cuda()), (deep, x)):
        logw = vpc.ais_chains(m, xx, sched, 2, engine="gemm", seed=1)[0]
        assert logw.shape == (2 * xx.shape[0],) and bool(torch.isfinite(logw).all())
    with pytest.raises(vpc.VpcError):  # CPU tensors under the new engine too
        vpc.ais_chains(wide, torch.rand(4, 200), sched, 2, engine="gemm")


def _raw_run(vpc, d, hid, L=10, B=8, nb=4):
    """vpc_aisg_run on a two-layer chain L -> hid -> d of zeros: the C entry's return code."""
    lib, P = vpc._lib.lib(), vpc._lib.ptr
    dev = "cuda"
    w = [torch.zeros(hid, L, device=dev), torch.zeros(d, hid, device=dev)]
    b = [torch.zeros(hid, device=dev), torch.zeros(d, device=dev)]
    Ks, Ns, acts = (C.c_int * 2)(L, hid), (C.c_int * 2)(hid, d), (C.c_int * 2)(3, 2)
    floats = int(lib.vpc_aisg_workspace_floats(B, L, 2, Ns))
    assert floats > 0
    work = torch.zeros(floats, device=dev)
    x, sched = torch.rand(nb, d, device=dev), torch.linspace(0, 1, 4, device=dev)
    rc = lib.vpc_aisg_run(P(x), None, vpc._lib.ptr_array(w), vpc._lib.ptr_array(b), Ks, Ns, acts, 2, d, -3.9, P(sched), 4, 1,
                          3, 1, P(work), floats, None, None, None, 0, 1.0, 10, 0.01, 1e4, B, nb, d, L, None)
    torch.cuda.synchronize()
    return rc, work


def test_shape_limits_of_the_c_entry(vpc):
    rc, work = _raw_run(vpc, 1024, 512)
    assert rc == 0 and bool(torch.isfinite(work[:8 * 10]).all())
    assert _raw_run(vpc, 1025, 512)[0] == 2
    assert _raw_run(vpc, 1024, 513)[0] == 2
    assert _raw_run(vpc, 64, 64, L=65)[0] == 2


# ---------------------------------------------------------------------------------------------- drivers
def test_eval_ais_gemm_writes_every_stage(vpc, tmp_path, monkeypatch):
    g = load_golden("ais_nm_reg_d14.npz")
    i = FC.golden_chain_inputs(g)
    d, L = g["x"].shape[1], int(g["L"])
    model = _model(vpc, "mnar", i["params"], d, L)
    monkeypatch.chdir(tmp_path)
    loaders = [([(i["x"], torch.from_numpy(g["post_z"]))], st) for st in ("train", "valid", "test")]
    draws = [(i["z0"].cuda(), i["v"].cuda(), i["u"].cuda())]
    vpc.eval_ais(*loaders, d, 500, 10, L, 40, "toy", TP, 7, "reg_notmiwae", 1, 1, schedule=g["schedule"],
                 n_sample=i["n_sample"], model=model, draws=draws, engine="gemm")
    for st in ("train", "valid", "test"):
        f_ais = f"experiments/reg_notmiwae/toy/elbos/40_missing/7_epochs/{st}_ais.pt"
        f_lat = f"experiments/reg_notmiwae/toy/latents/40_missing/7_epochs/{st}_ais_true_latents.pt"
        val = torch.load(f_ais).item()
        assert abs(val - float(g["saved_ais"])) <= 2e-5 * abs(float(g["saved_ais"]))  # the reference's saved mean
        lat = torch.load(f_lat)
        assert lat.shape == (g["x"].shape[0], i["n_sample"], L)
        assert _rel(lat, torch.from_numpy(g["saved_latents"])) <= 2e-4
    # masks= : one per batch; an observed-columns likelihood is another number
    masks = [(torch.rand(g["x"].shape, generator=torch.Generator().manual_seed(0)) < 0.7).float().cuda()]
    m = vpc.ais_trajectory(loaders[0][0], d, 500, 10, L, 40, "toy", TP, 7, "reg_notmiwae", "masked", 1, 1,
                           schedule=g["schedule"], n_sample=i["n_sample"], model=model, draws=draws, engine="gemm",
                           masks=masks)
    assert np.isfinite(m[0].item()) and abs(m[0].item() - float(g["saved_ais"])) > 1e-3
