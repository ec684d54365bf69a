"""CPU checks of the flow-path oracle (tests/flow_oracle.py): it reproduces the fixtures recorded from the reference
(tests/golden/make_golden_flow.py) and its closed-form gradients equal torch autograd of the same restatement, at the
config's hid_dim 500 included.  No GPU, no HIP library."""
import os

import numpy as np
import pytest

import flow_oracle as FO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    z = np.load(os.path.join(GOLD, name))
    return {k: z[k] for k in z.files}


def _params(g, prefix="param."):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def _check_grads(got, g, tag, tol=1e-4):
    pre = f"grad.{tag}."
    names = [k for k in g if k.startswith(pre)]
    assert sorted(n[len(pre):] for n in names) == sorted(FO.TRAINABLE)
    for n in names:
        ref, k = g[n], n[len(pre):]
        err = np.max(np.abs(got[k] - ref)) / (np.max(np.abs(ref)) + 1e-30)
        assert err < tol, (n, err)


@pytest.mark.parametrize("d", [12, 40])
def test_oracle_matches_reference_reg(d):
    g = _load(f"flow_reg_d{d}.npz")
    P = _params(g)
    for alpha in (1.0, 0.5, 0.0):
        r = FO.step(P, g["x"], g["mask"], g["mask_p"], g["eps"], alpha=alpha)
        ref = float(g[f"loss.a{alpha}"])
        assert abs(r["loss"] - ref) <= 1e-5 * abs(ref), (alpha, r["loss"], ref)
        _check_grads(r["grads"], g, f"a{alpha}")
    for k in ("z_q", "z_log_prob_q", "x_mean_q", "z_p", "z_log_prob_p", "x_mean_p"):
        np.testing.assert_allclose(r["fwd"][k], g["fwd." + k], rtol=1e-4, atol=1e-5, err_msg=k)
    for stage in ("train", "evaluate"):
        r = FO.step(P, g["x"], g["mask"], g["mask_p"], g["eps"], alpha=0.5, stage=stage)
        llh = g[f"llh.{stage}"]
        np.testing.assert_allclose([r["loss"], r["loss"]], llh[:2], rtol=1e-5)
        np.testing.assert_allclose(r["llh"][0], llh[2], rtol=1e-5)
        np.testing.assert_allclose(r["llh"][1] if stage == "evaluate" else 0.0, llh[3], rtol=1e-5)
    if "loss.eval" in g:
        r = FO.step(P, g["x"], g["mask"], g["mask_p"], g["eps"], alpha=0.5, stage="evaluate")
        assert abs(r["loss"] - float(g["loss.eval"])) <= 1e-5 * abs(float(g["loss.eval"]))
        _check_grads(r["grads"], g, "eval")


@pytest.mark.parametrize("d", [12, 40])
def test_oracle_matches_reference_vanilla(d):
    g = _load(f"flow_van_d{d}.npz")
    r = FO.step(_params(g), g["x"], g["mask"], None, g["eps"])
    assert abs(r["loss"] - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    assert abs(r["print_loss"] - float(g["print_loss"])) <= 1e-5 * abs(float(g["print_loss"]))
    _check_grads(r["grads"], g, "v")
    np.testing.assert_allclose(r["llh"], g["llh"][2:], rtol=1e-5)
    for k, ref in (("z_q", "z"), ("z_log_prob_q", "z_log_prob"), ("x_mean_q", "x_mean")):
        np.testing.assert_allclose(r["fwd"][k], g["fwd." + ref], rtol=1e-4, atol=1e-5, err_msg=k)


def test_oracle_quirk_pass_without_inside_draw():
    """p pass with every |eps| > 1: identity flow (z = eps), no gradient into t from that pass."""
    g = _load("flow_quirk_reg.npz")
    assert np.all(np.abs(g["eps"][1]) > 1) and np.any(np.abs(g["eps"][0]) <= 1)
    P = _params(g)
    for alpha in (1.0, 0.5):
        r = FO.step(P, g["x"], g["mask"], g["mask_p"], g["eps"], alpha=alpha)
        assert abs(r["loss"] - float(g[f"loss.a{alpha}"])) <= 1e-5 * abs(float(g[f"loss.a{alpha}"]))
        _check_grads(r["grads"], g, f"a{alpha}")
    np.testing.assert_array_equal(g["fwd.z_p"], g["eps"][1])
    np.testing.assert_allclose(r["fwd"]["z_p"], g["fwd.z_p"])


def test_oracle_trajectory_matches_reference():
    for kind in ("reg", "van"):
        g = _load(f"flow_traj_{kind}_d12.npz")
        P = {k: v.astype(np.float64) for k, v in _params(g, "param0.").items()}
        m1 = {k: np.zeros_like(P[k]) for k in FO.TRAINABLE}
        m2 = {k: np.zeros_like(P[k]) for k in FO.TRAINABLE}
        for s in range(5):
            r = FO.step(P, g["x"], g["mask"], g["mask_p"][s] if kind == "reg" else None, g["eps"][s],
                        alpha=float(g["alpha"]))
            assert abs(r["loss"] - g["losses"][s]) <= 2e-5 * abs(g["losses"][s]), (kind, s)
            for k in FO.TRAINABLE:  # torch.optim.Adam(lr=1e-3)
                gr = r["grads"][k]
                m1[k] = 0.9 * m1[k] + 0.1 * gr
                m2[k] = 0.999 * m2[k] + 0.001 * gr * gr
                P[k] = P[k] - 1e-3 * (m1[k] / (1 - 0.9 ** (s + 1))) / (np.sqrt(m2[k] / (1 - 0.999 ** (s + 1))) + 1e-8)
        for k in FO.TRAINABLE:
            np.testing.assert_allclose(P[k], g["param5." + k], atol=2e-5, err_msg=(kind, k))


@pytest.mark.parametrize("reg,stage,alpha", [(True, "train", 0.5), (True, "train", 1.0), (True, "evaluate", 0.5),
                                             (False, "train", 0.0)])
def test_closed_form_equals_autograd_hid500(reg, stage, alpha):
    d, H, B = 12, 500, 16
    P = FO.init_params(d, H, seed=3)
    rng = np.random.default_rng(5)
    x = rng.random((B, d))
    mask = rng.random((B, d)) < 0.7
    mask_p = mask & (rng.random((B, d)) < 0.7) if reg else None
    eps = rng.standard_normal((2 if reg else 1, B, FO.L))
    r = FO.step(P, x, mask, mask_p, eps, alpha=alpha, stage=stage)
    tl, tg = FO.torch_step(P, x, mask, mask_p, eps, alpha=alpha, stage=stage)
    assert abs(r["loss"] - tl) <= 1e-10 * abs(tl)
    for k in FO.TRAINABLE:
        err = np.max(np.abs(r["grads"][k] - tg[k])) / (np.max(np.abs(tg[k])) + 1e-30)
        assert err < 1e-9, (k, err)


def test_flow_backward_equals_autograd():
    """flow_bwd alone, with outside draws, against autograd of the torch restatement."""
    import torch
    rng = np.random.default_rng(11)
    B = 9
    t = rng.standard_normal((B, 100)) * 2
    eps = rng.standard_normal((B, FO.L)) * 1.3
    dz, dzlp = rng.standard_normal((B, FO.L)), rng.standard_normal((B, FO.L))
    z, zlp, cache = FO.flow_fwd(t, eps)
    tt = torch.tensor(t, requires_grad=True)
    zt, zlpt = FO._torch_flow(tt, torch.tensor(eps))
    np.testing.assert_allclose(z, zt.detach().numpy(), atol=1e-12)
    np.testing.assert_allclose(zlp, zlpt.detach().numpy(), atol=1e-12)
    (zt * torch.tensor(dz) + zlpt * torch.tensor(dzlp)).sum().backward()
    np.testing.assert_allclose(FO.flow_bwd(cache, dz, dzlp), tt.grad.numpy(), atol=1e-10)
