"""CPU checks of the flow-path oracle (tests/flow_oracle.py): it reproduces the fixtures recorded from the reference
(tests/golden/make_golden_flow.py) and its closed-form gradients equal torch autograd of the same restatement, at the
config's hid_dim 500 included; and what the kernel-parity cases (tests/flow_cases.py) lean on: forced decisions reproduce
the free ones, closed-form flow_bwd equals autograd on those grids, the flagged shares, the loss restatement.  No GPU, no
HIP library."""
import itertools
import os

import numpy as np
import pytest
import torch

import flow_cases as C
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


# ------------------------------------------------------------------------------------------------ the kernel-parity cases
# (tests/flow_cases.py, compared on the GPU by tests/test_flow_kernels_gpu.py): what the GPU tests lean on is asserted
# here, on the oracle alone
GRID = [(B, P, s) for (B, P) in C.FLOW_SHAPES for s in C.SIGMAS]


def _case_refs():
    yield from ((k, C.grid_reference(*k), k[0], k[1]) for k in GRID)
    for ps, idx in C.PLACEMENTS:
        yield (ps, idx), C.reference(C.placement_inputs(ps, idx), C.PLACE_B, 2), C.PLACE_B, 2
    for s in C.SIGMAS:
        yield ("planted", s), C.reference(C.planted_inputs(s), C.PLANT_B, 1), C.PLANT_B, 1


def test_forced_decisions_equal_free_decisions():
    """flow_fwd / flow_bwd given the decisions they returned, and alternative 0, reproduce themselves bit for bit."""
    for key, ref, B, P in _case_refs():
        for p, sl in enumerate(C._passes(B, P)):
            cache = ref["caches"][p]
            if cache is None:
                continue
            for dec in (cache[4], FO.alternative(cache, ref["flags"][p], 0)):
                z, zlp, c2 = FO.flow_fwd(ref["t"][sl], ref["eps"][sl], dec)
                assert np.array_equal(z, ref["z64"][sl]) and np.array_equal(zlp, ref["zlp64"][sl]), key
                assert np.array_equal(FO.flow_bwd(c2, ref["dzs"][sl], ref["dzlp"][sl]), ref["dt64"][sl]), key
            assert np.array_equal(cache[4]["bins"][0], FO.bin_of(ref["eps"][sl] * cache[0])), key


def test_closed_form_flow_bwd_equals_autograd_on_the_kernel_grids():
    for key, ref, B, P in _case_refs():
        for dec in (None, [None if c is None else c[4] for c in ref["caches"]]):
            z, zlp, dt = C.torch_flow(torch.from_numpy(ref["t"]), torch.from_numpy(ref["eps"]),
                                      torch.from_numpy(ref["dzs"]), torch.from_numpy(ref["dzlp"]), B, P, dec)
            np.testing.assert_allclose(z.numpy(), ref["z64"], atol=1e-12, err_msg=str(key))
            np.testing.assert_allclose(zlp.numpy(), ref["zlp64"], rtol=1e-12, atol=1e-12, err_msg=str(key))
            np.testing.assert_allclose(dt.numpy(), ref["dt64"], rtol=1e-9, atol=1e-9 * np.abs(ref["dt64"]).max(),
                                       err_msg=str(key))


def test_an_alternative_moves_only_flagged_elements():
    """Switching the flagged decisions leaves every unflagged element's z_log_prob and dt block as they were, and z
    (continuous across a knot and a clamp) within 1e-4 everywhere."""
    B, P = 257, 2
    ref = C.grid_reference(B, P, C.WIDE)
    moved = 0
    for c in (1, 2, 4, 8, 16, 31):
        zlp, dt = C.alternative_reference(ref, B, P, c)
        keep = ~ref["flagged"]
        assert np.array_equal(zlp[keep], ref["zlp64"][keep])
        assert np.array_equal(dt.reshape(-1, FO.L, FO.L)[keep], ref["dt64"].reshape(-1, FO.L, FO.L)[keep])
        moved += int((zlp != ref["zlp64"]).sum()) + int((dt != ref["dt64"]).sum())
        for p, sl in enumerate(C._passes(B, P)):
            z = FO.flow_fwd(ref["t"][sl], ref["eps"][sl], FO.alternative(ref["caches"][p], ref["flags"][p], c))[0]
            assert np.abs(z - ref["z64"][sl]).max() < 1e-4
    assert moved > 0


def test_flagged_shares_of_the_kernel_grids():
    """Narrow logits: at most 1e-3 of the inside elements carry a flag, over each sigma's whole grid (the numerator
    counts every splined element, so this is the stricter reading).  Wide logits: every case keeps at least 10 % of its
    inside elements unflagged, every z_log_prob is finite and some pdf[bin] is below 1e-20."""
    for s in C.NARROW:
        tot = np.sum([C.flag_counts(C.grid_reference(B, P, s)) for B, P in C.FLOW_SHAPES], 0)
        print(f"sigma {s}: {tot[0]} flagged of {tot[2]} inside elements ({tot[0] / tot[2]:.1e})")
        assert tot[0] <= 1e-3 * tot[2], (s, tot)
    tot, minpdf = np.zeros(3), 1.0
    for B, P in C.FLOW_SHAPES:
        ref = C.grid_reference(B, P, C.WIDE)
        n = C.flag_counts(ref)
        tot += n
        assert n[1] >= 0.1 * n[2] and n[2] > 0, ((B, P), n)
        assert np.isfinite(ref["zlp64"]).all() and np.isfinite(ref["zlp32"]).all() and np.isfinite(ref["dt32"]).all()
        minpdf = min([minpdf] + [float(st[2].min()) for c in ref["caches"] for st in c[3]])
    print(f"sigma {C.WIDE}: {int(tot[0])} flagged, {int(tot[1])} unflagged inside of {int(tot[2])} inside; min pdf[bin] {minpdf:.1e}")
    assert minpdf < 1e-20
    # the placement and planted cases: narrow logits too, except the wide planted one.  A row with no inside draw has a
    # zero context, so all its elements sit at 0 -> bin position 5.0, an exact tie, and are flagged: with the uniform
    # pdf of such a row neither bin changes z_log_prob, and its dt rows are masked to zero, so the flag frees nothing
    for key, ref, B, P in _case_refs():
        if key[0] in ("q", "p") or (key[0] == "planted" and key[1] != C.WIDE):
            n = int((ref["flagged"] & ref["inside"].any(1, keepdims=True)).sum())
            # planted: +-1 and their inside neighbours land on o = 0 / 1 (the clamp gate) and from there on bin position 0 / 10
            assert n <= (4 if key[0] == "planted" else 2), (key, n)


def test_placement_and_planted_inputs_are_what_they_claim():
    for ps, idx in C.PLACEMENTS:
        ins = (np.abs(C.placement_inputs(ps, idx)["eps"]) <= 1).reshape(2, -1)
        k = "qp".index(ps)
        assert not ins[1 - k].any()
        if idx is None:
            assert ins[k].sum() > 1000
        else:
            assert ins[k].sum() == 1 and ins[k, idx]
    v = C.planted_values()
    eps = C.planted_inputs(1.0)["eps"].reshape(-1)
    assert sorted(eps[:v.size].tolist()) == sorted(v.tolist()) and v.size == 36
    bins = FO.bin_of(np.sort(v[:33]).reshape(11, 3))   # per knot: below, at, above; fp32 decides which side a neighbour is
    assert all(set(bins[k]) <= {max(k - 1, -1), min(k, 9)} for k in range(11)), bins
    assert len({tuple(b - k) for k, b in enumerate(bins[1:10], 1)}) > 1   # and it does not decide alike at every knot
    inf = np.isinf(C.reference(C.underflow_inputs(), C.UNDER_B, 2)["zlp32"])
    assert inf.any() and not inf.all()


def test_loss_restatement_against_autograd_and_numpy():
    """FO.loss_terms in float64: the loss equals the numpy formulas of FO.step, the closed-form gradients equal autograd
    (ungated; gated = the same times x_mean (1 - x_mean)), and a z_log_prob tie has sign 0."""
    for (B, d), kind, alpha, beta in [((5, 9), "reg", 0.5, 0.25), ((3, 65), "reg", 1.0, 1.0), ((4, 1), "reg_eval", 0.5, 0.25),
                                      ((5, 9), "van", 0.0, 0.25)]:
        inp = C.loss_inputs(B, d)
        r = C.loss_reference(inp, kind, alpha, beta, 0, 1.0 / B, torch.float64)
        f = {k: ([a.astype(np.float64) for a in v] if isinstance(v, list) else v.astype(np.float64)) for k, v in inp.items()}
        kl = lambda k: np.sum(f["zlp"][k] + f["z"][k] ** 2 / 2 + FO.HL)
        loss_q = np.sum(FO.nll(f["x"], f["xm"][0], f["m"])) + beta * kl(0)
        loss = loss_q
        if kind == "reg":
            loss_p = np.sum(FO.nll(f["x"], f["xm"][1], f["mp"])) + beta * kl(1)
            loss = loss_q + alpha * (np.sum(np.abs(f["zlp"][0] - f["zlp"][1])) - loss_q + loss_p +
                                     np.sum(FO.nll(f["x"], f["xm"][0], f["m"] * (1 - f["mp"]))))
        assert abs(r["out8"][0].item() - loss) <= 1e-12 * r["abs8"][0].item()
        assert abs(r["out8"][7].item() - np.sum(FO.nll(f["x"], f["xm"][0], 1 - f["m"]))) <= 1e-12 * r["abs8"][7].item()
        leaves = [torch.from_numpy(a).double().requires_grad_() for a in (*inp["xm"], *inp["z"], *inp["zlp"])]
        c = lambda a: torch.from_numpy(a).double()
        t = FO.loss_terms(c(inp["x"]), c(inp["m"]), None if kind == "van" else c(inp["mp"]), leaves[0:2], leaves[2:4],
                          leaves[4:6], alpha, beta, "evaluate" if kind == "reg_eval" else "train", 0, 1.0 / B)
        auto = torch.autograd.grad(t["out8"][0] / B, leaves, allow_unused=True)
        for g, a in zip(r["grads"], auto):
            a = torch.zeros_like(g) if a is None else a
            assert float((g - a).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))
        gated = C.loss_reference(inp, kind, alpha, beta, 1, 1.0 / B, torch.float64)["grads"]
        for k in range(2):
            assert torch.equal(gated[k], r["grads"][k] * (c(inp["xm"][k]) * (1 - c(inp["xm"][k]))))
        if kind == "reg":
            ties = torch.from_numpy(inp["ties"])
            assert ties.any() and bool((r["grads"][4][ties] == (1 - alpha) * beta / B).all())
            assert bool((r["grads"][5][ties] == alpha * beta / B).all())


def test_loss_cases_cover_every_value_with_every_kind():
    cs = C.LOSS_CASES
    for kind in C.KINDS:
        mine = [c for c in cs if c["kind"] == kind]
        assert {(c["d"], c["B"]) for c in mine} == set(itertools.product(C.LOSS_D, C.LOSS_B))
        for key, vals in (("alpha", C.ALPHAS), ("beta", C.BETAS), ("gated", (0, 1))):
            assert {c[key] for c in mine} == set(vals), (kind, key)
            for dim, dvals in (("d", C.LOSS_D), ("B", C.LOSS_B)):   # and each d / B meets both gated values and betas
                if key != "alpha":
                    assert {(c[dim], c[key]) for c in mine} == set(itertools.product(dvals, vals)), (kind, dim, key)
