"""CPU checks of the float64 MIWAE oracle (tests/miwae_oracle.py): it reproduces the vectors recorded from the reference
(tests/golden/miwae_*.npz), its closed-form gradients match torch autograd, and the two pairings it states differ."""
import numpy as np
import pytest
import torch

import miwae_oracle as O
from conftest import load_golden


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-12)


def _grad_err(got, ref):
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


@pytest.mark.parametrize("name", ["miwae_reg_d14", "miwae_reg_d40", "miwae_van_d14", "miwae_van_d40"])
def test_oracle_reproduces_reference(name):
    g = load_golden(name + ".npz")
    reg = "reg" in name
    x, mask = _t(g["x"]), _t(g["mask"])
    mask_p = _t(g["mask_p"]) if reg else None
    eps = [_t(e) for e in g["eps"]]
    cases = [(a, f"loss.a{a}", f"a{a}") for a in (1.0, 0.5, 0.0)] if reg else [(0.0, "loss", "v")]
    for alpha, lk, gk in cases:
        p = O.params64(g, requires_grad=True)
        lo, _, q, pp = O.run(p, x, mask, mask_p, eps, alpha)
        assert _rel(lo.item(), g[lk]) < 1e-5, (alpha, lo.item(), float(g[lk]))
        lo.backward()
        for k in O.KEYS:
            assert _grad_err(p[k].grad, _t(g[f"grad.{gk}.{k}"]).double()) < 1e-4, (alpha, k)
    # forward outputs and the llh_eval branch
    p = O.params64(g)
    lo, a_q, q, pp = O.run(p, x, mask, mask_p, eps, 0.5)
    tag = "_q" if reg else ""
    assert torch.allclose(q[0][0], _t(g[f"fwd.x_mean{tag}"]).double(), atol=1e-5)
    assert torch.allclose(q[0][2], _t(g[f"fwd.deg_free{tag}"]).double(), atol=1e-4)
    el = [_t(e) for e in g["eps_llh"]]
    lo_l, a_l = O.loss(x, mask, mask_p, q, pp, el, 0.5)
    assert _rel(lo_l.item(), g["llh_loss"]) < 1e-5
    xm = O.impute(a_l, q[0][0])
    assert torch.allclose(xm, _t(g["llh_xm"]).double(), atol=1e-5)
    if not reg:  # logpxobsgivenz_imp.sum() / (B * 5000)
        lp = O.student_lp(x.double()[:, None, :], *q[0])
        third = (lp * (~mask).double()[:, None, :]).sum() / (x.shape[0] * 5000)
        assert _rel(third.item(), g["llh_third"]) < 1e-5


def _random_case(B, S, d, Ld, reg, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = r(B, d)
    mask = r(B, d) < 0.7
    mask_p = mask & (r(B, d) < 0.5) if reg else None

    def one():
        dec = (torch.sigmoid(n(B, S, d)).requires_grad_(), (0.05 + r(B, S, d)).requires_grad_(),
               (3 + 5 * r(B, S, d)).requires_grad_())
        return dec, n(B, Ld).requires_grad_(), (0.2 + r(B, Ld)).requires_grad_()

    q = one()
    p = one() if reg else None
    eps2 = [n(B, S, Ld) for _ in range(2 if reg else 1)]
    return x, mask, mask_p, q, p, eps2


@pytest.mark.parametrize("reg", [True, False])
@pytest.mark.parametrize("pairing", ["reference", "per_row"])
def test_closed_form_gradients_match_autograd(reg, pairing):
    x, mask, mask_p, q, p, eps2 = _random_case(7, 3, 9, 4, reg, 5 if reg else 6)
    alpha = 0.3
    lo, _ = O.loss(x, mask, mask_p, q, p, eps2, alpha, pairing)
    leaves = [*q[0], q[1], q[2]] + ([*p[0], p[1], p[2]] if reg else [])
    auto = torch.autograd.grad(lo, leaves)
    cf = O.closed_form_grads(x, mask, mask_p, q, p, eps2, alpha, pairing)
    flat = [t for pas in cf for t in pas]
    for i, (a, c) in enumerate(zip(auto, flat)):
        assert torch.allclose(a, c, rtol=1e-9, atol=1e-12), (i, float((a - c).abs().max()))


def test_pairings_differ():
    """B = 7, S = 3: the reference's mixed pairing and the per-row pairing give different losses (the pairing tests
    mean something); at B = 1 they agree."""
    for reg in (True, False):
        x, mask, mask_p, q, p, eps2 = _random_case(7, 3, 9, 4, reg, 11)
        a = O.loss(x, mask, mask_p, q, p, eps2, 0.5, "reference")[0].item()
        b = O.loss(x, mask, mask_p, q, p, eps2, 0.5, "per_row")[0].item()
        assert abs(a - b) > 1e-3 * abs(a), (reg, a, b)
        x, mask, mask_p, q, p, eps2 = _random_case(1, 3, 9, 4, reg, 12)
        a = O.loss(x, mask, mask_p, q, p, eps2, 0.5, "reference")[0].item()
        b = O.loss(x, mask, mask_p, q, p, eps2, 0.5, "per_row")[0].item()
        assert a == b


def test_per_row_equals_single_row_calls():
    x, mask, mask_p, q, p, eps2 = _random_case(5, 4, 6, 3, True, 13)
    with torch.no_grad():
        _, a_all = O.loss(x, mask, mask_p, q, p, eps2, 0.5, "per_row")
        xm_all = O.impute(a_all, q[0][0])
        for j in range(5):
            sl = lambda t: t[j:j + 1]
            qj = (tuple(sl(t) for t in q[0]), sl(q[1]), sl(q[2]))
            pj = (tuple(sl(t) for t in p[0]), sl(p[1]), sl(p[2]))
            _, a_j = O.loss(sl(x), sl(mask), sl(mask_p), qj, pj, [sl(e) for e in eps2], 0.5, "reference")
            assert torch.allclose(O.impute(a_j, qj[0][0]), xm_all[j:j + 1], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_oracle_adam_trajectory(kind):
    g = load_golden(f"miwae_traj_{kind}_d14.npz")
    p = O.params64(g, "param0.", requires_grad=True)
    opt = torch.optim.Adam(list(p.values()), lr=0.001)
    x, mask = _t(g["x"]), _t(g["mask"])
    for s in range(5):
        eps = [_t(e) for e in g["eps"][s]]
        mp = _t(g["mask_p"][s]) if kind == "reg" else None
        lo = O.run(p, x, mask, mp, eps, 0.5)[0]
        assert _rel(lo.item(), g["losses"][s]) < 1e-4, (s, lo.item(), g["losses"][s])
        opt.zero_grad()
        lo.backward()
        opt.step()
    for k in O.KEYS:
        ref = _t(g["param5." + k]).double()
        assert float((p[k].detach() - ref).abs().max()) < 1e-4, k
