"""CPU checks of the float64 MIWAE oracle (tests/miwae_oracle.py): it reproduces the vectors recorded from the reference
(tests/golden/miwae_*.npz), its closed-form gradients match torch autograd, the two pairings it states differ, and the
helpers the GPU kernel tests lean on hold: the out8 terms, the restatements of the elementwise kernels, the gated run,
the seeds of tests/miwae_cases.py."""
import numpy as np
import pytest
import torch

import miwae_cases as C
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


@pytest.mark.parametrize("reg", [True, False])
@pytest.mark.parametrize("pairing", ["reference", "per_row"])
def test_terms_compose_the_loss(reg, pairing):
    """terms()[0] is loss(), built from its own entries as the kernel builds out8[0]; the third value is the golden's."""
    x, mask, mask_p, q, p, eps2 = _random_case(7, 3, 9, 4, reg, 21)
    alpha = 0.3
    with torch.no_grad():
        t = O.terms(x, mask, mask_p, q, p, eps2, alpha, pairing)
        lo = O.loss(x, mask, mask_p, q, p, eps2, alpha, pairing)[0]
    assert abs(t[0].item() - lo.item()) <= 1e-13 * abs(lo.item())
    assert t[1].item() == -t[6].item() / 7 and t[2].item() == -t[7].item() / 7
    if reg:
        assert abs((t[1] + alpha * (t[3] - t[1] + t[2] - t[4])).item() - t[0].item()) <= 1e-13 * abs(t[0].item())
        assert t[3].item() > 0 and t[4].item() != 0
    else:
        assert t[0].item() == t[1].item() and [t[k].item() for k in (2, 3, 4, 7)] == [0.0] * 4
    g = load_golden("miwae_van_d14.npz")
    pr = O.params64(g)
    xg, mg = _t(g["x"]), _t(g["mask"])
    _, _, qg, _ = O.run(pr, xg, mg, None, [_t(e) for e in g["eps"]], 0.5)
    tg = O.terms(xg, mg, None, qg, None, [_t(e) for e in g["eps_llh"]], 0.5)
    assert _rel(tg[5].item(), g["llh_third"]) < 1e-5 and _rel(tg[0].item(), g["llh_loss"]) < 1e-5


@pytest.mark.parametrize("given", ["dz+eps+g", "dz+eps", "g", "dz+g"])
def test_sample_backward_matches_autograd(given):
    """sample_bwd / softplus_d against autograd through sample(), threshold values included."""
    R, S, Ld = 5, 4, 3
    i = C.sample_inputs(R, S, Ld)
    heads = _t(i["heads"]).double().requires_grad_()
    eps = _t(i["eps"]).double() if "eps" in given else None
    dz = _t(i["dz"]).double() if "dz" in given else None
    g = _t(i["g_hact"]).double() if "g" in given.split("+") else None
    z, hact = O.sample(heads, eps, S)
    assert z.shape == (R, S, Ld)
    if eps is None:
        assert torch.equal(z, heads.detach()[:, None, :Ld].expand(R, S, Ld))
    obj = (0 if dz is None else (z * dz).sum()) + (0 if g is None else (hact * g).sum())
    auto, = torch.autograd.grad(obj, heads)
    cf = O.sample_bwd(dz, eps, heads.detach(), g, S)
    assert torch.allclose(auto, cf, rtol=1e-12, atol=1e-300), float((auto - cf).abs().max())
    assert (i["heads"][:3, Ld] == np.array([20, np.nextafter(np.float32(20), np.float32(99)),
                                            np.nextafter(np.float32(20), np.float32(0))], np.float32)).all()


def test_heads_backward_matches_autograd():
    i = C.heads_inputs(5, 3)
    y = _t(i["y"]).double().requires_grad_()
    gup = _t(i["g"]).double()
    act = O.heads_act(y)
    d = 3
    mu, sc, v = C.raw_to_act(i["y"], d)
    assert torch.equal(act.detach(), torch.cat([mu, sc, v], 1))
    auto, = torch.autograd.grad((act * gup).sum(), y)
    cf = O.heads_bwd(y.detach(), gup)
    # autograd's sigmoid backward is s (1 - s): its 1 - s carries one rounding of 1 (2^-53), so near s = 1 the closed form,
    # which never forms 1 - s, is the more accurate of the two and the two agree to that absolute error only
    assert torch.allclose(auto[:, :d], cf[:, :d], rtol=1e-12, atol=2.0 ** -52 * float(gup.abs().max()))
    assert torch.allclose(auto[:, d:], cf[:, d:], rtol=1e-12, atol=1e-300), float((auto - cf).abs().max())
    # the threshold is torch's: identity strictly above 20
    t = torch.tensor([20.0, float(np.nextafter(np.float32(20), np.float32(99)))], dtype=torch.float64)
    assert O.softplus_d(t)[1].item() == 1.0 and O.softplus_d(t)[0].item() < 1.0


@pytest.mark.parametrize("reg", [True, False])
def test_gated_run_with_its_own_gates_is_the_plain_run(reg):
    """run(gates=, stats=): given the float64 gates themselves nothing is taken over and loss and gradients are those of
    the plain run; a flipped gate outside the band is counted as a mismatch and not taken."""
    c = C.model_case(4, 3, 5, 2, reg, 3)
    p, x, m, mp, eps = C.oracle_inputs(c)
    lo = O.run(p, x, m, mp, eps, 0.3)[0]
    ref = torch.autograd.grad(lo, [p[k] for k in O.KEYS])
    gates = {}

    def own(pre, h, n):
        out = {}
        for i in (0, 2):
            a = torch.nn.functional.linear(h, p[f"{pre}.{i}.weight"], p[f"{pre}.{i}.bias"])
            out[i], h = (a > 0).reshape(n, -1), torch.relu(a)
        return out

    with torch.no_grad():
        for tag, mk, e in (("q", m, eps[0]), ("p", mp, eps[1]))[:2 if reg else 1]:
            gates["enc_" + tag] = own("seq_encoder", x.double() * mk.double(), 4)
            gates["dec_" + tag] = own("seq_decoder", O.encode(p, x, mk, e)[2], 12)
    stats = O.new_gate_stats()
    lo2 = O.run(p, x, m, mp, eps, 0.3, gates=gates, stats=stats)[0]
    got = torch.autograd.grad(lo2, [p[k] for k in O.KEYS])
    assert lo2.item() == lo.item() and all(torch.equal(a, b) for a, b in zip(got, ref))
    assert stats["units"] == (2 if reg else 1) * (4 + 12) * 2 * C.HID
    assert stats["taken_from_device"] == 0 and stats["mismatch_outside"] == 0
    with torch.no_grad():
        pre = torch.nn.functional.linear(x.double() * m.double(), p["seq_encoder.0.weight"], p["seq_encoder.0.bias"])
    far = int(pre.abs().reshape(-1).argmax())
    gates["enc_q"][0].view(-1)[far] ^= True
    stats = O.new_gate_stats()
    assert O.run(p, x, m, mp, eps, 0.3, gates=gates, stats=stats)[0].item() == lo.item()
    assert stats["mismatch_outside"] == 1 and stats["taken_from_device"] == 0


@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("shape", list(C.TRAINER_CASES))
def test_trainer_case_seeds_keep_the_kink_band_small(shape, kind):
    """The condition the GPU test of MIWTrainer.step relies on, on the oracle alone: at most 1e-4 of the hidden units
    (rounded up) have a float64 pre-activation within KINK_BAND of their layer's max."""
    p, x, m, mp, eps = C.oracle_inputs(C.trainer_case(shape, kind))
    stats = O.new_gate_stats()
    with torch.no_grad():
        O.run(p, x, m, mp, eps, C.ALPHA, stats=stats)
    B, S = shape[:2]
    assert stats["units"] == (2 if kind == "reg" else 1) * (B + B * S) * 2 * C.HID
    assert stats["in_band"] <= C.band_limit(stats["units"]), stats


def test_loss_case_distributions():
    """The wide head distribution reaches what it is for: df on both sides of the digamma recurrence's end (6) and raw
    heads on both sides of the softplus threshold; the narrow one is the draw the single-shape test always used."""
    x, m, mp, oq, op, e = C.rand_inputs(33, 7, 64, 5, 106, "wide")
    d = 64
    df = C.raw_to_act(oq[0], d)[2]
    assert df.min() < 3.001 and df.max() > 40 and ((df + 1) / 2 < 6).any() and (df / 2 > 6).any()
    assert (oq[0][:, d:] > 20).any() and oq[0].min() >= -75 and (op[2] >= 0.05).all() and (op[2] <= 3).all()
    assert ((mp <= m).all()) and e.shape == (2, 33, 7, 5)
    rng = np.random.default_rng(9)
    xn = C.rand_inputs(33, 7, 70, 5, 9)[0]
    assert np.array_equal(xn, rng.random((33, 70)).astype(np.float32))
