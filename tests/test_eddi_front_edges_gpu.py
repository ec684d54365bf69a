"""The narrow point-net front-end (csrc/vpc_eddi.hip: vpc_eddi_fold, vpc_eddi_front_fwd, vpc_eddi_front_bwd with its tail
eddi_reduce_kernel + eddi_param_bwd_kernel) against float64 at every instantiation of the backward kernel, on both sides of
every boundary of its dispatch, and at row counts that make the grid-stride loops iterate (tests/eddi_front_cases.py; its
soundness is tests/test_eddi_front_cases_cpu.py).

a. every EDGE and STRIDE case, one mask and stacked passes: every output filled with NaN first and fenced by 64 sentinel floats
   on both sides, the scratch a view of exactly vpc_eddi_front_scratch() floats, fenced too; afterwards the fences are intact,
   everything is finite, the agg row of an unobserved row is exactly 0, and agg / the four gradients lie within 1e-5 / 2e-5 of
   the float64 tensor's OWN maximum (no floor of 1; the bounds and their sqrt(n) 2^-24 argument are those of
   tests/test_eddi_mnist_gpu.py).  vpc_eddi_fold is held elementwise to (K + 2) 2^-24 S, S the magnitude sum of the K + 1 term
   dot product (the a-priori bound of a recursive fp32 sum).  The worst error / bound per instantiation and output is printed
   when the module ends (`pytest -s`, or -rA).
b. equalities without a tolerance: the backward run twice; the stacked forward against the two single-mask forwards; accumulate
   onto a random prior against prior + fresh in fp32; mask bytes 0xFF and 2 against 1; exact against oversized scratch.
c. the argument guards of the three entry points: VpcError, nothing written.
d. the launch chain around the front-end (EDDITrainer with VPC_STEP_SMALL=0, and the API path) at the new variants against
   EDDIPort, at the bounds of tests/test_latent_widths_gpu.py.
"""
import numpy as np
import pytest
import torch

import eddi_front_cases as fc
from oracle import eddi_oracle as EO

pytestmark = pytest.mark.gpu
DEV = "cuda"
FENCE, FENCE_VALUE = 64, -12345.678
SHAPES = lambda d, K: ((d, K), (d, 1), (K, 2 + K), (K,))  # gE, gtb, gWp, gcp
OUTPUTS = ("fold", "agg") + fc.GRAD_KEYS
SHORT = dict(zip(OUTPUTS, ("fold", "agg") + fc.GRAD_NAMES))
WORST = {}  # (group, (T, KP), output) -> worst error / bound
LOSS_RTOL, GRAD_RTOL = 2e-5, 2e-4  # tests/latent_cases.py


@pytest.fixture(scope="module")
def ed():
    import vpc_amd
    from vpc_amd import eddi
    return eddi


def _cus():
    from vpc_amd import _lib
    return _lib.num_cus()


@pytest.fixture(scope="module")
def cus():
    return _cus()


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    print("\nEDDIFRONT worst error / bound per instantiation <T, KP> and output (fold: (K + 2) 2^-24 S elementwise; agg: 1e-5 of max; "
          "gradients: 2e-5 of max)")
    print("EDDIFRONT " + " ".join(f"{h:>10s}" for h in ("cases", "<T,KP>", "fold", "agg", "gE", "gtb", "gWp", "gcp")))
    for group in ("EDGE", "STRIDE"):
        for v in sorted(fc.VARIANTS):
            row = [WORST.get((group, v, o)) for o in OUTPUTS]
            if any(r is not None for r in row):
                print("EDDIFRONT " + " ".join([f"{group:>10s}", f"{'<%d,%d>' % v:>10s}"] +
                                             [f"{'-' if r is None else '%.3f' % r:>10s}" for r in row]))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Fenced:
    """A tensor of `shape` between two fences of FENCE floats, filled with NaN (or a copy of `init`)."""

    def __init__(self, shape, init=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * FENCE,), FENCE_VALUE, device=DEV)
        self.t = self.buf[FENCE:FENCE + n].view(*shape)
        if init is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(init)
        self.n = n

    def intact(self):
        return bool((self.buf[:FENCE] == FENCE_VALUE).all()) and bool((self.buf[FENCE + self.n:] == FENCE_VALUE).all())


def launch(ed, c, passes, mask_byte=1, prior=None, extra_scratch=0):
    """fold, forward and backward of the passes `passes` ((0,), (1,) or (0, 1): stacked) of case c through vpc_amd.eddi.
    Returns (AC, agg, [gE, gtb, gWp, gcp]) after checking every fence and that the scratch was the one passed in."""
    from vpc_amd._lib import lib
    B, d, K = c.B, c.d, c.K
    R = len(passes) * B
    masks = [_dev((c.m, c.m2)[p].astype(np.uint8) * mask_byte) for p in passes]
    dagg = _dev(np.concatenate([c.dagg[p * B:(p + 1) * B] for p in passes], 0))
    x, E, tb, Wp, cp = (_dev(a) for a in (c.x, c.E, c.tb, c.Wp, c.cp))
    m2 = masks[1] if len(passes) == 2 else None
    AC, agg = Fenced((2, K, d)), Fenced((R, K))
    ed.eddi_fold(E, tb, Wp, cp, AC.t, d, K)
    ed.eddi_front_fwd(x, masks[0], AC.t, agg.t, B, d, K, mask2_u8=m2)
    need = int(lib().vpc_eddi_front_scratch(R, d, K))
    assert need == (fc.bwd_blocks(R, _cus()) + 1) * 2 * K * d
    sc = Fenced((need + extra_scratch,))
    gs = [Fenced(s, None if prior is None else prior[i]) for i, s in enumerate(SHAPES(d, K))]
    ed.eddi_front_bwd(x, masks[0], AC.t, dagg, E, tb, Wp, *[g.t for g in gs], B, d, K, accumulate=prior is not None, mask2_u8=m2,
                      scratch=sc.t)
    torch.cuda.synchronize()
    for name, f in zip(("AC", "agg", "scratch", "gE", "gtb", "gWp", "gcp"), [AC, agg, sc] + gs):
        assert f.intact(), f"{c.what}: a write outside {name}"
    # every partial block and the reduced (dA | dC) are written in full: the scratch rule is exactly what the launch uses
    assert bool(torch.isfinite(sc.t[:need]).all()) and bool(torch.isnan(sc.t[need:]).all()), c.what
    return AC.t, agg.t, [g.t for g in gs]


def check_case(ed, c, passes, group):
    """a. of the module docstring for one launch set; returns the failures (every figure is recorded and printed first)."""
    B, d, K = c.B, c.d, c.K
    v = fc.variant(d, K)
    what = f"{c.what} passes={passes}"
    AC, agg, gs = launch(ed, c, passes)
    for name, t in zip(("AC", "agg") + fc.GRAD_KEYS, [AC, agg] + gs):
        assert bool(torch.isfinite(t).all()), f"{what}: {name} is not finite"
    if len(passes) == 2:
        ref_agg, ref_g = c.stacked()
    else:
        ref_agg, ref_g = c.ref[passes[0]]
    agg_np = agg.cpu().numpy()
    unobserved = np.concatenate([~(c.m, c.m2)[p].any(1) for p in passes])
    assert (B <= 2 or unobserved[0]) and not agg_np[unobserved].any(), f"{what}: agg of an unobserved row is not exactly 0"
    figs = {}
    ac_ref, S = fc.fold_ref(c)
    err = np.abs(AC.cpu().numpy().astype(np.float64) - ac_ref)
    bound = (K + 2) * 2.0 ** -24 * S
    figs["fold"] = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    figs["agg"] = fc.rel_err(agg_np, ref_agg) / fc.AGG_TOL
    for k, g in zip(fc.GRAD_KEYS, gs):
        figs[k] = fc.rel_err(g.cpu().numpy(), ref_g[k]) / fc.GRAD_TOL
    for o, f in figs.items():
        key = (group, v, o)
        WORST[key] = max(WORST.get(key, 0.0), f)
    print(f"EDDIFIG {group} <{v[0]},{v[1]}> {what}: " + " ".join(f"{SHORT[o]}={f:.3f}" for o, f in figs.items()))
    return [(what, o, f) for o, f in figs.items() if not f <= 1.0]


# ------------------------------------------------------------------------------------------------ a. against float64
@pytest.mark.parametrize("d,K", fc.EDGE_SHAPES)
def test_edge_cases_vs_float64(ed, d, K):
    bad = []
    for d_, K_, B, two, xd in fc.EDGE:
        if (d_, K_) == (d, K):
            c = fc.edge_case(d, K, B, two, xd)
            assert c.removed <= fc.KINK_CAP
            bad += check_case(ed, c, (0, 1) if two else (0,), "EDGE")
    assert not bad, bad


@pytest.mark.parametrize("stacked", [False, True], ids=["one_mask", "stacked"])
@pytest.mark.parametrize("d,K", fc.STRIDE)
def test_stride_cases_vs_float64(ed, cus, d, K, stacked):
    c = fc.stride_case(d, K, cus)
    assert c.removed <= fc.KINK_CAP
    R = (2 if stacked else 1) * c.B
    # the loops iterate: forward waves take a second (third) row, the backward prefetch runs, a stacked stride crosses passes
    assert fc.loop_trips(R, cus) == (((2, 3), (4, 5)) if stacked else ((1, 2), (2, 3))) and c.B % (12 * cus) == 3
    bad = check_case(ed, c, (0, 1) if stacked else (0,), "STRIDE")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ b. equalities
def _same(a, b, what):
    for name, s, t in zip(("AC", "agg", "gE", "gtb", "gWp", "gcp"), [a[0], a[1]] + a[2], [b[0], b[1]] + b[2]):
        assert torch.equal(s, t), f"{what}: {name} differs, max {float((s - t).abs().max()):.3e}"


def _equalities(ed, c):
    base = launch(ed, c, (0, 1))
    _same(launch(ed, c, (0, 1)), base, f"{c.what}: run twice")
    p0, p1 = launch(ed, c, (0,)), launch(ed, c, (1,))
    assert torch.equal(base[1][:c.B], p0[1]) and torch.equal(base[1][c.B:], p1[1]), f"{c.what}: stacked forward vs single-mask forwards"
    _same(launch(ed, c, (0,)), p0, f"{c.what}: one mask, run twice")
    gen = torch.Generator().manual_seed(c.d * 100 + c.K)
    for passes, fresh in (((0, 1), base), ((0,), p0)):
        prior = [(torch.randn(*s, generator=gen) * 3.0).to(DEV) for s in SHAPES(c.d, c.K)]
        acc = launch(ed, c, passes, prior=prior)
        for name, got, pr, fr in zip(("gE", "gtb", "gWp", "gcp"), acc[2], prior, fresh[2]):
            assert torch.equal(got, pr + fr), f"{c.what} passes={passes}: accumulate {name} is not prior + fresh"
    for byte in (0xFF, 2):
        _same(launch(ed, c, (0, 1), mask_byte=byte), base, f"{c.what}: mask byte {byte}")
    _same(launch(ed, c, (0, 1), extra_scratch=4097), base, f"{c.what}: oversized scratch")
    _same(launch(ed, c, (0,), extra_scratch=1), p0, f"{c.what}: scratch one float larger")


@pytest.mark.parametrize("d,K", fc.STRIDE)
def test_stride_equalities(ed, cus, d, K):
    _equalities(ed, fc.stride_case(d, K, cus))


@pytest.mark.parametrize("d,K", fc.EDGE_SHAPES)
def test_edge_equalities(ed, d, K):
    for B in (1, 37):
        _equalities(ed, fc.edge_case(d, K, B, True, "uniform"))


# ------------------------------------------------------------------------------------------------ c. guards
def test_guards_return_before_any_launch(ed):
    """d = 0 / 129, K = 0 / 33, B = 0, a scratch one float short, a null x / AC / dagg (and a null mask / output): VpcError from
    every entry point that takes the argument, and not one byte of any output or of the scratch written."""
    import vpc_amd
    from vpc_amd._lib import check, lib, ptr, stream_ptr
    B, d, K = 5, 8, 4
    g = torch.Generator().manual_seed(0)
    x, E, tb = torch.rand(B, d, generator=g).to(DEV), torch.randn(d, K, generator=g).to(DEV), torch.randn(d, 1, generator=g).to(DEV)
    Wp, cp, dagg = torch.randn(K, 2 + K, generator=g).to(DEV), torch.randn(K, generator=g).to(DEV), torch.randn(2 * B, K, generator=g).to(DEV)
    m = (torch.rand(B, d, generator=g) < 0.6).to(torch.uint8).to(DEV)
    need = int(lib().vpc_eddi_front_scratch(2 * B, d, K))
    assert need == 4 * 2 * K * d and int(lib().vpc_eddi_front_scratch(B, d, K)) == 3 * 2 * K * d
    for bad in ((0, d, K), (-1, d, K), (B, 0, K), (B, d, 0)):
        assert int(lib().vpc_eddi_front_scratch(*bad)) == 0
    AC_in = torch.empty(2, K, d, device=DEV)
    ed.eddi_fold(E, tb, Wp, cp, AC_in, d, K)
    outs = {n: torch.full(s, FENCE_VALUE, device=DEV) for n, s in
            (("AC", (2, K, d)), ("agg", (2 * B, K)), ("scratch", (need,)), ("gE", (d, K)), ("gtb", (d, 1)), ("gWp", (K, 2 + K)), ("gcp", (K,)))}

    def fold(d_=d, K_=K, E_=E, AC_=outs["AC"]):
        check(lib().vpc_eddi_fold(ptr(E_), ptr(tb), ptr(Wp), ptr(cp), ptr(AC_), d_, K_, stream_ptr()), "vpc_eddi_fold")

    def fwd(B_=B, d_=d, K_=K, x_=x, m_=m, AC_=AC_in, agg_=outs["agg"], m2_=m):
        check(lib().vpc_eddi_front_fwd(ptr(x_), ptr(m_), ptr(m2_), ptr(AC_), ptr(agg_), B_, d_, K_, stream_ptr()), "vpc_eddi_front_fwd")

    def bwd(B_=B, d_=d, K_=K, x_=x, m_=m, AC_=AC_in, dagg_=dagg, sc_=outs["scratch"], n_=need, gE_=outs["gE"], m2_=m, acc=0):
        check(lib().vpc_eddi_front_bwd(ptr(x_), ptr(m_), ptr(m2_), ptr(AC_), ptr(dagg_), ptr(E), ptr(tb), ptr(Wp), ptr(sc_), n_,
                                       ptr(gE_), ptr(outs["gtb"]), ptr(outs["gWp"]), ptr(outs["gcp"]), acc, B_, d_, K_, stream_ptr()),
              "vpc_eddi_front_bwd")

    calls = []
    for kw in (dict(d_=0), dict(d_=129), dict(d_=-1), dict(K_=0), dict(K_=33), dict(K_=-1)):
        calls += [(fold, kw), (fwd, kw), (bwd, kw), (bwd, dict(kw, acc=1))]
    for kw in (dict(B_=0), dict(B_=-1), dict(x_=None), dict(AC_=None), dict(m_=None)):
        calls += [(fwd, kw), (bwd, kw)]
    calls += [(fold, dict(E_=None)), (fold, dict(AC_=None)), (fwd, dict(agg_=None)), (bwd, dict(dagg_=None)), (bwd, dict(sc_=None)),
              (bwd, dict(gE_=None)), (bwd, dict(n_=need - 1)), (bwd, dict(n_=0)),
              (bwd, dict(m2_=None, n_=int(lib().vpc_eddi_front_scratch(B, d, K)) - 1)),
              (bwd, dict(n_=int(lib().vpc_eddi_front_scratch(B, d, K))))]  # enough for one pass, short for two
    for fn, kw in calls:
        with pytest.raises(vpc_amd.VpcError):
            fn(**kw)
    torch.cuda.synchronize()
    for n, t in outs.items():
        assert bool((t == FENCE_VALUE).all()), f"a refused call wrote to {n}"
    # (the same calls with nothing wrong run: the guards above refused the argument, not the set-up)
    fold(), fwd(), bwd()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) and not bool((t == FENCE_VALUE).any()) for t in outs.values())
    # the Python wrapper replaces a scratch that is too small by one of its own instead of passing it on
    gs = [torch.full(s, float("nan"), device=DEV) for s in SHAPES(d, K)]
    small = torch.full((need - 1,), FENCE_VALUE, device=DEV)
    ed.eddi_front_bwd(x, m, AC_in, dagg, E, tb, Wp, *gs, B, d, K, mask2_u8=m, scratch=small)
    assert bool((small == FENCE_VALUE).all()) and all(torch.equal(a, outs[n]) for a, n in zip(gs, ("gE", "gtb", "gWp", "gcp")))


# ------------------------------------------------------------------------------------------------ d. the chain around it
TP = {"batch_size": 64, "patience": 100}
CHAIN_SHAPES = ((64, 16, 37), (65, 11, 130), (33, 32, 5), (128, 20, "12cus+5"))  # (d, K, B): <1,16>, <2,16>, <1,32>, <2,20> with 2 rows per wave


def _inputs(B, d, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, d, generator=g)
    mk = torch.rand(B, d, generator=g) < 0.7
    mp = mk & (torch.rand(B, d, generator=g) < 0.7)
    return (x, mk, mp) + tuple(torch.randn(B, L, generator=g) for _ in range(3))


def _port_step(p, L, kind, x, mk, mp, eq, ep, eml):
    rt = "ml_reg" if kind == "ml_reg" else "kl_reg"
    port = EO.EDDIPort(p, L, rt)
    if kind == "kl_reg":
        o = port.reg_forward(x, mk, mp, eq, ep)
        _, ref = port.reg_loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mk, mp, 1, alpha=0.5, beta=1.0)
    elif kind == "ml_reg":
        o = port.reg_forward(x, mk, mp, eq, ep)
        _, ref = port.reg_loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mk, mp, 1400, alpha=0.8, beta=0.9, eps_ml=eml)
    else:
        o = port.vanilla_forward(x, mk, eq)
        _, ref = port.vanilla_loss(x, o[2], o[3], o[0], o[1], 1, mk)
    ref.backward()
    return ref


def _check_grads(model, p, loss, ref, what):
    le = abs(loss - ref.item()) / abs(ref.item())
    errs = {}
    for k, prm in model.named_parameters():
        if k in p:
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), (what, k)
            errs[k] = fc.rel_err(prm.grad.cpu().numpy(), p[k].grad.numpy())
    print(f"EDDICHAIN {what}: loss {le:.2e} (tol {LOSS_RTOL:.0e}), worst gradient {max(errs.values()):.2e} (tol {GRAD_RTOL:.0e})")
    assert set(errs) == set(EO.EDDI_KEYS)
    assert le <= LOSS_RTOL, (what, loss, ref.item())
    for k, e in errs.items():
        assert e < GRAD_RTOL, (what, k, e)


@pytest.mark.parametrize("kind", ["kl_reg", "ml_reg", "vanilla"])
@pytest.mark.parametrize("d,K,B", CHAIN_SHAPES, ids=[f"d{d}_K{K}_B{B}" for d, K, B in CHAIN_SHAPES])
def test_chain_step_vs_port(cus, monkeypatch, d, K, B, kind):
    """One EDDITrainer step on the launch chain (VPC_STEP_SMALL=0) against EDDIPort, as
    tests/test_latent_widths_gpu.test_eddi_trainer_vs_port: loss 2e-5 relative, every gradient 2e-4 of its maximum."""
    import vpc_amd as vpc
    L = 10
    B = 12 * cus + 5 if B == "12cus+5" else B
    monkeypatch.setenv("VPC_STEP_SMALL", "0")
    seed = 1000 * L + 7 * d + B + K
    x, mk, mp, eq, ep, eml = _inputs(B, d, L, seed)
    torch.manual_seed(seed)
    rt = "ml_reg" if kind == "ml_reg" else "kl_reg"
    model = vpc.vanilla_EDDI(d, 500, K, L, TP, "exp") if kind == "vanilla" else vpc.Reg_EDDI(d, 500, K, L, TP, "exp", rt)
    p = {k: v.detach().clone().float().requires_grad_(True) for k, v in model.state_dict().items() if k in EO.EDDI_KEYS}
    model = model.to(DEV)
    ref = _port_step(p, L, kind, x, mk, mp, eq, ep, eml)
    tr = vpc.EDDITrainer(model, lr=1e-3)
    if kind == "kl_reg":
        tr.step(x.to(DEV), mk.to(DEV), mask_p=mp.to(DEV), eps_q=eq.to(DEV), eps_p=ep.to(DEV), epoch=1, alpha=0.5)
    elif kind == "ml_reg":
        tr.step(x.to(DEV), mk.to(DEV), mask_p=mp.to(DEV), eps_q=eq.to(DEV), eps_p=ep.to(DEV), eps_ml=eml.to(DEV), epoch=1400,
                alpha=0.8, beta=0.9)
    else:
        tr.step(x.to(DEV), mk.to(DEV), eps_q=eq.to(DEV), epoch=1)
    assert tr.last_path == "chain"
    _check_grads(model, p, tr.loss_value(), ref, f"chain {kind} d={d} K={K} B={B} <%d,%d>" % fc.variant(d, K))


def test_api_path_vs_port():
    """Reg_EDDI.forward -> loss -> backward (EDDIEncoderFn: the front-end with the wrapper's own scratch) at d = 65, K = 16, the
    <2,16> instantiation, against EDDIPort with the same eps."""
    import vpc_amd as vpc
    d, K, B, L = 65, 16, 37, 10
    x, mk, mp, eq, ep, eml = _inputs(B, d, L, 6516)
    torch.manual_seed(6516)
    model = vpc.Reg_EDDI(d, 500, K, L, TP, "exp", "kl_reg")
    p = {k: v.detach().clone().float().requires_grad_(True) for k, v in model.state_dict().items() if k in EO.EDDI_KEYS}
    model = model.to(DEV)
    ref = _port_step(p, L, "kl_reg", x, mk, mp, eq, ep, eml)
    xd, md, mpd = x.to(DEV), mk.to(DEV), mp.to(DEV)
    draws = iter([eq.to(DEV), ep.to(DEV), eml.to(DEV)])
    orig = torch.randn
    torch.randn = lambda *a, **k: next(draws)
    try:
        o = model.forward(xd, md, mpd, "train")
        _, tl = model.loss(xd, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], md, mpd, 1, alpha=0.5, beta=1.0)
    finally:
        torch.randn = orig
    tl.backward()
    _check_grads(model, p, tl.item(), ref, f"API path d={d} K={K} B={B}")
