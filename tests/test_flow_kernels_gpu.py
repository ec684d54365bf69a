"""The flow kernels (csrc/vpc_flow.hip, csrc/vpc_flow_device.h) against float64 at their edges, kernel by kernel:
  1. vpc_flow_fwd / vpc_flow_bwd on tests/flow_cases.FLOW_SHAPES with narrow (sigma 0.5, 1) and concentrated (sigma 8)
     logits, a pass's only inside draw in every chunk position, the spline knots and the inside / outside threshold
     planted, logits that underflow expf, every subset of the upstream gradients, padded pitches, the guards;
  2. vpc_flow_loss on the cross of d and B with reg (train / evaluate) and vanilla: all of out8, loss_f32, accum, the six
     gradients, exact 0 / 1 in x_mean under the Sigmoid gate, z_log_prob ties, masks at the extremes, padded pitches,
     the guards;
  3. vpc_flow_prep: the stacked encoder input exactly, the mask_p forms, and its device draws bit for bit against
     vpc_nm_prep / vpc_fill_normal (the same Philox counters: group index + offset, stream 0 / 1).
Elementwise outputs are bounded per block by 8 x the error the same expression has in fp32 torch on the CPU, floor 2^-21
of the block's max (the rule of tests/test_miwae_kernels_gpu.py).  The flow's discrete decisions (the bin of layers 2 / 3,
each layer's clamp gate) are the float64 oracle's; an element whose decision is a tie in fp32 (tests/flow_oracle.py
flow_flags; how many there are is asserted on the CPU, tests/test_flow_oracle.py) must meet the same bound in
(z_log_prob, its dt row) under some assignment of its flagged decisions.  z is continuous and gets no leeway; layer 1's
bin is flow_oracle.bin_of(eps) and gets none either."""
import math

import numpy as np
import pytest
import torch

import flow_cases as C
import flow_oracle as FO

pytestmark = pytest.mark.gpu
SENT = 12345.0
MARGIN = 64
FLOOR = 2.0 ** -21
CTX, L = 100, 10
WORST = {}   # kernel -> largest kernel error / fp32-torch error seen in this session (printed)


@pytest.fixture(scope="module")
def fl():
    import vpc_amd
    from vpc_amd import flow
    return flow


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(*shape, fill=SENT, dtype=torch.float32):
    """An output of `shape` with MARGIN sentinel elements behind it: (whole buffer, the output view)."""
    n = math.prod(shape)
    buf = torch.full((n + MARGIN,), SENT, device="cuda", dtype=dtype)
    buf[:n] = fill
    return buf, buf[:n].view(*shape)


def _margin_intact(*bufs):
    return all(bool((b[-MARGIN:] == SENT).all()) for b in bufs)


def _bound(kernel, what, name, got, r64, r32, keep=None):
    """(bound, |got - r64|) of one block: 8 x the error of fp32 torch, floor 2^-21 of the block's max.  The ratio of the
    kernel's error to fp32 torch's is printed and recorded, over the elements of `keep` (all by default)."""
    got, r64, r32 = np.asarray(got, np.float64), np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    mx = float(np.abs(r64).max())
    err = np.abs(got - r64)
    kept = err if keep is None else err[keep]
    ek, e32 = float(kept.max()) if kept.size else 0.0, float(np.abs(r32 - r64).max())
    bound = max(8.0 * e32, FLOOR * mx)
    ratio = ek / e32 if e32 > 0 else (0.0 if ek == 0 else float("inf"))
    if math.isfinite(ratio):
        WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print(f"{kernel} {what} {name}: kernel {ek:.3e} fp32 torch {e32:.3e} (ratio {ratio:.2f}, largest so far "
          f"{WORST.get(kernel, 0.0):.2f}) block max {mx:.3e} bound {bound:.3e}")
    return bound, err


def _bounded(kernel, what, name, got, r64, r32):
    bound, err = _bound(kernel, what, name, got, r64, r32)
    assert float(err.max()) <= bound, (kernel, what, name, float(err.max()), bound)


# ------------------------------------------------------------------------------------------------ 1. flow_fwd / flow_bwd
def _run_flow(fl, inp, B, P, given=C.ALL, ldt=CTX, lddt=CTX, fwd=True, bwd=True):
    """Both kernels on the device; t's pad columns hold NaN, dt's the sentinel; a margin behind every output."""
    R = B * P
    t = torch.full((R, ldt), float("nan"), device="cuda")
    t[:, :CTX] = _dev(inp["t"])
    eps = _dev(inp["eps"])
    zbuf, z = _guarded(R, L)
    lbuf, zlp = _guarded(R, L)
    dbuf, dt = _guarded(R, lddt)
    if fwd:
        fl.flow_fwd(t, eps, z, zlp, R, B, ldt=ldt)
    if bwd:
        g = lambda k: _dev(inp[k]) if k in given else None
        fl.flow_bwd(t, eps, g("dz"), g("dz2"), g("dzlp"), dt, R, B, ldt=ldt, lddt=lddt)
    torch.cuda.synchronize()
    assert _margin_intact(zbuf, lbuf, dbuf)
    assert bool((dt[:, CTX:] == SENT).all())
    return dict(z=z.cpu().numpy(), zlp=zlp.cpu().numpy(), dt=dt[:, :CTX].cpu().numpy())


def _check_flow(what, got, ref, B, P, fwd=True, bwd=True):
    """z everywhere; z_log_prob and dt (per pass) by the plain bound on unflagged elements, and on flagged ones under
    some assignment of their flagged decisions."""
    R = B * P
    flagged = ref["flagged"]
    ok = np.ones((R, L), bool)           # element meets the z_log_prob and dt bounds under the oracle's own decisions
    bounds = {}
    if fwd:
        _bounded("flow_fwd", what, "z", got["z"], ref["z64"], ref["z32"])
        bounds["zlp"], err = _bound("flow_fwd", what, "z_log_prob", got["zlp"], ref["zlp64"], ref["zlp32"], ~flagged)
        ok &= err <= bounds["zlp"]
    if bwd:
        for p, sl in enumerate(C._passes(B, P)):
            bounds[p], err = _bound("flow_bwd", what, f"dt pass {p}", got["dt"][sl], ref["dt64"][sl], ref["dt32"][sl],
                                    np.repeat(~flagged[sl], L, 1))
            ok[sl] &= err.reshape(B, L, L).max(-1) <= bounds[p]
    assert ok[~flagged].all(), (what, "unflagged elements past the bound", np.argwhere(~ok & ~flagged)[:8].tolist())
    todo = ~ok & flagged
    print(f"{what}: {int(flagged.sum())} flagged elements, {int(todo.sum())} of them need another assignment")
    for c in range(1, FO.N_ALTERNATIVES):
        if not todo.any():
            break
        zlp, dt = C.alternative_reference(ref, B, P, c)
        meets = np.ones((R, L), bool)
        if fwd:
            meets &= np.abs(got["zlp"] - zlp) <= bounds["zlp"]
        if bwd:
            for p, sl in enumerate(C._passes(B, P)):
                meets[sl] &= np.abs(got["dt"][sl] - dt[sl]).reshape(B, L, L).max(-1) <= bounds[p]
        todo &= ~meets
    assert not todo.any(), (what, "flagged elements past the bound under every assignment", np.argwhere(todo)[:8].tolist())


@pytest.mark.parametrize("sigma", C.SIGMAS)
@pytest.mark.parametrize("shape", C.FLOW_SHAPES)
def test_flow_grid_vs_float64(fl, shape, sigma):
    B, P = shape
    _check_flow((shape, sigma), _run_flow(fl, C.flow_inputs(B, P, sigma), B, P), C.grid_reference(B, P, sigma), B, P)


@pytest.mark.parametrize("place", C.PLACEMENTS)
def test_flow_inside_draw_placement(fl, place):
    """A pass's only inside draw in the first chunk, at a chunk's last and first element, in the last full chunk, in the
    partial one and at the very end; the other pass has none: z = eps bit for bit, z_log_prob = log N(eps), dt rows 0."""
    B = C.PLACE_B
    inp = C.placement_inputs(*place)
    got = _run_flow(fl, inp, B, 2)
    ref = C.reference(inp, B, 2)
    _check_flow(place, got, ref, B, 2)
    sl = C._passes(B, 2)[1 - "qp".index(place[0])]
    assert ref["caches"][1 - "qp".index(place[0])] is None
    assert np.array_equal(got["z"][sl].view(np.uint32), inp["eps"][sl].view(np.uint32))
    assert not got["dt"][sl].any()
    assert not np.array_equal(got["z"][C._passes(B, 2)["qp".index(place[0])]], inp["eps"][C._passes(B, 2)["qp".index(place[0])]])


@pytest.mark.parametrize("sigma", C.SIGMAS)
def test_flow_planted_knots(fl, sigma):
    """eps on the spline knots, their fp32 neighbours, the inside / outside threshold +- 1 ulp, +-0.0 and 5.0: layer 1's
    bin is the oracle's fp32 bin_of, the mask is |eps| <= 1."""
    B = C.PLANT_B
    inp = C.planted_inputs(sigma)
    _check_flow(("planted", sigma), _run_flow(fl, inp, B, 1), C.reference(inp, B, 1), B, 1)


def test_flow_underflow_row(fl):
    """exp(-120) = 0 in fp32: z_log_prob is +inf exactly where fp32 torch's is (the taken bin's pdf is 0) and finite
    elsewhere; z and dt hold no NaN."""
    B = C.UNDER_B
    inp = C.underflow_inputs()
    got = _run_flow(fl, inp, B, 2)
    ref = C.reference(inp, B, 2)
    pinf = np.isposinf(ref["zlp32"])
    assert pinf.any() and np.array_equal(np.isposinf(got["zlp"]), pinf)
    assert np.isfinite(got["zlp"][~pinf]).all()
    assert np.isfinite(got["z"]).all() and np.isfinite(got["dt"]).all()
    _bounded("flow_fwd", "underflow", "z", got["z"], ref["z64"], ref["z32"])


@pytest.mark.parametrize("given", C.GIVEN, ids=lambda g: "+".join(g) or "none")
def test_flow_bwd_optional_gradients(fl, given):
    """An absent dz / dz2 / dz_log_prob is a zero gradient; none at all: dt is all zero."""
    B, P = 37, 2
    inp = C.flow_inputs(B, P, 1.0)
    got = _run_flow(fl, inp, B, P, given, fwd=False)
    _check_flow(("given", given), got, C.reference(inp, B, P, given), B, P, fwd=False)
    if not given:
        assert not got["dt"].any()
    else:
        assert got["dt"].any()


@pytest.mark.parametrize("sigma", [1.0, C.WIDE])
@pytest.mark.parametrize("shape", [(26, 2), (257, 1)])
def test_flow_padded_pitch_is_bit_equal(fl, shape, sigma):
    """ldt = 104 (NaN in t's pad columns) and lddt = 112: bit-equal to the dense run, dt's pad columns untouched."""
    B, P = shape
    inp = C.flow_inputs(B, P, sigma)
    dense, pad = _run_flow(fl, inp, B, P), _run_flow(fl, inp, B, P, ldt=104, lddt=112)
    for k in ("z", "zlp", "dt"):
        assert np.array_equal(dense[k].view(np.uint32), pad[k].view(np.uint32)), k


@pytest.mark.parametrize("guard", ["ldt", "lddt", "R_mod_B", "three_passes", "no_t", "no_eps", "no_z", "no_zlp", "no_dt"])
def test_flow_guards(fl, guard):
    """Each bad argument raises before any launch: the outputs keep their fill."""
    B, R = 2, 4
    inp = C.flow_inputs(3, 2, 1.0)   # six rows: enough for R = 6
    kw = dict(t=_dev(inp["t"]), eps=_dev(inp["eps"]), R=R, B=B, ldt=CTX, lddt=CTX)
    zbuf, z = _guarded(6, L)
    lbuf, zlp = _guarded(6, L)
    dbuf, dt = _guarded(6, CTX)
    out = dict(z=z, zlp=zlp, dt=dt)
    if guard == "ldt":
        kw["ldt"] = CTX - 1
    elif guard == "lddt":
        kw["lddt"] = CTX - 1
    elif guard == "R_mod_B":
        kw["R"] = 5
    elif guard == "three_passes":
        kw["R"] = 6
    else:
        (kw if guard[3:] in kw else out)[guard[3:]] = None
    g = _dev(inp["dz"])
    if guard not in ("lddt", "no_dt"):
        with pytest.raises(fl.L.VpcError):
            fl.flow_fwd(kw["t"], kw["eps"], out["z"], out["zlp"], kw["R"], kw["B"], ldt=kw["ldt"])
    if guard not in ("no_z", "no_zlp"):
        with pytest.raises(fl.L.VpcError):
            fl.flow_bwd(kw["t"], kw["eps"], g, g, g, out["dt"], kw["R"], kw["B"], ldt=kw["ldt"], lddt=kw["lddt"])
    torch.cuda.synchronize()
    assert bool((zbuf == SENT).all()) and bool((lbuf == SENT).all()) and bool((dbuf == SENT).all())


# ------------------------------------------------------------------------------------------------ 2. vpc_flow_loss
GRAD_NAMES = ("g x_mean q", "g x_mean p", "g z q", "g z p", "g z_log_prob q", "g z_log_prob p")
OUT8_NAMES = ("loss", "RE_q", "RE_p", "KL_q", "KL_p", "KL_reg", "NLL_r", "RE_q_imputed")
OUT8_WORST = {}


def _run_loss(fl, inp, c, grads=True, ldxm=None, ldg=None, loss_f32=True, accum=None):
    """vpc_flow_loss on the device: x_mean's pad columns hold NaN, those of its gradients the sentinel."""
    B, d, kind = c["B"], c["d"], c["kind"]
    reg = kind != "van"
    ldxm, ldg = ldxm or d, ldg or d
    P = 2 if reg else 1

    def xm_buf(a):
        t = torch.full((B, ldxm), float("nan"), device="cuda")
        t[:, :d] = _dev(a)
        return t

    pair = lambda k, f=_dev: [f(a) for a in inp[k][:P]] + [None] * (2 - P)
    bufs, g = [], None
    if grads:
        g = []
        for shape in ((B, ldg), (B, L), (B, L)):
            for p in range(2):
                buf, view = _guarded(*shape) if p < P else (None, None)
                bufs.append(buf)
                g.append(view)
    out8 = torch.full((8,), SENT, dtype=torch.float64, device="cuda")
    lf = torch.full((1,), SENT, device="cuda") if loss_f32 else None
    gscale = float(np.float32(1.0 / B))
    fl.flow_loss(_dev(inp["x"]), _dev(inp["m"]), _dev(inp["mp"]) if reg else None, pair("xm", xm_buf), pair("z"),
                 pair("zlp"), g, fl.flow_loss_scratch(B, "cuda"), out8, lf, accum, B, d,
                 fl.STAGE_EVAL if kind == "reg_eval" else fl.STAGE_TRAIN, c["alpha"], c["beta"], gscale, c["gated"],
                 ldxm=ldxm, ldg=ldg)
    torch.cuda.synchronize()
    assert _margin_intact(*[b for b in bufs if b is not None])
    return dict(out8=out8.cpu(), loss_f32=None if lf is None else lf.cpu(), g=g, gscale=gscale)


def _check_loss(what, got, inp, c, grads=True):
    B, d = c["B"], c["d"]
    args = (inp, c["kind"], c["alpha"], c["beta"], c["gated"], got["gscale"])
    r64, r32 = C.loss_reference(*args, torch.float64), C.loss_reference(*args, torch.float32)
    for k, name in enumerate(OUT8_NAMES):
        ref, scale, v = r64["out8"][k].item(), r64["abs8"][k].item(), got["out8"][k].item()
        rel = abs(v - ref) / scale if scale > 0 else (0.0 if v == 0.0 else float("inf"))
        OUT8_WORST[name] = max(OUT8_WORST.get(name, 0.0), rel)
        print(f"flow_loss {what} out8 {name}: {v!r} oracle {ref!r} |terms| {scale:.3e} rel {rel:.2e} "
              f"(largest so far {OUT8_WORST[name]:.2e})")
        assert rel <= 2e-5, (what, name, v, ref, scale)
    if got["loss_f32"] is not None:
        assert got["loss_f32"].item() == float(np.float32(got["out8"][0].item() / B)), what
    if not grads:
        return
    P = 1 if c["kind"] == "van" else 2
    for k, name in enumerate(GRAD_NAMES):
        if k % 2 < P:
            view = got["g"][k][:, :d] if k < 2 else got["g"][k]
            _bounded("flow_loss", what, name, view.cpu().numpy(), r64["grads"][k].numpy(), r32["grads"][k].numpy())
            if k < 2:
                assert bool((got["g"][k][:, d:] == SENT).all()), (what, name, "pad columns")
    if c["kind"] == "reg_eval":   # the p pass does not enter the loss
        assert all(not bool(got["g"][k][:, :d if k == 1 else L].any()) for k in (1, 3, 5)), what
    if c["kind"] == "reg":        # a z_log_prob tie: sign 0 in both gradients, exactly
        ties = torch.from_numpy(inp["ties"])
        gs, al, be = np.float32(got["gscale"]), np.float32(c["alpha"]), np.float32(c["beta"])
        assert bool((got["g"][4].cpu()[ties] == float(gs * ((np.float32(1) - al) * be))).all()), (what, "tie q")
        assert bool((got["g"][5].cpu()[ties] == float(gs * (al * be))).all()), (what, "tie p")
    if c["gated"]:                # x_mean exactly 0 or 1: the Sigmoid gate closes
        assert got["g"][0].reshape(-1)[0].item() == 0.0 and got["g"][0][B - 1, d - 1].item() == 0.0, what


def _loss_case(fl, inp, c, what, **pitch):
    """With gradients (loss_f32 given, accum preloaded: the step's loss is added), then forward only (neither)."""
    accum = torch.full((1,), 3.5, device="cuda")
    got = _run_loss(fl, inp, c, accum=accum, **pitch)
    _check_loss(what, got, inp, c)
    assert accum.item() == float(np.float32(3.5) + np.float32(got["loss_f32"].item())), (what, accum.item())
    fwd = _run_loss(fl, inp, c, grads=False, loss_f32=False, **pitch)
    _check_loss((what, "forward only"), fwd, inp, c, grads=False)
    assert torch.equal(fwd["out8"], got["out8"]), what
    return got


@pytest.mark.parametrize("shape", C.LOSS_SHAPES)
def test_loss_grid_vs_float64(fl, shape):
    d, B = shape
    inp = C.loss_inputs(B, d)
    for c in C.LOSS_CASES:
        if (c["d"], c["B"]) == shape:
            _loss_case(fl, inp, c, tuple(c.values()))


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("masks", C.MASK_CASES)
def test_loss_masks_at_the_extremes(fl, masks, kind):
    B, d = 5, 65
    inp = C.loss_inputs(B, d, masks)
    for gated in (0, 1):
        c = dict(d=d, B=B, kind=kind, alpha=0.5, beta=0.25, gated=gated)
        got = _loss_case(fl, inp, c, (masks, kind, gated))
        if masks == "none_observed":
            assert not bool(got["g"][0].any())
        if masks in ("mask_p_is_mask", "none_observed") and kind != "van":   # NLL_r: every weight 0, the constant alone
            assert abs(got["out8"][6].item() - B * d * FO.HL) <= 2e-5 * B * d * FO.HL


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", C.PITCH_SHAPES)
def test_loss_padded_pitch_is_bit_equal(fl, shape, kind):
    """ldxm = d + 3 (NaN in x_mean's pad columns), ldg = d + 5: bit-equal to the dense run, the pad columns of both
    x_mean gradients untouched."""
    d, B = shape
    inp = C.loss_inputs(B, d)
    c = dict(d=d, B=B, kind=kind, alpha=0.5, beta=0.25, gated=1)
    dense = _run_loss(fl, inp, c)
    pad = _loss_case(fl, inp, c, ("pitch", shape, kind), ldxm=d + 3, ldg=d + 5)
    assert torch.equal(pad["out8"], dense["out8"]) and torch.equal(pad["loss_f32"], dense["loss_f32"])
    for k in range(6):
        if dense["g"][k] is not None:
            assert torch.equal(pad["g"][k][:, :d] if k < 2 else pad["g"][k], dense["g"][k]), k


@pytest.mark.parametrize("guard", ["scratch_short", "scratch_misaligned", "ldxm", "ldg", "stage", "no_xm_p", "no_z_p",
                                   "no_zlp_p", "no_gz_q", "no_gzlp_q", "no_gxm_p", "no_gz_p", "no_gzlp_p"])
def test_loss_guards(fl, guard):
    """Each bad argument raises before any launch: out8 keeps its fill."""
    B, d = 5, 9
    inp = C.loss_inputs(B, d)
    e = lambda *s: torch.empty(*s, device="cuda")
    sc = fl.flow_loss_scratch(B, "cuda")
    nbytes = sc.numel() * sc.element_size()
    xm, z, zlp = ([_dev(a) for a in inp[k]] for k in ("xm", "z", "zlp"))
    g = [e(B, d), e(B, d), e(B, L), e(B, L), e(B, L), e(B, L)]
    kw = dict(ldxm=d, ldg=d)
    stage = fl.STAGE_TRAIN
    if guard == "scratch_short":
        sc = sc.view(torch.uint8)[:nbytes - 1]
    elif guard == "scratch_misaligned":
        sc = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")[4:4 + nbytes]
        assert sc.data_ptr() % 8 == 4
    elif guard in kw:
        kw[guard] = d - 1
    elif guard == "stage":
        stage = 2
    elif guard in ("no_xm_p", "no_z_p", "no_zlp_p"):
        {"no_xm_p": xm, "no_z_p": z, "no_zlp_p": zlp}[guard][1] = None
    else:
        g[["gxm_q", "gxm_p", "gz_q", "gz_p", "gzlp_q", "gzlp_p"].index(guard[3:])] = None
    out8 = torch.full((8,), SENT, dtype=torch.float64, device="cuda")
    with pytest.raises(fl.L.VpcError):
        fl.flow_loss(_dev(inp["x"]), _dev(inp["m"]), _dev(inp["mp"]), xm, z, zlp, g, sc, out8, None, None, B, d, stage, 0.5,
                     1.0, 1.0 / B, 0, **kw)
    torch.cuda.synchronize()
    assert bool((out8 == SENT).all())


# ------------------------------------------------------------------------------------------------ 3. vpc_flow_prep
def _run_prep(fl, inp, B, d, mode, n_eps=0, seed=7, offset=11, offset_eps=1 << 40, keep=0.6):
    two = mode != "vanilla"
    xbuf, xin = _guarded((2 if two else 1) * B, 2 * d)
    mbuf, mp_out = _guarded(B, d)
    ebuf, eps = _guarded(max(n_eps, 1))
    fl.flow_prep(_dev(inp["x"]), _dev(inp["m"]), _dev(inp["mp"]) if mode in ("mask_p_in", "mask_p_in_out") else None,
                 mp_out if mode in ("mask_p_in_out", "mask_p_out") else None, xin, eps[:n_eps] if n_eps else None, B, d, keep,
                 seed, offset, offset_eps)
    torch.cuda.synchronize()
    assert _margin_intact(xbuf, mbuf, ebuf)
    if n_eps == 0:
        assert bool((ebuf == SENT).all())
    if mode in ("vanilla", "mask_p_in"):
        assert bool((mbuf == SENT).all())
    return xin.cpu(), mp_out.cpu(), eps[:n_eps].cpu()


@pytest.mark.parametrize("n_eps", [0, 10, 37 * 10 + 3])
@pytest.mark.parametrize("mode", C.PREP_MODES)
@pytest.mark.parametrize("shape", C.PREP_SHAPES)
def test_prep_stacked_input_is_exact(fl, shape, mode, n_eps):
    """xin = [x * m | m] and, with a mask_p, the p half [x * mask_p | mask_p], exactly; a given mask_p is copied through
    to mask_p_out; a drawn one is a sub-mask of mask."""
    B, d = shape
    inp = C.prep_inputs(B, d)
    xin, mp_out, eps = _run_prep(fl, inp, B, d, mode, n_eps)
    x, m = torch.from_numpy(inp["x"]), torch.from_numpy(inp["m"])
    assert torch.equal(xin[:B], torch.cat([x * m, m], 1))
    if mode != "vanilla":
        mp = torch.from_numpy(inp["mp"]) if mode != "mask_p_out" else mp_out
        if mode != "mask_p_in":
            assert torch.equal(mp_out, mp)
        assert bool(((mp == 0) | ((mp == 1) & (m == 1))).all())
        assert torch.equal(xin[B:], torch.cat([x * mp, mp], 1))
    assert bool(torch.isfinite(eps).all())


@pytest.mark.parametrize("shape", C.PREP_SHAPES)
def test_prep_draws_equal_the_shared_draw_entry_points(fl, shape):
    """The device draws repeat bit for bit for a (seed, offset), move with the offset, and equal what vpc_nm_prep (mask_p:
    Philox counter = group-of-four index + offset, stream 0) and vpc_fill_normal (eps: flat groups of four + offset_eps,
    stream 1) write for the same seed and counters."""
    B, d = shape
    n_eps = 2 * B * L + 3
    inp = C.prep_inputs(B, d)
    _, mp1, e1 = _run_prep(fl, inp, B, d, "mask_p_out", n_eps)
    _, mp2, e2 = _run_prep(fl, inp, B, d, "mask_p_out", n_eps)
    _, mp3, e3 = _run_prep(fl, inp, B, d, "mask_p_out", n_eps, offset=12, offset_eps=(1 << 40) + 1)
    assert torch.equal(mp1, mp2) and torch.equal(e1, e2)
    assert not torch.equal(e1, e3) and (B * d < 64 or not torch.equal(mp1, mp3))
    if n_eps > 7:   # offset_eps + 1: the same stream, one group of four later
        assert torch.equal(e3[:n_eps - 4], e1[4:])
    lib, ptr, sp = fl.L.lib(), fl.L.ptr, fl.L.stream_ptr
    mbuf, mp_nm = _guarded(B, d)
    xbuf, xin_nm = _guarded(2, B * d)
    x, m = _dev(inp["x"]), _dev(inp["m"])
    assert lib.vpc_nm_prep(ptr(x), ptr(m), ptr(mp_nm), ptr(xin_nm), B, d, 0.6, None, 0, 7, 11, 0,
                           None, 0, 0, 0, 0, 0, sp()) == 0
    ebuf, e_fn = _guarded(n_eps)
    assert lib.vpc_fill_normal(ptr(e_fn), n_eps, 7, 1 << 40, None, 0, 0, 0, 4, sp()) == 0
    torch.cuda.synchronize()
    assert _margin_intact(mbuf, xbuf, ebuf)
    assert torch.equal(mp_nm.cpu(), mp1) and torch.equal(e_fn.cpu(), e1)
    if B * d >= 64:
        assert 0.3 < mp1.sum().item() / inp["m"].sum() < 0.9   # keep_prob 0.6 of the observed entries
