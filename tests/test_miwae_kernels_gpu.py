"""The MIWAE kernels (csrc/vpc_miw.hip) and MIWTrainer against float64 at their edges, per kernel and per head block:
  1. miw_sample / miw_sample_bwd / miw_heads / miw_heads_bwd against tests/miwae_oracle.py in float64, bounded by 8 x the
     error the same expression has in fp32 torch on the CPU (floor 2^-21 of the block's max), optional pointers given and
     None, the softplus threshold planted, a sentinel margin behind every output;
  2. vpc_miw_loss on tests/miwae_cases.LOSS_GRID, reg / vanilla, both pairings, raw and activated heads, a narrow and a
     wide head distribution: all of out8, loss_f32, accum, every decoder-head gradient block and encoder-head block on its
     own max, the llh_eval imputation; padded pitches, masks at the ends, the argument guards;
  3. one MIWTrainer step and the API path against the oracle from the parameters (ReLU gates inside the kink band taken
     from the step, tests/miwae_oracle._mlp), and the trainer's workspace rule across a batch-size change;
  4. the per-row imputation at S = 700.
Tolerances are relative to the max of the compared tensor."""
import math

import numpy as np
import pytest
import torch

import miwae_cases as C
import miwae_oracle as O

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 1}
SENT = 12345.0   # fill of the margins, the pad columns of G and the out8 of the guard tests
MARGIN = 64
FLOOR = 2.0 ** -21
WORST = {}       # kernel -> largest kernel error / fp32-torch error seen in this session (printed)


@pytest.fixture(scope="module")
def mw():
    import vpc_amd
    from vpc_amd import miwae
    return miwae


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _t64(a):
    return None if a is None else torch.from_numpy(a).double()


def _t32(a):
    return None if a is None else torch.from_numpy(a)


def _close(got, ref, tol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = float((got - ref).abs().max() / (ref.abs().max() + 1e-30))
    assert err <= tol, (what, err)


def _guarded(*shape):
    """An output of `shape` with MARGIN sentinel floats behind it: (whole buffer, the output view)."""
    n = math.prod(shape)
    buf = torch.full((n + MARGIN,), SENT, device="cuda")
    return buf, buf[:n].view(*shape)


def _margin_intact(buf):
    return bool((buf[-MARGIN:] == SENT).all())


def _bounded(kernel, what, got, ref64, ref32, blocks):
    """Per column block: the kernel's error against float64 is at most 8 x that of fp32 torch on the CPU."""
    got, ref32 = got.detach().double().cpu().reshape(ref64.shape), ref32.double()
    for name, sl in blocks:
        g, r, f = got[..., sl], ref64[..., sl], ref32[..., sl]
        mx = float(r.abs().max())
        ek, e32 = float((g - r).abs().max()), float((f - r).abs().max())
        bound = max(8.0 * e32, FLOOR * mx)
        ratio = ek / e32 if e32 > 0 else (0.0 if ek == 0 else float("inf"))
        if math.isfinite(ratio):
            WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
        print(f"{kernel} {what} {name}: kernel {ek:.3e} fp32 torch {e32:.3e} (ratio {ratio:.2f}, largest so far "
              f"{WORST.get(kernel, 0.0):.2f}) block max {mx:.3e} bound {bound:.3e}")
        assert ek <= bound, (kernel, what, name, ek, e32, mx)


# ------------------------------------------------------------------------------------------------ 1. elementwise kernels
@pytest.mark.parametrize("shape", C.SAMPLE_SHAPES)
@pytest.mark.parametrize("with_hact", [True, False])
@pytest.mark.parametrize("with_eps", [True, False])
def test_sample_vs_float64(mw, shape, with_eps, with_hact):
    R, S, Ld = shape
    i = C.sample_inputs(*shape)
    eps = i["eps"] if with_eps else None
    zbuf, z = _guarded(R * S, Ld)
    hbuf, hact = _guarded(R, 2 * Ld)
    mw.miw_sample(_dev(i["heads"]), hact if with_hact else None, _dev(eps), z, R, S, Ld)
    z64, h64 = O.sample(_t64(i["heads"]), _t64(eps), S)
    z32, h32 = O.sample(_t32(i["heads"]), _t32(eps), S)
    _bounded("miw_sample", (shape, with_eps, with_hact), z, z64, z32, [("z", slice(None))])
    if not with_eps:  # sample = False: z is the mean, bit for bit
        assert torch.equal(z.cpu().view(R, S, Ld), torch.from_numpy(i["heads"][:, None, :Ld]).expand(R, S, Ld))
    if with_hact:
        _bounded("miw_sample", (shape, with_eps, with_hact), hact, h64, h32,
                 [("hact mean", slice(0, Ld)), ("hact scale", slice(Ld, None))])
        assert torch.equal(hact[:, :Ld].cpu(), torch.from_numpy(i["heads"][:, :Ld]))
    else:
        assert bool((hbuf == SENT).all())
    assert _margin_intact(zbuf) and _margin_intact(hbuf)


@pytest.mark.parametrize("shape", C.SAMPLE_SHAPES)
@pytest.mark.parametrize("given", ["dz+eps+g", "dz+eps", "g", "dz+g", "none"])
def test_sample_bwd_vs_float64(mw, shape, given):
    """dz = None leaves the g_hact term, g_hact = None the dz term; eps = None (z was the mean) leaves no dz term in the
    scale half."""
    R, S, Ld = shape
    i = C.sample_inputs(*shape)
    dz = i["dz"] if "dz" in given else None
    eps = i["eps"] if "eps" in given else None
    g = i["g_hact"] if "g" in given.split("+") else None
    obuf, out = _guarded(R, 2 * Ld)
    mw.miw_sample_bwd(_dev(dz), _dev(eps), _dev(i["heads"]), _dev(g), out, R, S, Ld)
    r = lambda a: None if a is None else a.reshape(R, S, Ld)
    ref64 = O.sample_bwd(r(_t64(dz)), r(_t64(eps)), _t64(i["heads"]), _t64(g), S)
    ref32 = O.sample_bwd(r(_t32(dz)), r(_t32(eps)), _t32(i["heads"]), _t32(g), S)
    _bounded("miw_sample_bwd", (shape, given), out, ref64, ref32, [("d mean", slice(0, Ld)), ("d raw scale", slice(Ld, None))])
    assert _margin_intact(obuf)


def _head_blocks(d):
    return [("mean", slice(0, d)), ("scale", slice(d, 2 * d)), ("df", slice(2 * d, None))]


@pytest.mark.parametrize("shape", C.HEADS_SHAPES)
def test_heads_vs_float64(mw, shape):
    M, d = shape
    i = C.heads_inputs(*shape)
    obuf, out = _guarded(M, 3 * d)
    mw.miw_heads(_dev(i["y"]), out, M, d)
    _bounded("miw_heads", shape, out, O.heads_act(_t64(i["y"])), O.heads_act(_t32(i["y"])), _head_blocks(d))
    assert _margin_intact(obuf)


@pytest.mark.parametrize("shape", C.HEADS_SHAPES)
def test_heads_bwd_vs_float64(mw, shape):
    M, d = shape
    i = C.heads_inputs(*shape)
    obuf, out = _guarded(M, 3 * d)
    mw.miw_heads_bwd(_dev(i["y"]), _dev(i["g"]), out, M, d)
    _bounded("miw_heads_bwd", shape, out, O.heads_bwd(_t64(i["y"]), _t64(i["g"])),
             O.heads_bwd(_t32(i["y"]), _t32(i["g"])), _head_blocks(d))
    assert _margin_intact(obuf)


# ------------------------------------------------------------------------------------------------ 2. vpc_miw_loss
def _heads_in(o, d, raw):
    return o[0] if raw else C.act_f32(o[0], d)


def _oracle_loss(inp, dims, reg, pairing, raw, alpha):
    """float64: out8, per pass (d heads [N, 3d], d mean, d scale) by autograd, the llh_eval imputation.  The leaves are
    the fp32 arrays the kernel is given."""
    B, S, d, Ld = dims
    x, m, mp, oq, op, e = inp
    leaves = []

    def pas(o):
        Y = torch.from_numpy(_heads_in(o, d, raw)).double().requires_grad_()
        Ya = O.heads_act(Y) if raw else Y
        mean, scale = _t64(o[1]).requires_grad_(), _t64(o[2]).requires_grad_()
        leaves.append((Y, mean, scale))
        return tuple(Ya[:, k * d:(k + 1) * d].reshape(B, S, d) for k in range(3)), mean, scale

    q = pas(oq)
    p = pas(op) if reg else None
    mpt = torch.from_numpy(mp) if reg else None
    eps2 = [torch.from_numpy(e[0]), torch.from_numpy(e[1])]
    t = O.terms(torch.from_numpy(x), torch.from_numpy(m), mpt, q, p, eps2, alpha, pairing)
    t[0].backward()
    with torch.no_grad():
        a_q = O.slot_matrix(torch.from_numpy(x), torch.from_numpy(m), q[0], q[1], q[2], eps2[0], pairing)
        imp = O.impute(a_q, q[0][0])
    return dict(out8=t.detach(), grads=[(Y.grad, mean.grad, scale.grad) for Y, mean, scale in leaves], imp=imp)


def _run_loss(mw, inp, dims, reg, pairing, raw, alpha, grads=True, impute=True, ldy=None, ldg=None, accum=None):
    """vpc_miw_loss on the device.  ldy / ldg past 3d: the pad columns of Y hold NaN, those of G the sentinel."""
    B, S, d, Ld = dims
    N = B * S
    x, m, mp, oq, op, e = inp
    pid = mw.PAIR_REFERENCE if pairing == "reference" else mw.PAIR_PER_ROW
    ldy, ldg = ldy or 3 * d, ldg or 3 * d
    P = 2 if reg else 1

    def head_buf(o):
        Y = torch.full((N, ldy), float("nan"), device="cuda")
        Y[:, :3 * d] = _dev(_heads_in(o, d, raw))
        return Y

    Y = [head_buf(o) for o in (oq, op)[:P]] + [None]
    h = [_dev(np.concatenate([o[1], o[2]], 1)) for o in (oq, op)[:P]] + [None]
    G = [torch.full((N, ldg), SENT, device="cuda") if grads else None for _ in range(P)] + [None]
    gh = [torch.empty(B, 2 * Ld, device="cuda") if grads else None for _ in range(P)] + [None]
    imp = torch.empty(B, d, device="cuda") if impute else None
    out8 = torch.empty(8, dtype=torch.float64, device="cuda")
    lf = torch.empty(1, device="cuda")
    ed = _dev(e)
    mw.miw_loss(_dev(x), _dev(m), _dev(mp) if reg else None, Y[0], Y[1], ldy, raw, h[0], h[1], ed[0],
                ed[1] if reg else None, G[0], G[1], ldg, gh[0], gh[1], imp, mw.miw_loss_scratch(B, S, "cuda"), out8, lf,
                accum, B, S, d, Ld, alpha, pid)
    return dict(out8=out8.cpu(), G=G[:P], gh=gh[:P], imp=imp, loss_f32=lf.cpu())


def _term_tol(ref, ref0):
    """2e-5 of the term's own magnitude; of |loss| where the term is (about) empty, e.g. reg_like with mask_p == mask."""
    return 2e-5 * (abs(ref) if abs(ref) >= 1e-3 else abs(ref0))


def _check_loss(got, ora, dims, what, grads=True):
    B, S, d, Ld = dims
    o8, r8 = got["out8"], ora["out8"]
    ref0 = r8[0].item()
    print(f"{what}: out8 {o8.tolist()} oracle {r8.tolist()}")
    assert abs(o8[0].item() - ref0) <= 2e-5 * abs(ref0), (what, o8[0].item(), ref0)
    for k in (1, 2, 3, 4, 6, 7):
        assert abs(o8[k].item() - r8[k].item()) <= _term_tol(r8[k].item(), ref0), (what, k, o8[k].item(), r8[k].item())
    # out8[5] = sum(lpm) / (B * 5000): the same fp32 row sums and double reduction as reg_like (out8[4]), so the same rule
    # on the per-row mean sum(lpm) / B, i.e. before the literal 5000 makes the number small
    assert abs(o8[5].item() - r8[5].item()) * 5000 <= _term_tol(r8[5].item() * 5000, ref0), (what, 5, o8[5].item(), r8[5].item())
    assert got["loss_f32"].item() == float(np.float32(o8[0].item())), what
    if grads:
        for k, (gY, gm, gs) in enumerate(ora["grads"]):
            G = got["G"][k][:, :3 * d]
            for name, sl in _head_blocks(d):
                _close(G[:, sl], gY[:, sl], 5e-5, (what, "pass", k, "d", name))
            _close(got["gh"][k][:, :Ld], gm, 5e-5, (what, "pass", k, "d enc mean"))
            _close(got["gh"][k][:, Ld:], gs, 5e-5, (what, "pass", k, "d enc scale"))
    if got["imp"] is not None:
        _close(got["imp"], ora["imp"], 2e-5, (what, "xm_imp"))


def _loss_case(mw, inp, dims, reg, pairing, alpha, what):
    """Both head forms of one case against the oracle: every output with gradients requested, the imputation and out8
    again without, accum over the two runs, and the raw pair against each other."""
    B, S, d, Ld = dims
    accum = torch.zeros(1, device="cuda")
    runs = {}
    for raw in (1, 0):
        ora = _oracle_loss(inp, dims, reg, pairing, raw, alpha)
        got = _run_loss(mw, inp, dims, reg, pairing, raw, alpha, accum=accum)
        _check_loss(got, ora, dims, (what, "raw", raw))
        nog = _run_loss(mw, inp, dims, reg, pairing, raw, alpha, grads=False)
        _check_loss(nog, ora, dims, (what, "raw", raw, "no gradients"), grads=False)
        assert torch.equal(nog["imp"], got["imp"]) and torch.equal(nog["out8"], got["out8"]), what
        runs[raw] = (got, ora)
    l1, l0 = runs[1][0]["loss_f32"], runs[0][0]["loss_f32"]
    assert accum.item() == (l1 + l0).item(), (what, accum.item(), l1.item(), l0.item())
    # the two head forms of the same draws.  raw = 0 is given fp32-rounded activations, so the pair differs by input
    # rounding even in exact arithmetic: each entry to 1e-6 of its own magnitude, the loss (a signed sum that cancels,
    # e.g. -0.064 from terms near 5 at (4, 130, 3, 2) wide) to 1e-6 of its largest term; never looser than 1e-6 of the
    # whole tensor's max
    a, b = runs[1][0]["out8"], runs[0][0]["out8"]
    ref0 = max(abs(b[k].item()) for k in range(5))
    for k in range(8):
        scale = 5000 if k == 5 else 1
        tol = 1e-6 * (abs(b[k].item()) * scale if k and abs(b[k].item()) * scale >= 1e-3 else ref0)
        assert abs(a[k].item() - b[k].item()) * scale <= tol, (what, "raw pair", k, a[k].item(), b[k].item())
    _close(a, b, 1e-6, (what, "raw pair"))  # the bound as stated for the whole tensor; the per-entry rule above is stricter
    return runs


@pytest.mark.parametrize("dist", ["narrow", "wide"])
@pytest.mark.parametrize("pairing", ["reference", "per_row"])
@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("dims", C.LOSS_GRID)
def test_loss_grid_vs_oracle(mw, dims, kind, pairing, dist):
    inp = C.rand_inputs(*dims, seed=100 + C.LOSS_GRID.index(dims), dist=dist)
    _loss_case(mw, inp, dims, kind == "reg", pairing, C.ALPHA, (dims, kind, pairing, dist))


@pytest.mark.parametrize("pairing", ["reference", "per_row"])
@pytest.mark.parametrize("raw", [0, 1])
@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("dims", C.PITCH_CASES)
def test_loss_padded_pitch_is_bit_equal(mw, dims, kind, raw, pairing):
    """ldy = 3d + 5 (NaN in the pad columns of Y) and ldg = 3d + 3: every result bit-equal to the dense run, the pad
    columns of G untouched."""
    B, S, d, Ld = dims
    inp = C.rand_inputs(*dims, seed=200 + C.PITCH_CASES.index(dims), dist="wide")
    reg = kind == "reg"
    dense = _run_loss(mw, inp, dims, reg, pairing, raw, C.ALPHA)
    pad = _run_loss(mw, inp, dims, reg, pairing, raw, C.ALPHA, ldy=3 * d + 5, ldg=3 * d + 3)
    assert torch.equal(pad["out8"], dense["out8"]) and torch.equal(pad["loss_f32"], dense["loss_f32"])
    assert not bool(torch.isnan(pad["out8"]).any())
    assert torch.equal(pad["imp"], dense["imp"])
    for k in range(2 if reg else 1):
        assert torch.equal(pad["G"][k][:, :3 * d], dense["G"][k]), k
        assert bool((pad["G"][k][:, 3 * d:] == SENT).all()), k
        assert not bool((dense["G"][k] == SENT).any()), k
        assert torch.equal(pad["gh"][k], dense["gh"][k]), k


@pytest.mark.parametrize("pairing", ["reference", "per_row"])
@pytest.mark.parametrize("case", ["all_ones", "empty_mask_row", "empty_mask_p_row"])
def test_loss_masks_at_the_ends(mw, case, pairing):
    dims = (6, 9, 12, 4)
    x, m, mp, oq, op, e = C.rand_inputs(*dims, seed=300)
    m, mp = m.copy(), mp.copy()
    if case == "all_ones":            # mask_p == mask: reg_like is 0 and the `g -= ..` term of the q pass vanishes
        m[:] = 1.0
        mp[:] = 1.0
    elif case == "empty_mask_row":    # likelihood sum 0, the row still takes part in the log-sum-exp
        m[2] = 0.0
        mp[2] = 0.0
    else:
        mp[1] = 0.0
    for reg in (True, False):
        if not reg and case == "empty_mask_p_row":
            continue
        runs = _loss_case(mw, (x, m, mp, oq, op, e), dims, reg, pairing, C.ALPHA, (case, reg, pairing))
        if case == "all_ones":
            for raw in (0, 1):
                assert runs[raw][0]["out8"][4].item() == 0.0 and runs[raw][0]["out8"][5].item() == 0.0


@pytest.mark.parametrize("guard", ["ldy", "ldg", "scratch_short", "scratch_misaligned", "pairing", "no_y_p"])
def test_loss_guards(mw, guard):
    """Each bad argument raises before any launch: out8 keeps its fill."""
    dims = B, S, d, Ld = 3, 5, 12, 4
    x, m, mp, oq, op, e = C.rand_inputs(*dims, seed=400)
    N = B * S
    Yq, Yp = _dev(oq[0]), _dev(op[0])
    hq, hp = _dev(np.concatenate([oq[1], oq[2]], 1)), _dev(np.concatenate([op[1], op[2]], 1))
    Gq, Gp = torch.empty(N, 3 * d, device="cuda"), torch.empty(N, 3 * d, device="cuda")
    ghq, ghp = torch.empty(B, 2 * Ld, device="cuda"), torch.empty(B, 2 * Ld, device="cuda")
    ed = _dev(e)
    sc = mw.miw_loss_scratch(B, S, "cuda")
    nbytes = sc.numel() * sc.element_size()
    out8 = torch.full((8,), SENT, dtype=torch.float64, device="cuda")
    kw = dict(ldy=3 * d, ldg=3 * d, scratch=sc, pairing=mw.PAIR_REFERENCE, y_p=Yp)
    if guard == "ldy":
        kw["ldy"] = 3 * d - 1
    elif guard == "ldg":
        kw["ldg"] = 3 * d - 1
    elif guard == "scratch_short":
        kw["scratch"] = sc.view(torch.uint8)[:nbytes - 1]
    elif guard == "scratch_misaligned":
        kw["scratch"] = torch.empty(nbytes + 8, dtype=torch.uint8, device="cuda")[4:4 + nbytes]
        assert kw["scratch"].data_ptr() % 8 == 4
    elif guard == "pairing":
        kw["pairing"] = 2
    else:
        kw["y_p"] = None
    with pytest.raises(mw.L.VpcError):
        mw.miw_loss(_dev(x), _dev(m), _dev(mp), Yq, kw["y_p"], kw["ldy"], 1, hq, hp, ed[0], ed[1], Gq, Gp, kw["ldg"], ghq,
                    ghp, None, kw["scratch"], out8, None, None, B, S, d, Ld, C.ALPHA, kw["pairing"])
    torch.cuda.synchronize()
    assert bool((out8 == SENT).all())


# ------------------------------------------------------------------------------------------------ 3. trainer and API path
def _model(mw, c):
    cls = mw.Reg_MIWAE if c["reg"] else mw.MIWAE
    model = cls(c["d"], 500, 10, c["L"], TP, c["S"], 1)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c["params"].items()})
    return model.cuda()


def _step_gates(tr, c):
    """The ReLU gates the step took, per pass and chain, keyed as tests/miwae_oracle.run takes them."""
    B, BS = c["B"], c["B"] * c["S"]
    g = lambda a, b, r: {0: (a[r] > 0).cpu(), 2: (b[r] > 0).cpu()}
    gates = {"enc_q": g(tr.h1, tr.h2, slice(0, B)), "dec_q": g(tr.g1, tr.g2, slice(0, BS))}
    if c["reg"]:
        gates.update({"enc_p": g(tr.h1, tr.h2, slice(B, None)), "dec_p": g(tr.g1, tr.g2, slice(BS, None))})
    return gates


@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("shape", list(C.TRAINER_CASES))
def test_trainer_step_and_api_vs_oracle(mw, shape, kind):
    """One MIWTrainer.step and the API path (forward, loss, backward) on the same parameters and draws: loss 1e-4, each of
    the twelve gradients 2e-4 of its max against float64 autograd, the two device paths 2e-5 of the flat gradient's max.
    fp32 and float64 may gate a hidden unit whose pre-activation is within rounding of 0 differently, and one such unit
    moves a weight-gradient row by a whole batch row's term: the oracle takes the step's own gate for the units within
    O.KINK_BAND of their layer's max |pre-activation| and its own everywhere else (as tests/test_eddi_mnist_gpu.py)."""
    c = C.trainer_case(shape, kind)
    x, m, mp, eps = _dev(c["x"]), _dev(c["mask"]), _dev(c["mask_p"]), _dev(c["eps"])
    model = _model(mw, c)
    tl, _ = C.api_loss(model, x, m, mp, eps, C.ALPHA)
    tl.backward()
    api_loss = tl.item()
    api_grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    tr = mw.MIWTrainer(model, lr=1e-3)
    tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    p, xo, mo, mpo, epo = C.oracle_inputs(c)
    stats = O.new_gate_stats()
    lo = O.run(p, xo, mo, mpo, epo, C.ALPHA, gates=_step_gates(tr, c), stats=stats)[0]
    ref = dict(zip(O.KEYS, torch.autograd.grad(lo, [p[k] for k in O.KEYS])))
    print(f"{shape} {kind}: {stats['in_band']} of {stats['units']} units inside the kink band, "
          f"{stats['taken_from_device']} gated as the step did, {stats['mismatch_outside']} gate mismatches outside it")
    assert stats["in_band"] <= C.band_limit(stats["units"])
    assert stats["mismatch_outside"] == 0
    assert abs(tr.loss_value() - lo.item()) <= 1e-4 * abs(lo.item()), (tr.loss_value(), lo.item())
    assert abs(api_loss - lo.item()) <= 1e-4 * abs(lo.item()), (api_loss, lo.item())
    assert list(api_grads) == O.KEYS
    for k, prm in model.named_parameters():  # MIWTrainer rebound every .grad to its view of tr.grad: the step's gradient
        assert prm.grad.data_ptr() >= tr.grad.data_ptr() and prm.grad.data_ptr() != api_grads[k].data_ptr()
        _close(prm.grad, ref[k], 2e-4, ("trainer", k))
        _close(api_grads[k], ref[k], 2e-4, ("api", k))
    _close(tr.grad, torch.cat([api_grads[k].reshape(-1) for k in O.KEYS]), 2e-5, "trainer vs api")


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_trainer_workspace_across_batch_sizes(mw, kind):
    """Two steps at B = 37, then one at B = 5 on the same trainer (the workspaces and the Y[BS:] / G[BS:] / hact[B:]
    slices are re-made): bit-equal to a fresh trainer stepped from the same parameters and Adam state."""
    big = C.model_case(37, 5, 70, 10, kind == "reg", 12)
    small = C.model_case(5, 5, 70, 10, kind == "reg", 13)
    dv = lambda c: (_dev(c["x"]), _dev(c["mask"]), _dev(c["mask_p"]), _dev(c["eps"]))
    model = _model(mw, big)
    tr = mw.MIWTrainer(model, lr=1e-3)
    x, m, mp, eps = dv(big)
    tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    tr.step(x, m, mask_p=mp, eps=eps.flip(2), alpha=C.ALPHA)
    fresh = _model(mw, big)
    fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
    tr2 = mw.MIWTrainer(fresh, lr=1e-3)
    tr2.exp_avg.copy_(tr.exp_avg)
    tr2.exp_avg_sq.copy_(tr.exp_avg_sq)
    tr2.step_count, tr2.rng_offset = tr.step_count, tr.rng_offset
    x, m, mp, eps = dv(small)
    tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    tr2.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    assert tr.loss_value() == tr2.loss_value() and math.isfinite(tr.loss_value())
    assert torch.equal(tr.grad, tr2.grad)
    assert torch.equal(model._flat, fresh._flat)
    assert torch.equal(tr.exp_avg, tr2.exp_avg) and torch.equal(tr.exp_avg_sq, tr2.exp_avg_sq)


# ------------------------------------------------------------------------------------------------ 4. large-S imputation
@pytest.mark.parametrize("kind", ["reg", "van"])
def test_per_row_imputation_at_large_S(mw, kind):
    """model._loss(llh_eval, PAIR_PER_ROW) at S = 700: eleven trips of the wave-stride loops and the serial S loop of the
    imputation, as eval_miwae runs them with valid_k draws."""
    B, S, d, Ld = 5, 700, 12, 10
    reg = kind == "reg"
    c = C.model_case(B, S, d, Ld, reg, 21)
    x, m, mp, eps = _dev(c["x"]), _dev(c["mask"]), _dev(c["mask_p"]), _dev(c["eps"])
    model = _model(mw, c)
    with torch.no_grad():
        z, mean, scale = model._encode(x, m, eps=eps[0], S=S)
        outs_q = (*model.decoder(z), mean, scale)
        outs_p = None
        if reg:
            z, mean, scale = model._encode(x, mp, eps=eps[1], S=S)
            outs_p = (*model.decoder(z), mean, scale)
        loss, out8, xm = model._loss(x, m, mp, outs_q, outs_p, 0.5, list(eps[2:] if reg else eps[1:]), True,
                                     pairing=mw.PAIR_PER_ROW, S=S)
        p, xo, mo, mpo, epo = C.oracle_inputs(c)
        lo, a_q, q, _ = O.run(p, xo, mo, mpo, epo, 0.5, "per_row")
        ref = O.impute(a_q, q[0][0])
    assert xm.shape == (B, d)
    assert abs(loss.item() - lo.item()) <= 1e-4 * abs(lo.item()), (loss.item(), lo.item())
    _close(xm, ref, 2e-5, "xm_imp")
