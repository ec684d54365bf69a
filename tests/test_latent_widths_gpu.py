"""The dense VAE family at every latent width it accepts (MI355X).  The rest of the GPU suite runs the register-chained kernels
at L = 10 only; the cases, their boundaries and the tolerances are in tests/latent_cases.py, their soundness (float32 port
against the float64 closed form on these very inputs) in tests/test_latent_widths_cpu.py.

One group per path: 1 raw forward kernels on dense [B][L] tensors, 2 API path backward, 3 FusedTrainer fp32 in every workgroup
shape (+ two Adam steps), 4 bf16 / bf16x3 against the fp32 path, 5 mask-augmented classes, 6 in-kernel draws, 7 evaluation,
8 reward and acquisition, 9 EnsembleTrainer, 10 EDDITrainer, 11 the wide path at L = 16, 33, 64.

No case skips: where a path is expected, the test asserts that the library took it."""
import copy

import numpy as np
import pytest
import torch

import latent_cases as lc
import vpc_amd as vpc
from latent_cases import rel
from oracle import eddi_oracle as EO
from oracle import vae_oracle as O
from vpc_amd import active as A
from vpc_amd import ensemble as E
from vpc_amd import harness as H
from vpc_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TP = lc.TP
ENV_SWITCHES = ("VPC_TILE", "VPC_DEC8", "VPC_STEP_SMALL", "VPC_DRAW_FUSED", "VPC_STEP_FUSED")


def ids(cases):
    return [lc.case_id(c) for c in cases]


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    """Every test starts from the library's own choices; a test sets the switches of the path it is about."""
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)


def set_env(monkeypatch, env):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def dev(*ts):
    return [t.to(DEV) for t in ts]


def cls_of(kind):
    return vpc.vanilla_VAE if kind == "vanilla" else vpc.Reg_VAE


def fused_step(tr, kind, data, **kw):
    """kind: "vanilla", or a two-pass one ("reg" = "kl_reg", "ml_reg": the third eps plane is injected too)."""
    x, mask, mask_p, eq, ep, eml = dev(*data)
    if kind == "vanilla":
        tr.step(x, mask, eps_q=eq, **kw)
    else:
        tr.step(x, mask, mask_p, eq, ep, eml if kind == "ml_reg" else None, **kw)


# ------------------------------------------------------------------------------------------ 1. raw forward kernels
@pytest.mark.parametrize("L,d,B", lc.FORWARD_CASES, ids=ids(lc.FORWARD_CASES))
def test_raw_forward_kernels_dense_latents(L, d, B):
    """vpc_encoder_fwd / vpc_decoder_fwd on dense [B][L] mean / logvar / z (row pitch L: odd L gives rows that are only 4-byte
    aligned), every output filled with NaN first and the latent outputs followed by one guard row."""
    from vpc_amd._lib import HIDDEN_POS1 as P1, HIDDEN_POS2 as P2
    seed = lc.case_seed(L, d, B)
    params = O.init_params(d, L, seed=seed)
    x, mask, _, eq, _, _ = lc.synth(B, d, L, seed=seed + 1)
    port = O.TorchPort(params, L)
    z_ref, mean_ref, lv_ref = port.encoder(x, mask, eq)
    xh_ref, _ = port.decoder(z_ref)
    c = O.closed_form_pass(O._np(params), x.numpy().astype(np.float64), mask.numpy().astype(np.float64),
                           eq.numpy().astype(np.float64), L)
    m = lc.make_model(vpc.Reg_VAE, d, L, params)
    xd, md, ed = x.to(DEV), ops.as_mask_u8(mask.to(DEV)), eq.to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    h1, h2 = nan(B, 112), nan(B, 64)
    mean_g, lv_g, z_g, xh_g = nan(B + 1, L), nan(B + 1, L), nan(B + 1, L), nan(B + 1, d)
    mean, lv, z, xh = mean_g[:B], lv_g[:B], z_g[:B], xh_g[:B]
    ops.encoder_fwd(xd, m._enc_img(), [md], [ed], [h1], [h2], [mean], [lv], [z], d, L)
    ops.decoder_fwd(z, m._dec_img(), xh, d, L)
    for name, got, ref32, ref64, tol in (("mean", mean, mean_ref, c.mean, lc.FWD_ATOL), ("logvar", lv, lv_ref, c.logvar, lc.FWD_ATOL),
                                         ("z", z, z_ref, c.z, lc.Z_ATOL), ("xhat", xh, xh_ref, c.xhat, lc.FWD_ATOL)):
        g = got.cpu()
        assert not torch.isnan(g).any(), name  # every entry of [B][L] (of [B][d]) was written
        e32, e64 = float((g - ref32).abs().max()), float(np.max(np.abs(g.numpy() - ref64)))
        lc.record("1_forward", name, max(e32, e64), tol)
        assert e32 <= tol and e64 <= tol, (name, e32, e64)
    for name, guard in (("mean", mean_g), ("logvar", lv_g), ("z", z_g), ("xhat", xh_g)):
        assert torch.isnan(guard[B]).all(), f"{name}: the row past B was written"
    # hidden activations: the units, the constant-1 units of the bias chain, exact zeros in the padding
    h1n, h2n = h1.cpu().numpy(), h2.cpu().numpy()
    assert not np.isnan(h1n).any() and not np.isnan(h2n).any()
    lc.record("1_forward", "h1", float(np.max(np.abs(h1n[:, P1[:100]] - c.h1))), lc.FWD_ATOL)
    lc.record("1_forward", "h2", float(np.max(np.abs(h2n[:, P2[:50]] - c.h2))), lc.FWD_ATOL)
    assert np.allclose(h1n[:, P1[:100]], c.h1, atol=lc.FWD_ATOL, rtol=0)
    assert np.all(h1n[:, P1[100]] == 1.0) and np.all(np.delete(h1n, P1, axis=1) == 0)
    assert np.allclose(h2n[:, P2[:50]], c.h2, atol=lc.FWD_ATOL, rtol=0) and np.all(h2n[:, P2[50]] == 1.0)
    # sample=False: z is the mean, bit for bit, and the guard row stays
    z2_g = nan(B + 1, L)
    ops.encoder_fwd(xd, m._enc_img(), [md], [None], [h1], [h2], [mean], [lv], [z2_g[:B]], d, L)
    assert torch.equal(z2_g[:B], mean) and torch.isnan(z2_g[B]).all()


# ------------------------------------------------------------------------------------------ 2. API path backward
class _Randn:
    """Stands in for torch.randn while model.forward / model.loss run: hands out the case's normals in the order the model
    draws them (eps_q, eps_p, the ml_reg sample) and insists on the shape [B][L]."""

    def __init__(self, draws):
        self.draws, self.taken = list(draws), 0

    def __call__(self, *shape, **kw):
        e = self.draws[self.taken]
        assert tuple(shape) == tuple(e.shape), (shape, tuple(e.shape))
        self.taken += 1
        return e


@pytest.mark.parametrize("L,d,B,form", lc.API_CASES, ids=ids(lc.API_CASES))
def test_api_forward_loss_backward(L, d, B, form, monkeypatch):
    """model.forward -> model.loss -> backward (RegEncoderFn / EncoderFn, DecoderFn, LossFn on dense [B][L] tensors) against
    torch_reg_step / torch_vanilla_step."""
    params, data, loss_ref, grads_ref, outs = lc.step_case(form, L, d, B)
    x, mask, mask_p, eq, ep, eml = dev(*data)
    kw = lc.STEP_KW[form]
    if form == "vanilla":
        m = lc.make_model(vpc.vanilla_VAE, d, L, params)
        mf = mask * torch.ones(x.shape, device=DEV)  # train.py:58,97: a float mask
        fake = _Randn([eq])
        with monkeypatch.context() as mp:
            mp.setattr(torch, "randn", fake)
            o = m.forward(x, mf)
            _, tl = m.loss(x, o[2], o[3], o[0], o[1], 1, mf, **kw)
        fwd = (o[0], o[1], o[2])
    else:
        m = lc.make_model(vpc.Reg_VAE, d, L, params, reg_type=form)
        fake = _Randn([eq, ep] + ([eml] if form == "ml_reg" else []))
        kw = dict(kw)
        with monkeypatch.context() as mp:
            mp.setattr(torch, "randn", fake)
            o = m.forward(x, mask, mask_p, "train")
            _, tl = m.loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mask, mask_p, kw.pop("epoch", 1), **kw)
        fwd = (o[0], o[1], o[2], o[4], o[5], o[6])
    assert fake.taken == len(fake.draws)
    want = [outs[i] for i in ((0, 1, 2) if form == "vanilla" else (0, 1, 2, 4, 5, 6))]
    for got, ref in zip(fwd, want):
        assert got.shape == ref.shape
        e = float((got.detach().cpu() - ref).abs().max())
        lc.record("2_api", "forward", e, lc.FWD_ATOL)
        assert e <= lc.FWD_ATOL
    tl.backward()
    lc.check_loss_grads("2_api", tl.item(), lc.flat_grads(m), m, loss_ref, grads_ref, (L, d, B, form))


# ------------------------------------------------------------------------------------------ 3. FusedTrainer fp32
@pytest.mark.parametrize("L,d,B,form,kind", lc.STEP_CASES, ids=ids(lc.STEP_CASES))
def test_fused_step_every_workgroup_shape(L, d, B, form, kind, monkeypatch):
    """tr.step(..., update=False) against the port, as test_gpu_parity.test_fused_step_ragged_shapes_vs_oracle, in every
    workgroup shape (latent_cases.STEP_ENV) and for kl_reg, ml_reg and vanilla_VAE."""
    set_env(monkeypatch, lc.STEP_ENV[form])
    params, data, loss_ref, grads_ref, _ = lc.step_case(kind, L, d, B)
    m = lc.make_model(cls_of(kind), d, L, params, reg_type=kind)
    tr = vpc.FusedTrainer(m)
    fused_step(tr, kind, data, update=False, **lc.STEP_KW[kind])
    if kind == "ml_reg":
        assert tr.coefficients(1400, 0.8, 0.9, False).ml_on
    assert tr.dominant_launch() == ("step_small" if form == "nsplit" else "decoder_fused")
    if form != "nsplit":
        # the row-tiled kernels hand the latent statistics and their seeds over in [B][16] workspaces whose features >= L are
        # exact zeros (vpc_enc_fwd_body.h; st_lat of both decoder kernels).  Loss and gradients cannot see a seed in column L:
        # the rows >= L of the packed W3 image are zero and their wgrad rows are not gathered.
        for name in ("mean", "logvar", "dmean", "dlogvar"):
            for p, t in enumerate(getattr(tr, name)):
                assert tuple(t.shape) == (B, 16) and bool(torch.isfinite(t[:, :L]).all()), (name, p)
                assert not bool(t[:, L:].any()), (name, p, "a column >= L is not zero")
    lc.check_loss_grads("3_step_" + form, tr.loss_value(), tr.grad.cpu().numpy(), m, loss_ref, grads_ref, (L, d, B, form, kind))


@pytest.mark.parametrize("L,kind", lc.ADAM_CASES, ids=ids(lc.ADAM_CASES))
def test_fused_two_adam_steps(L, kind):
    """update=True twice against the oracle's TorchTrainer (stock optim.Adam): the second step reads the weight images that
    the first step's Adam launch re-packed at this L.  Bounds of test_fused_adam_trajectory_matches_golden."""
    d, B = lc.ADAM_SHAPE
    form = lc.kind_form(kind)
    params, _, _, _, _ = lc.step_case(form, L, d, B)
    steps = [lc.synth(B, d, L, seed=lc.case_seed(L, d, B) + 50 + i) for i in range(2)]
    ref = O.TorchTrainer(params, L, vanilla=kind == "vanilla")
    m = lc.make_model(cls_of(kind), d, L, params)
    tr = vpc.FusedTrainer(m, lr=1e-3)
    for i, data in enumerate(steps):
        x, mask, mask_p, eq, ep, _ = data
        want = ref.step(x, mask, mask_p, eq, ep, epoch=i + 1, **lc.STEP_KW[form])
        fused_step(tr, kind, data, epoch=i + 1, **lc.STEP_KW[form])
        e = abs(tr.loss_value() - want) / abs(want)
        lc.record("3_adam", "loss", e, lc.TRAJ_LOSS_RTOL)
        assert e <= lc.TRAJ_LOSS_RTOL, (i, tr.loss_value(), want)
    state = ref.state()
    for k, p in zip(O.PARAM_KEYS, m.trainable()):
        e = rel(p.detach().cpu().numpy(), state[k].numpy())
        lc.record("3_adam", "param", e, lc.TRAJ_PARAM_RTOL)
        assert e < lc.TRAJ_PARAM_RTOL, k
    # the API path reads the re-packed images
    with torch.no_grad():
        _, mean, _ = m.encoder(steps[0][0].to(DEV), steps[0][1].to(DEV), sample=False)
    _, mean_ref, _ = O.TorchPort(state, L).encoder(steps[0][0], steps[0][1], sample=False)
    assert torch.allclose(mean.cpu(), mean_ref, atol=1e-4)


# ------------------------------------------------------------------------------------------ 4. bf16 / bf16x3
@pytest.mark.parametrize("L,d,B,tile,prec", lc.BF16_CASES, ids=ids(lc.BF16_CASES))
def test_bf16_engines_vs_f32_path(L, d, B, tile, prec, monkeypatch):
    """test_bf16.test_ragged_and_full_size_vs_f32_path with the latent width passed in: the requested engine (VPC_STEP_SMALL=0)
    against the fp32 kernels on the same injected draws.  Plain bf16 in the 128-row shape is the whole-step kernel."""
    set_env(monkeypatch, {"VPC_STEP_SMALL": "0", "VPC_TILE": tile})
    seed = lc.case_seed(L, d, B)
    params = O.init_params(d, L, seed=seed)
    data = lc.synth(B, d, L, seed=seed + 1)
    res = {}
    for p in ("f32", prec):
        m = lc.make_model(vpc.Reg_VAE, d, L, params)
        tr = vpc.FusedTrainer(m, precision=p)
        fused_step(tr, "reg", data, alpha=0.8, beta=0.9, update=False)
        assert tr.dominant_launch() != "step_small"
        whole = p == "bf16" and tile == "128"
        assert tr._used_step_fused == whole
        if whole:
            assert ops.step_fused_applicable(B, d, L, 2)
        res[p] = (tr.loss_value(), tr.grad.cpu().numpy().copy())
    tl, tg = lc.BF16_TOL[prec]
    le, ge = abs(res[prec][0] - res["f32"][0]) / abs(res["f32"][0]), rel(res[prec][1], res["f32"][1])
    lc.record("4_" + prec, "loss", le, tl)
    lc.record("4_" + prec, "grad", ge, tg)
    assert np.isfinite(res[prec][1]).all()
    assert le <= tl, (res[prec][0], res["f32"][0])
    assert ge < tg


# ------------------------------------------------------------------------------------------ 5. mask-augmented classes
@pytest.mark.parametrize("L,d,kind,path", lc.AUGM_CASES, ids=ids(lc.AUGM_CASES))
def test_mask_augmented_step(L, d, kind, path, monkeypatch):
    """Reg_VAE_mask / vanilla_VAE_mask on the N-split kernel and on the row-tiled kernels against the port with
    mask_augm=True (tests/test_small_augm_gpu.py at L = 10)."""
    set_env(monkeypatch, {"VPC_STEP_SMALL": "0"} if path == "decoder_fused" else {})
    params, data, loss_ref, grads_ref, _ = lc.step_case(kind, L, d, lc.AUGM_B, True)
    m = lc.make_model(vpc.vanilla_VAE_mask if kind == "vanilla" else vpc.Reg_VAE_mask, d, L, params, reg_type=kind)
    tr = vpc.FusedTrainer(m)
    fused_step(tr, kind, data, update=False, **lc.STEP_KW[kind])
    assert tr.dominant_launch() == path
    lc.check_loss_grads("5_augm_" + path, tr.loss_value(), tr.grad.cpu().numpy(), m, loss_ref, grads_ref, (L, d, kind, path))


# ------------------------------------------------------------------------------------------ 6. in-kernel draws
class _Recorder:
    """Stands in for the loaded library: records every vpc_* symbol fetched, hands out the real one."""

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        if name.startswith("vpc_"):
            self.names.append(name)
        return getattr(self.real, name)


def _drawn_step(L, rt, fused, monkeypatch):
    """One step of a fresh trainer (seed 5) at the smallest batch at which FusedTrainer draws inside its kernels by itself
    (fused) or with the separate draw launch kept (VPC_DRAW_FUSED=0); the throughput shape in both."""
    from vpc_amd import _lib
    set_env(monkeypatch, {"VPC_TILE": "128"} if fused else {"VPC_TILE": "128", "VPC_DRAW_FUSED": "0"})
    d = lc.DRAW_D
    torch.manual_seed(0)
    m = vpc.Reg_VAE(d, 500, 10, L, TP, "exp", rt) if rt else vpc.vanilla_VAE(d, 500, 10, L, TP, "exp")
    tr = vpc.FusedTrainer(m.to(DEV), seed=5)
    B = tr._draw_fused_rows
    assert B > ops.step_small_max_rows()
    g = torch.Generator().manual_seed(B + d)
    x, mask = torch.rand(B, d, generator=g).to(DEV), (torch.rand(B, d, generator=g) < 0.7).to(DEV)
    rec = _Recorder(_lib.lib())
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "_lib", rec)
        tr.step(x, mask, alpha=0.8, beta=0.9)
    assert ("vpc_decoder_fused_draw_f32" in rec.names) == fused, rec.names
    assert ("vpc_encoder_fwd_draw_f32" in rec.names) == (fused and rt is not None), rec.names
    assert (("vpc_draw_step" if rt else "vpc_fill_normal") in rec.names) == (not fused), rec.names
    planes = 2 if rt else 1
    return {"mask_p": tr.mask_p_buf.clone(), "eps": tr.eps_buf[:planes].clone(), "out9": tr.out9.clone(), "grad": tr.grad.clone(),
            "flat": tr.model._flat.clone(), "exp_avg": tr.exp_avg.clone(), "exp_avg_sq": tr.exp_avg_sq.clone(),
            "rng_offset": tr.rng_offset}


@pytest.mark.parametrize("L,rt", lc.DRAW_CASES, ids=ids(lc.DRAW_CASES))
def test_inkernel_draws_equal_draw_step(L, rt, monkeypatch):
    """test_inkernel_draws.test_inkernel_draws_equal_draw_step at the batch the library's own threshold sets: everything a step
    leaves behind, bit for bit (L = 10 runs too: a failure is then seen to be one of a width)."""
    new, old = _drawn_step(L, rt, True, monkeypatch), _drawn_step(L, rt, False, monkeypatch)
    assert torch.isfinite(new["grad"]).all() and torch.isfinite(new["out9"]).all()
    for k in new:
        if k == "mask_p" and rt is None:
            continue
        a, b = new[k], old[k]
        if k == "rng_offset":
            assert a == b
        else:
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b), k


# ------------------------------------------------------------------------------------------ 7. evaluation
EVAL_N, EVAL_BS, EVAL_M, EVAL_G = 37, 16, 2, 3


def oracle_eval(params, L, x, mask, eps, N, batch_size, M, bw=1.0):
    """test_ensemble_eval_gpu.oracle_eval with the latent width passed in: float64 closed form per batch, the mean over the
    batches of a pass, the mean over the passes -> (rmse, elbo, negll, negll_imp)."""
    P = O._np(params)
    x, mk, eps = np.asarray(x, np.float64), np.asarray(mask, np.float64), np.asarray(eps, np.float64)
    s2, passes = np.exp(O.X_LOGVAR), []
    for p in range(M):
        rows = []
        for lo in range(0, N, batch_size):
            hi = min(lo + batch_size, N)
            xb, mb = x[lo:hi], mk[lo:hi]
            c = O.closed_form_pass(P, xb, mb, eps[p * N + lo:p * N + hi], L)
            t = 0.5 * O.X_LOGVAR + (xb - c.xhat) ** 2 / (2 * s2)
            const = O.HALF_LOG_2PI * xb.size
            negll, negll_imp = (np.sum(mb * t) + const) / (hi - lo), (np.sum((1 - mb) * t) + const) / (hi - lo)
            kl = np.sum(0.5 * (np.exp(c.logvar) + c.mean ** 2 - 1.0 - c.logvar))
            assert np.sum(1 - mb) > 0, "every batch needs an unobserved entry"
            rows.append((np.sqrt(np.sum((1 - mb) * (c.xhat - xb) ** 2) / np.sum(1 - mb)), negll + bw * kl / (hi - lo), negll, negll_imp))
        passes.append(np.mean(np.array(rows), 0))
    return np.mean(np.array(passes), 0)


def check_eval_numbers(group, got, want, llh_tol, rmse_tol, what):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    le, re_ = rel(got[1:], want[1:]), abs(got[0] - want[0]) / want[0]
    lc.record(group, "llh", le, llh_tol)
    lc.record(group, "rmse", re_, rmse_tol)
    assert want[0] >= 0.25, "the rmse bound was derived for rmse >= 0.25 (tests/test_ensemble_eval_gpu.py)"
    assert le < llh_tol and re_ <= rmse_tol, what


def _eval_data(L, d, G):
    g = torch.Generator().manual_seed(lc.case_seed(L, d, EVAL_N))
    x, mask = torch.rand(EVAL_N, d, generator=g), torch.rand(EVAL_N, d, generator=g) < 0.7
    eps = torch.randn(G, EVAL_M * EVAL_N, L, generator=g)
    return x, mask, eps


@pytest.mark.parametrize("L,d,kind", lc.EVAL_CASES, ids=ids(lc.EVAL_CASES))
def test_ensemble_evaluator_and_eval_sweep(L, d, kind):
    """EnsembleEvaluator for G = 3 (vpc_eval_small_multi_f32: the one-kernel evaluation of 16-row tiles): injected normals
    against the float64 closed form at the bounds of tests/test_ensemble_eval_gpu.py (2e-5 relative, rmse 1e-4); device draws
    against each member's stand-alone evaluation and against eval_sweep, bit for bit as there."""
    G, N, bs, M = EVAL_G, EVAL_N, EVAL_BS, EVAL_M
    cls = cls_of(kind)
    plist = [O.init_params(d, L, seed=lc.case_seed(L, d, N) + k) for k in range(G)]
    ms = [lc.make_model(cls, d, L, p) for p in plist]
    x, mask, eps = _eval_data(L, d, G)
    xd, md = x.to(DEV), mask.to(DEV)
    seeds = [3 + 5 * k for k in range(G)]
    ev = E.EnsembleEvaluator(ms, seeds=seeds)
    out = ev.evaluate(xd, md, bs, M, epoch=5, beta=0.7, eps=eps.to(DEV))
    assert out.shape == (G, 4)
    for k in range(G):
        want = oracle_eval(plist[k], L, x, mask, eps[k], N, bs, M, bw=0.7)
        check_eval_numbers("7_eval_ensemble", out[k].cpu().numpy(), want, 2e-5, 1e-4, (L, d, kind, k))
    drawn = ev.evaluate(xd, md, bs, M, epoch=5, beta=0.7)
    assert torch.isfinite(drawn).all() and len({tuple(r) for r in drawn.tolist()}) == G
    for k in range(G):
        alone = E.EnsembleEvaluator([lc.make_model(cls, d, L, plist[k])], seeds=[seeds[k]])
        assert torch.equal(alone.evaluate(xd, md, bs, M, epoch=5, beta=0.7)[0], drawn[k]), k
    # eval_sweep: one evaluate call over the batches of both passes, gathered behind each other
    vt = "reg_vae1" if kind == "reg" else "vanilla_vae1"
    cfgs = [dict(vae_type=vt, alpha=0.5, seed=seeds[k]) for k in range(G)]
    loader = [(x[lo:lo + bs], mask[lo:lo + bs]) for lo in range(0, N, bs)]
    sweep = H.eval_sweep([(loader, "test")], cfgs, 30, d, 500, 10, M, L, "uci", TP, "exp", 5, 1, 1, reg_type="kl_reg", beta=0.7,
                         models=ms, save=False)
    ranges = [[(p * N + lo, p * N + min(lo + bs, N)) for lo in range(0, N, bs)] for p in range(M)]
    direct = E.EnsembleEvaluator(ms, seeds=seeds).evaluate(torch.cat([xd] * M), torch.cat([md] * M), M=M, batches=ranges,
                                                           epoch=5, beta=0.7).cpu()
    for k in range(G):
        got = torch.stack([sweep[k]["test"][n] for n in ("rmse", "elbo", "negll", "negll_imp")])
        assert torch.equal(got, direct[k]), k
    assert torch.equal(direct, drawn.cpu())  # the same layout spelled as ranges: the same draws, the same bits


@pytest.mark.parametrize("L,d,kind", lc.EVAL_CASES, ids=ids(lc.EVAL_CASES))
def test_eval_vae_vs_closed_form(L, d, kind, tmp_path, monkeypatch):
    """harness.eval_vae (the API path at stage "evaluate") against the float64 closed form; the device normals are replayed
    under the same torch seed, as tests/test_gpu_parity.py::test_eval_vae_matches_oracle does, at its bound (3e-5 relative)."""
    monkeypatch.chdir(tmp_path)
    N, bs, M = EVAL_N, EVAL_BS, EVAL_M
    params = O.init_params(d, L, seed=lc.case_seed(L, d, N))
    x, mask, _ = _eval_data(L, d, 1)
    loader = [(x[lo:lo + bs], mask[lo:lo + bs]) for lo in range(0, N, bs)]
    m = lc.make_model(cls_of(kind), d, L, params)
    vt = "reg_vae1" if kind == "reg" else "vanilla_vae1"
    torch.manual_seed(77)
    out = vpc.eval_vae([(loader, "test")], 30, d, 500, 10, M, L, "synth", TP, "exp", vt, 100, 5, 1, device=torch.device(DEV),
                       alpha=1.0, stage="evaluate", p_missingness=30, reg_type="kl_reg", beta=1.0, model=m, save=False)["test"]
    torch.manual_seed(77)
    eps = []
    for _ in range(M):
        for xb, _mb in loader:
            eps.append(torch.randn(xb.shape[0], L, device=DEV).cpu())
            if kind == "reg":
                torch.randn(xb.shape[0], L, device=DEV)  # eps_p: drawn by forward(), unused at stage "evaluate"
    want = oracle_eval(params, L, x, mask, torch.cat(eps), N, bs, M, bw=1.0)
    got = [out[k].item() for k in ("rmse", "elbo", "negll", "negll_imp")]
    check_eval_numbers("7_eval_vae", got, want, 3e-5, 3e-5, (L, d, kind))


# ------------------------------------------------------------------------------------------ 8. reward and acquisition
def _reward_model(kind, d, L, seed):
    """(model on the GPU, the oracle's port of it).  Weights 2.5 x the default init, as test_gpu_reward_vs_oracle: larger
    rewards.  The point-net model takes 1.5 x: its front-end sums over the features, and at 2.5 x the float32 port's rewards at
    d = 100 reach the hundreds (1.5 x: 1e-4 .. 1e-2, still far above round-off)."""
    if kind == "eddi":
        torch.manual_seed(seed)
        m = vpc.Reg_EDDI(d, 500, 10, L, TP, "exp", "kl_reg")
        params = {k: v.detach().clone() * (1.5 if "weight" in k else 1.0) for k, v in m.state_dict().items() if "prior" not in k}
        m.load_state_dict({**m.state_dict(), **{k: v.clone() for k, v in params.items()}})
        return m.to(DEV), EO.EDDIPort(params, L)
    params = O.init_params(d, L, seed=seed, mask_augm=kind == "mask")
    params = {k: v * (2.5 if "weight" in k else 1.0) for k, v in params.items()}
    m = lc.make_model(vpc.Reg_VAE_mask if kind == "mask" else vpc.Reg_VAE, d, L, params)
    return m, O.TorchPort(params, L, mask_augm=kind == "mask")


def _reward_inputs(d, n, M, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, d, generator=g)
    mask = (torch.rand(n, d, generator=g) < 0.5).float()
    mask[:, -1] = (torch.rand(n, generator=g) < 0.3).float()
    return x, mask, torch.rand(M, n, d, generator=g)


@pytest.mark.parametrize("L,d,n,M,kind", lc.REWARD_CASES, ids=ids(lc.REWARD_CASES))
def test_reward_matrix_and_chains(L, d, n, M, kind):
    """vpc.reward_matrix of the plain, mask-augmented and point-net models (the mean | logvar head rows of the reward's chain
    kernel depend on L) against the oracle: the rule of test_gpu_reward_vs_oracle, the exact -1e4 pattern, the argmax; and
    chaini_I / chaini_II on the encoder kernels at 1e-6 absolute (tests/test_reward.py)."""
    seed = lc.case_seed(L, d, n)
    m, port = _reward_model(kind, d, L, seed)
    x, mask, im = _reward_inputs(d, n, M, seed + 1)
    with torch.no_grad():
        want = O.reward_matrix(port, x, mask, M, im).numpy()
    R = vpc.reward_matrix(m, x.to(DEV), mask.to(DEV), im.to(DEV)).cpu().numpy()
    assert np.array_equal(R == -1e4, want == -1e4)
    live = want != -1e4
    assert live.any() and np.isfinite(R).all()
    tol = 2e-6 + 1e-3 * np.max(np.abs(want[live]))
    err = float(np.max(np.abs(R[live] - want[live])))
    lc.record("8_reward_" + kind, "R", err, tol)
    assert err <= tol, (err, tol)
    top = np.argmax(want, 1)
    assert np.all(np.max(R, 1) - R[np.arange(n), top] <= tol)
    u = 3
    with torch.no_grad():
        k1, k2 = O.chaini_I(port, x, mask, u).numpy(), O.chaini_II(port, x, mask, u).numpy()
    g1 = vpc.chaini_I(x.to(DEV), mask.to(DEV), u, m).cpu().numpy()
    g2 = vpc.chaini_II(x.to(DEV), mask.to(DEV), u, m).cpu().numpy()
    e = float(max(np.max(np.abs(g1 - k1)), np.max(np.abs(g2 - k2))))
    lc.record("8_reward_" + kind, "chaini", e, 1e-6)
    assert g1.shape == (n,) and e <= 1e-6


def test_ensemble_acquirer_step_L15_bias_last_column():
    """One acquisition step of EnsembleAcquirer for G = 2 at L = 15: every member's rewards are its stand-alone
    reward_matrix on the imputations the step made (bit for bit, tests/test_ensemble_active_gpu.py), the action is the host's
    argmax, and the imputations are the oracle's decoder outputs."""
    L, G, d, n, M = 15, 2, 14, 21, 3
    plist = [O.init_params(d, L, seed=70 + k) for k in range(G)]
    ms = [lc.make_model(vpc.Reg_VAE, d, L, p) for p in plist]
    twins = [lc.make_model(vpc.Reg_VAE, d, L, p) for p in plist]
    g = torch.Generator().manual_seed(5)
    x = torch.rand(n, d, generator=g)
    calls = E.acquire_plan(G, d, L, x.shape, M, 1, 1)[2]
    eps = torch.randn(G, calls, M * n, L, generator=g)
    acq = E.EnsembleAcquirer(ms)
    info, action, R_hist, im_hist = acq.run(x.to(DEV), M, max_steps=1, eps=eps.to(DEV))
    mask0 = torch.zeros(n, d, dtype=torch.bool, device=DEV)
    for k in range(G):
        R = R_hist[k, 0, 0]
        assert torch.isfinite(R).all() and (R != -1e4).all()
        assert torch.equal(R, A.reward_matrix(twins[k], x.to(DEV), mask0, im_hist[k, 0, 0])), k
        assert np.array_equal(action[k, 0, :, 0].cpu().numpy(), np.argmax(R.cpu().numpy(), 1)), k
        # forward call 1 of the run (call 0 is the curve's first point) made the imputations
        port = O.TorchPort(plist[k], L)
        with torch.no_grad():
            z, _, _ = port.encoder(x.repeat(M, 1), torch.zeros(M * n, d, dtype=torch.bool), eps=eps[k, 1])
            want = port.decoder(z)[0].reshape(M, n, d)
        e = float((im_hist[k, 0, 0].cpu() - want).abs().max())
        lc.record("8_acquirer", "im", e, lc.FWD_ATOL)
        assert e <= lc.FWD_ATOL
    assert not torch.equal(R_hist[0, 0, 0], R_hist[1, 0, 0])


# ------------------------------------------------------------------------------------------ 9. EnsembleTrainer
ENS_D, ENS_B, ENS_K, ENS_G = 20, 37, 12, 3


@pytest.mark.parametrize("L,family", lc.ENSEMBLE_CASES, ids=ids(lc.ENSEMBLE_CASES))
def test_ensemble_members_equal_their_twins(L, family):
    """Plain, mask-augmented and point-net members for G = 3 against the stand-alone trainer of each member (same initial
    parameters, seed and hyperparameters, on its small-batch path): torch.equal on parameters, both Adam moments, gradient and
    loss terms after each of two steps with device draws, as tests/test_ensemble_gpu.py and test_ensemble_families_gpu.py."""
    d, B, G = ENS_D, ENS_B, ENS_G
    assert B <= ops.step_small_max_rows()
    torch.manual_seed(100 + L)
    if family == "eddi":
        ms = [vpc.Reg_EDDI(d, 500, ENS_K, L, TP, "e", "kl_reg").to(DEV) for _ in range(G)]
        ens_cls, twin_cls = vpc.EDDIEnsembleTrainer, vpc.EDDITrainer
    else:
        cls = vpc.Reg_VAE_mask if family == "mask" else vpc.Reg_VAE
        ms = [cls(d, 500, 10, L, TP, "e", "kl_reg").to(DEV) for _ in range(G)]
        ens_cls, twin_cls = (vpc.MaskEnsembleTrainer if family == "mask" else vpc.EnsembleTrainer), vpc.FusedTrainer
    tms = [copy.deepcopy(m) for m in ms]
    seeds, alphas = [11 + 3 * k for k in range(G)], [0.3, 0.6, 0.9]
    ens = ens_cls(ms, lr=1e-3, seeds=seeds)
    twins = [twin_cls(tms[k], lr=1e-3, seed=seeds[k]) for k in range(G)]
    g = torch.Generator().manual_seed(7 + L)
    x, mask = torch.rand(G, B, d, generator=g).to(DEV), (torch.rand(G, B, d, generator=g) < 0.7).to(DEV)
    for s in range(2):
        ens.step(x, mask, epoch=s + 1, alpha=alphas, beta=0.9)
        for k, tw in enumerate(twins):
            tw.step(x[k], mask[k], epoch=s + 1, alpha=alphas[k], beta=0.9)
            assert (tw.last_path == "small") if family == "eddi" else (tw.dominant_launch() == "step_small")
            theirs = (tw.model._flat, tw.exp_avg, tw.exp_avg_sq, tw.grad, tw.out9)
            ours = (ens.params[k], ens.exp_avg[k], ens.exp_avg_sq[k], ens.grad[k], ens.out9[k])
            for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "grad", "out9"), ours, theirs):
                assert a.shape == b.shape and bool(torch.isfinite(a).all()), (s, k, name)
                assert torch.equal(a, b), (s, k, name, float((a - b).abs().max()))
            assert ens.rng_offset == tw.rng_offset and ens.step_count == tw.step_count
    assert not torch.equal(ens.params[0], ens.params[1])


# ------------------------------------------------------------------------------------------ 10. EDDITrainer
@pytest.mark.parametrize("L,d,K,B,kind", lc.EDDI_CASES, ids=ids(lc.EDDI_CASES))
def test_eddi_trainer_vs_port(L, d, K, B, kind, monkeypatch):
    """EDDITrainer (it runs the VAE step's fused decoder kernel on [B][16] latent workspaces, and the trunk's head GEMM on dense
    [B][2 L] rows) against EDDIPort, as test_eddi_gpu.test_fused_trainer_d128_vs_oracle; d = 40 on the one-kernel small step and
    on the launch chain (VPC_STEP_SMALL=0), d = 128 on the chain."""
    seed = lc.case_seed(L, d, B) + K
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, d, generator=g)
    mk = torch.rand(B, d, generator=g) < 0.7
    mp = mk & (torch.rand(B, d, generator=g) < 0.7)
    eq, ep, eml = (torch.randn(B, L, generator=g) for _ in range(3))
    rt = "ml_reg" if kind == "ml_reg" else "kl_reg"
    for path in (("small", "chain") if d <= 64 else ("chain",)):
        set_env(monkeypatch, {"VPC_STEP_SMALL": "0"} if (path == "chain" and d <= 64) else {})
        torch.manual_seed(seed)
        model = vpc.vanilla_EDDI(d, 500, K, L, TP, "exp") if kind == "vanilla" else vpc.Reg_EDDI(d, 500, K, L, TP, "exp", rt)
        p = {k: v.detach().clone().float().requires_grad_(True) for k, v in model.state_dict().items() if k in EO.EDDI_KEYS}
        model = model.to(DEV)
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
        tr = vpc.EDDITrainer(model, lr=1e-3)
        if kind == "kl_reg":
            tr.step(x.to(DEV), mk.to(DEV), mask_p=mp.to(DEV), eps_q=eq.to(DEV), eps_p=ep.to(DEV), epoch=1, alpha=0.5)
        elif kind == "ml_reg":
            tr.step(x.to(DEV), mk.to(DEV), mask_p=mp.to(DEV), eps_q=eq.to(DEV), eps_p=ep.to(DEV), eps_ml=eml.to(DEV), epoch=1400,
                    alpha=0.8, beta=0.9)
        else:
            tr.step(x.to(DEV), mk.to(DEV), eps_q=eq.to(DEV), epoch=1)
        assert tr.last_path == path
        le = abs(tr.loss_value() - ref.item()) / abs(ref.item())
        lc.record("10_eddi_" + path, "loss", le, lc.LOSS_RTOL)
        errs = {}
        for k, prm in model.named_parameters():
            if k in p:
                assert prm.grad is not None and torch.isfinite(prm.grad).all(), k
                errs[k] = rel(prm.grad.cpu().numpy(), p[k].grad.numpy())
        assert set(errs) == set(EO.EDDI_KEYS)
        lc.record("10_eddi_" + path, "grad", max(errs.values()), lc.GRAD_RTOL)
        assert le <= lc.LOSS_RTOL, (path, tr.loss_value(), ref.item())
        for k, e in errs.items():
            assert e < lc.GRAD_RTOL, (path, k, e)


# ------------------------------------------------------------------------------------------ 11. the wide path
@pytest.mark.parametrize("d,L,B", lc.WIDE_CASES, ids=[f"L{L}-d{d}-B{B}" for d, L, B in lc.WIDE_CASES])
def test_wide_path_by_latent_width(d, L, B):
    """test_wide.test_reg_api_and_trainer_vs_oracle with the latent width passed in.  (14, 16, 37) is wide because of L alone."""
    seed = lc.case_seed(L, d, B)
    params = O.init_params(d, L, seed=seed)
    x, mask, mask_p, eq, ep, _ = lc.synth(B, d, L, seed=seed + 1)
    loss_ref, grads_ref, outs = O.torch_reg_step(params, L, x, mask, mask_p, eq, ep, alpha=0.8, beta=0.9)
    grads_ref = {k: v.numpy() for k, v in grads_ref.items()}
    m = lc.make_model(vpc.Reg_VAE, d, L, params)
    assert m._wide
    t = m.trainable()
    xd, mkd, mpd = x.to(DEV), mask.to(DEV), mask_p.to(DEV)
    md, mpu = ops.as_mask_u8(mkd), ops.as_mask_u8(mpd)
    zq, mq, lq = m._encode(xd, md, eps=eq.to(DEV))
    xq = m.decoder(zq)[0]
    zp, mp_, lp = m._encode(xd, mpu, eps=ep.to(DEV))
    xp = m.decoder(zp)[0]
    for got, want in ((mp_, outs[0]), (lp, outs[1]), (xp, outs[2]), (mq, outs[4]), (lq, outs[5]), (xq, outs[6])):
        e = float((got.detach().cpu() - want).abs().max())
        lc.record("11_wide", "forward", e, lc.FWD_ATOL)
        assert got.shape == want.shape and e <= lc.FWD_ATOL
    _, tl = m.loss(xd, xp, m.x_logvar, mp_, lp, xq, m.x_logvar, mq, lq, mkd, mpd, 1, beta=0.9, alpha=0.8)
    tl.backward()
    lc.check_loss_grads("11_wide_api", tl.item(), lc.flat_grads(m), m, loss_ref.item(), grads_ref, (d, L, B))
    out = m.forward(xd, mkd, mpd, "train")
    assert len(out) == 8 and out[2].shape == (B, d) and out[0].shape == (B, L) and out[3].shape == (1,)
    m2 = lc.make_model(vpc.Reg_VAE, d, L, params)
    tr = vpc.WideTrainer(m2)
    before = m2._flat.clone()
    tr.step(xd, mkd, mpd, eq.to(DEV), ep.to(DEV), alpha=0.8, beta=0.9)
    lc.check_loss_grads("11_wide_trainer", tr.loss_value(), tr.grad.cpu().numpy(), m2, loss_ref.item(), grads_ref, (d, L, B))
    assert not torch.equal(before, m2._flat)
    with pytest.raises(vpc.VpcError):
        vpc.FusedTrainer(m2)


def test_wide_routing_by_latent_width():
    assert not vpc.Reg_VAE(14, 500, 10, 15, TP, "exp", "kl_reg")._wide
    assert vpc.Reg_VAE(14, 500, 10, 16, TP, "exp", "kl_reg")._wide
    with pytest.raises(vpc.VpcError):
        vpc.Reg_VAE(14, 500, 10, 65, TP, "exp", "kl_reg")


# the parametrised tests and their case lists: test_latent_widths_cpu.py checks that these are the lists of latent_cases.py
CASES_OF = {
    "test_raw_forward_kernels_dense_latents": lc.FORWARD_CASES,
    "test_api_forward_loss_backward": lc.API_CASES,
    "test_fused_step_every_workgroup_shape": lc.STEP_CASES,
    "test_fused_two_adam_steps": lc.ADAM_CASES,
    "test_bf16_engines_vs_f32_path": lc.BF16_CASES,
    "test_mask_augmented_step": lc.AUGM_CASES,
    "test_inkernel_draws_equal_draw_step": lc.DRAW_CASES,
    "test_ensemble_evaluator_and_eval_sweep": lc.EVAL_CASES,
    "test_eval_vae_vs_closed_form": lc.EVAL_CASES,
    "test_reward_matrix_and_chains": lc.REWARD_CASES,
    "test_ensemble_members_equal_their_twins": lc.ENSEMBLE_CASES,
    "test_eddi_trainer_vs_port": lc.EDDI_CASES,
    "test_wide_path_by_latent_width": lc.WIDE_CASES,
}
