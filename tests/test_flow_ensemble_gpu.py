"""FlowEnsembleTrainer (vpc_amd/flow_ensemble.py) and the *_multi entries under it: member g of an ensemble computes BIT FOR BIT
what a stand-alone FlowTrainer(model_g, lr=lr_g, seed=seed_g) on the small path (VPC_FLOW_SMALL=128) computes - with injected
and with device draws, at the shapes where the few-row kernels take another path - and therefore also what the float64 closed
form (tests/flow_oracle.py) and the reference's recorded trajectories say, within the bounds of test_flow_small_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import flow_oracle as FO
from conftest import load_golden

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 1}
NO_GRAD = ["flow.flows.0.unnormalized_pdf", "flow.flows.1.unnormalized_pdf", "flow.flows.2.unnormalized_pdf",
           "encoder_mean.weight", "encoder_mean.bias", "encoder_logvar.weight", "encoder_logvar.bias",
           "decoder_logvar.0.weight", "decoder_logvar.0.bias"]
ALPHAS, BETAS, LRS = (0.3, 1.0, 0.7), (1.0, 0.5, 2.0), (1e-3, 2e-3, 5e-4)
ERR_ARG, ERR_SHAPE = 1, 2


@pytest.fixture(scope="module")
def fl():
    import vpc_amd
    from vpc_amd import flow
    return flow


@pytest.fixture(scope="module")
def E():
    from vpc_amd import flow_ensemble
    return flow_ensemble


@pytest.fixture(autouse=True)
def small(monkeypatch):
    monkeypatch.setenv("VPC_FLOW_SMALL", "128")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cls(fl, kind):
    return fl.REG_VAEFlow if kind == "reg" else fl.VAEFlow


def _models(fl, kind, G, d, H, seed0=0):
    """G models with different weights; the same call again gives their bit-equal twins."""
    out = []
    for g in range(G):
        torch.manual_seed(seed0 + g)
        out.append(_cls(fl, kind)(d, H, 10, 10, TP).cuda())
    return out


def _data(G, B, d, reg, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(G, B, d, generator=g)
    m = torch.rand(G, B, d, generator=g) < 0.7
    mp = (m & (torch.rand(G, B, d, generator=g) < 0.7)) if reg else None
    eps = torch.randn(G, 2 if reg else 1, B, 10, generator=g)
    return x.cuda(), m.cuda(), None if mp is None else mp.cuda(), eps.cuda()


def _same(ens, g, tr, what):
    v = ens.trainers[g]
    for name, a, b in (("loss", v.tail, tr.tail[:1]), ("out8", v.out8, tr.out8), ("grad", v.grad, tr.grad),
                       ("exp_avg", v.exp_avg, tr.exp_avg), ("exp_avg_sq", v.exp_avg_sq, tr.exp_avg_sq),
                       ("params", ens.params[g], tr.model._flat), ("accum", v.accum, tr.accum)):
        assert torch.equal(a, b), (what, g, name, float((a.double() - b.double()).abs().max()))
    assert bool(torch.isfinite(v.tail).all()) and ens.rng_offset == tr.rng_offset and ens.step_count == tr.step_count


def _run_pair(fl, E, kind, G, d, H, B, steps=2, inject=True, seeds=None, pms=30, order=None, members=None, stage="train",
              data_seed=5):
    """An ensemble and its stand-alone twins through `steps` steps; every member compared after every step."""
    reg = kind == "reg"
    al, be, lr = [(v * (G // 3 + 1))[:G] for v in (ALPHAS, BETAS, LRS)]
    seeds = list(range(G)) if seeds is None else seeds
    pms = [pms] * G if isinstance(pms, int) else pms
    ens = E.FlowEnsembleTrainer(_models(fl, kind, G, d, H), lr=lr, seeds=seeds, order=order)
    solo = {g: fl.FlowTrainer(m, lr=lr[g], seed=seeds[g]) for g, m in enumerate(_models(fl, kind, G, d, H))
            if members is None or g in members}
    for s in range(steps):
        x, m, mp, eps = _data(G, B, d, reg, data_seed + s)
        inj = dict(mask_p=mp, eps=eps) if inject else {}
        ens.step(x, m, alpha=al, beta=be, p_missingness=pms, stage=stage, **inj)
        for g, tr in solo.items():
            injg = dict(mask_p=None if mp is None else mp[g], eps=eps[g]) if inject else {}
            tr.step(x[g], m[g], alpha=al[g], beta=be[g], p_missingness=pms[g], stage=stage, **injg)
            assert tr.last_path == "small"
            _same(ens, g, tr, (kind, d, H, B, s))
            if not inject:
                assert torch.equal(ens.trainers[g].eps, tr.eps)
                if reg:
                    assert torch.equal(ens.trainers[g].mask_p, tr.mask_p)
    return ens, solo


# (d, hid, B of REG_VAEFlow; VAEFlow runs at 2 B, the same R): scalar first layer, K = 10 single-chunk tail, hid % 16 != 0 /
# every layer scalar, R = 34 crosses a 32-row block, member slices padded / 16-byte build, K = 24 tail / the wine shape, R = 128
SHAPES = [(5, 36, 1), (5, 37, 17), (12, 36, 37), (12, 500, 64)]


@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("d,H,B", SHAPES)
def test_bitwise_injected(fl, E, kind, d, H, B):
    """G = 3 members with different weights, data, alpha, beta and lr, two steps (so Adam's state matters).  VAEFlow at
    (12, 500, 128) is the issue's vanilla-only R = 128 case."""
    ens, _ = _run_pair(fl, E, kind, 3, d, H, B if kind == "reg" else 2 * B)
    assert len(ens.last_launches) == 21


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_device_draws(fl, E, kind):
    ens, solo = _run_pair(fl, E, kind, 3, 12, 36, 37, inject=False, seeds=[11, 3, 7], pms=[30, 50, 10])
    assert not torch.equal(ens.eps[0], ens.eps[1])
    if kind == "reg":  # keep_prob_g took effect: member 1 (50 %) keeps fewer entries than member 2 (10 %)
        assert float(ens.mask_p[1].sum()) < float(ens.mask_p[2].sum())


def test_inside_flag_is_per_member_and_pass(fl, E):
    """Member 1's p-pass eps all lie outside [-1, 1]: its p pass is the identity (z == eps exactly), its q pass and both
    passes of members 0 and 2 are splined; all three equal their stand-alone runs."""
    G, d, H, B = 3, 12, 36, 37
    x, m, mp, eps = _data(G, B, d, True, 21)
    eps[1, 1] = torch.sign(eps[1, 1] + 1e-3) * (1.05 + eps[1, 1].abs())
    ens = E.FlowEnsembleTrainer(_models(fl, "reg", G, d, H))
    ens.step(x, m, mask_p=mp, eps=eps, alpha=list(ALPHAS))
    for g, mdl in enumerate(_models(fl, "reg", G, d, H)):
        tr = fl.FlowTrainer(mdl, seed=g)
        tr.step(x[g], m[g], mask_p=mp[g], eps=eps[g], alpha=ALPHAS[g])
        _same(ens, g, tr, "flag")
        v = ens.trainers[g]
        assert torch.equal(v.z, tr.z) and torch.equal(v.zlp, tr.zlp)
        for p in range(2):
            identity = torch.equal(v.z[p * B:(p + 1) * B], v.eps[p * B:(p + 1) * B])
            assert identity == (g == 1 and p == 1), (g, p)
    assert bool((ens.eps[1, B:].abs() > 1).all()) and bool((ens.eps[1, :B].abs() <= 1).any())


def test_nine_members_both_orders(fl, E):
    runs = []
    for order in (0, 1):
        ens, _ = _run_pair(fl, E, "reg", 9, 12, 36, 17, order=order, members=(0, 8))
        assert ens.order == order
        runs.append((ens.params.clone(), ens.grad.clone(), ens.loss_f32.clone(), ens.exp_avg_sq.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_shared_data_equals_per_member_data(fl, E, kind):
    G, d, H, B = 3, 12, 36, 17
    x, m, mp, eps = _data(1, B, d, kind == "reg", 9)
    rep = lambda t: None if t is None else t.expand(G, *t.shape[1:]).contiguous()
    out = []
    for shared in (True, False):
        ens = E.FlowEnsembleTrainer(_models(fl, kind, G, d, H), lr=list(LRS))
        pick = (lambda t: None if t is None else t[0]) if shared else rep
        for _ in range(2):
            ens.step(pick(x), pick(m), mask_p=pick(mp), eps=pick(eps), alpha=list(ALPHAS))
        out.append((ens.params.clone(), ens.grad.clone(), ens.loss_f32.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not torch.equal(out[0][0][0], out[0][0][1])


# ------------------------------------------------------------------------------------------------ float64 closed form
def _n_flagged(P, x, mask, mask_p, eps):
    """Spline decisions, over both passes, that fp32 may take the other way (as test_flow_small_gpu.py counts them)."""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    n = 0
    for k, mk in enumerate([mask, mask_p]):
        mk = np.asarray(mk, np.float64)
        ecache, _ = FO.mlp(P, FO.ENC, np.concatenate([np.asarray(x, np.float64) * mk, mk], 1))
        cache = FO.flow_fwd(ecache[-1], np.asarray(eps[k], np.float64))[2]
        if cache is not None:
            n += int(FO.flagged(FO.flow_flags(cache)).sum())
    return n


def test_member_vs_float64_closed_form(fl, E):
    """Member 1 of a G = 3 REG ensemble at (12, 500, 37), alpha 0.5: loss 2e-5 relative, every gradient 2e-4 of its max.  Seed
    149 / 150: test_flow_small_gpu.py's (12, 37) case, at which no spline decision sits on a knot in float64 (checked here too)."""
    G, d, H, B, g1 = 3, 12, 500, 37, 1
    P = FO.init_params(d, H, seed=149)
    rng = np.random.default_rng(150)
    x = rng.random((B, d)).astype(np.float32)
    mask = rng.random((B, d)) < 0.7
    mask_p = mask & (rng.random((B, d)) < 0.7)
    eps = rng.standard_normal((2, B, FO.L)).astype(np.float32)
    assert _n_flagged(P, x, mask, mask_p, eps) == 0
    models = _models(fl, "reg", G, d, H)
    sd = models[g1].state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in P.items()})
    models[g1].load_state_dict(sd)
    ens = E.FlowEnsembleTrainer(models)
    ens.grad.fill_(float("nan"))  # (every gradient is written by a rows_bwd launch: nothing is accumulated)
    xs, ms, mps, es = _data(G, B, d, True, 3)
    xs[g1], ms[g1], mps[g1], es[g1] = _dev(x), _dev(mask), _dev(mask_p), _dev(eps)
    ens.step(xs, ms, mask_p=mps, eps=es, alpha=[1.0, 0.5, 0.2])
    r = FO.step(P, x, mask, mask_p, eps, alpha=0.5)
    loss = ens.trainers[g1].loss_value()
    print("loss", loss, r["loss"])
    assert abs(loss - r["loss"]) <= 2e-5 * abs(r["loss"])
    flat, off = ens.grad[g1].cpu().double(), 0
    for k in FO.TRAINABLE:
        n, ref = P[k].size, torch.from_numpy(r["grads"][k]).double()
        err = float((flat[off:off + n].view(ref.shape) - ref).abs().max() / (ref.abs().max() + 1e-30))
        print(k, f"err {err:.3e}")
        assert err <= 2e-4, (k, err)
        off += n
    assert bool(torch.isfinite(ens.grad).all())


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_reference_trajectory(fl, E, kind):
    """Both members of a G = 2 ensemble start from the golden file's param0 and take its five recorded steps: losses within
    2e-5, final parameters within 5e-5, the epoch total, and the 9 tensors without a gradient bitwise unchanged."""
    g = load_golden(f"flow_traj_{kind}_d12.npz")
    models = []
    for _ in range(2):
        m = _cls(fl, kind)(g["x"].shape[1], int(g["hid"]), 10, 10, TP)
        m.load_state_dict({k[7:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("param0.")})
        models.append(m.cuda())
    before = [{k: v.detach().clone() for k, v in m.state_dict().items() if k in NO_GRAD} for m in models]
    ens = E.FlowEnsembleTrainer(models, lr=1e-3)
    x, m = _dev(g["x"]), _dev(g["mask"]).bool()
    total = 0.0
    for s in range(len(g["losses"])):
        ens.step(x, m, mask_p=_dev(g["mask_p"][s]) if kind == "reg" else None, eps=_dev(g["eps"][s]), alpha=float(g["alpha"]))
        for got in ens.loss_values():
            assert abs(got - g["losses"][s]) <= 2e-5 * abs(g["losses"][s]), (s, got, g["losses"][s])
        total += g["losses"][s]
    for got in ens.epoch_total():
        assert abs(got - total) <= 2e-5 * abs(total)
    assert ens.epoch_total() == [0.0, 0.0]
    for mi, mdl in enumerate(models):
        sd = mdl.state_dict()
        for k, v in g.items():
            if k.startswith("param5."):
                ref = torch.from_numpy(v).double()
                err = float((sd[k[7:]].cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-30))
                assert err <= 5e-5, (k, err)
        for k, v in before[mi].items():
            assert torch.equal(sd[k], v), k


# ------------------------------------------------------------------------------------------------ launches
class _Recorder:
    """Stands in for the loaded library: records every vpc_* symbol fetched, hands out the real one."""

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        if name.startswith("vpc_"):
            self.names.append(name)
        return getattr(self.real, name)


def test_launch_set_does_not_depend_on_G(fl, E, monkeypatch):
    from vpc_amd import _lib
    seen = {}
    for G in (1, 9):
        ens = E.FlowEnsembleTrainer(_models(fl, "reg", G, 12, 36))
        x, m, _, _ = _data(G, 17, 12, True, 2)
        ens.step(x, m, alpha=0.5)
        rec = _Recorder(_lib.lib())
        monkeypatch.setattr(_lib, "_lib", rec)
        ens.step(x, m, alpha=0.5)
        monkeypatch.setattr(_lib, "_lib", rec.real)
        seen[G] = rec.names
        assert tuple(rec.names) == E.LAUNCHES == ens.last_launches and len(rec.names) == 21
        assert all(n.endswith("_multi") or n == "vpc_flow_multi_prep" for n in rec.names)
    assert seen[1] == seen[9]


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_short_last_batch(fl, E, kind):
    """Five steps at B = 64, then one at B = 37: the workspaces are rebuilt, members still equal their stand-alone runs."""
    G, d, H = 3, 12, 36
    ens = E.FlowEnsembleTrainer(_models(fl, kind, G, d, H), lr=list(LRS), seeds=[4, 5, 6])
    solo = [fl.FlowTrainer(m, lr=LRS[g], seed=4 + g) for g, m in enumerate(_models(fl, kind, G, d, H))]
    for s, B in enumerate([64] * 5 + [37]):
        x, m, _, _ = _data(G, B, d, False, 40 + s)
        ens.step(x, m, alpha=list(ALPHAS), p_missingness=30)
        assert ens.xin.shape[1] == (2 if kind == "reg" else 1) * B
        for g, tr in enumerate(solo):
            tr.step(x[g], m[g], alpha=ALPHAS[g], p_missingness=30)
    for g, tr in enumerate(solo):
        _same(ens, g, tr, "short")
        assert torch.equal(ens.trainers[g].eps, tr.eps)
    tot = ens.epoch_total()
    assert tot == [tr.epoch_total() for tr in solo]


def test_evaluate_stage(fl, E):
    _run_pair(fl, E, "reg", 3, 12, 36, 37, steps=1, stage="evaluate")


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_two_runs_are_bitwise_equal(fl, E, kind):
    runs = []
    for _ in range(2):
        ens = E.FlowEnsembleTrainer(_models(fl, kind, 3, 12, 36), seeds=[11, 3, 7])
        x, m, _, _ = _data(3, 37, 12, False, 8)
        losses = []
        for _s in range(4):
            ens.step(x, m, alpha=0.5, p_missingness=[30, 50, 10])
            losses.append(ens.loss_f32.clone())
        runs.append((torch.stack(losses), ens.params.clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    assert bool(torch.isfinite(runs[0][0]).all())


# ------------------------------------------------------------------------------------------------ train_sweep
def _sweep_setup(fl):
    from torch.utils.data import DataLoader, TensorDataset
    torch.manual_seed(0)
    x, m = torch.rand(74, 12), torch.rand(74, 12) < 0.7
    loader = DataLoader(TensorDataset(x, m), batch_size=37, shuffle=False)
    cfgs = [dict(vae_type=f"{'reg' if k == 'reg' else 'vanilla'}_flow{i + 1}", alpha=ALPHAS[i], p_missingness=(30, 50, 10)[i],
                 seed=7 + i) for k in ("reg", "van") for i in range(3)]
    build = lambda: _models(fl, "reg", 3, 12, 36) + _models(fl, "van", 3, 12, 36, seed0=10)
    return loader, cfgs, build


def test_train_sweep(fl, E, tmp_path, monkeypatch, capsys):
    import vpc_amd
    from vpc_amd import harness
    loader, cfgs, build = _sweep_setup(fl)
    made = []
    real = harness.FlowEnsembleTrainer
    monkeypatch.setattr(harness, "FlowEnsembleTrainer", lambda ms, **kw: made.append(len(ms)) or real(ms, **kw))
    (tmp_path / "sweep").mkdir()
    monkeypatch.chdir(tmp_path / "sweep")
    capsys.readouterr()
    out = vpc_amd.train_sweep((loader, None), cfgs, 50, 12, 36, 10, 1, 10, "toy", TP, "exp", 1, 1, max_epochs=2,
                              reg_type="kl_reg", models=build())
    lines = sorted(l for l in capsys.readouterr().out.splitlines() if l.startswith("Epoch"))
    assert made == [3, 3] and len(lines) == 12
    (tmp_path / "solo").mkdir()
    monkeypatch.chdir(tmp_path / "solo")
    solo_lines = []
    for c, mdl, got in zip(cfgs, build(), out):
        vpc_amd.train((loader, None), 50, 12, 36, 10, 1, 10, "toy", TP, "exp", c["vae_type"], 1, 1, max_epochs=2,
                      alpha=c["alpha"], p_missingness=c["p_missingness"], reg_type="kl_reg", seed=c["seed"], model=mdl)
        solo_lines += [l for l in capsys.readouterr().out.splitlines() if l.startswith("Epoch")]
        sd, ref = got.state_dict(), mdl.state_dict()
        assert list(sd) == list(ref)
        for k in ref:
            assert torch.equal(sd[k], ref[k]), (c["vae_type"], k)
        ck = vpc_amd.checkpoint_path("exp", "toy", c["vae_type"], 50, c["alpha"], c["p_missingness"], "kl_reg")
        saved = torch.load(tmp_path / "sweep" / ck, weights_only=True)
        for k in ref:
            assert torch.equal(saved[k], ref[k].cpu()), (c["vae_type"], k)
    assert lines == sorted(solo_lines)


def test_train_sweep_without_the_variable(fl, tmp_path, monkeypatch):
    import vpc_amd
    from vpc_amd import harness
    loader, cfgs, build = _sweep_setup(fl)
    monkeypatch.delenv("VPC_FLOW_SMALL", raising=False)
    monkeypatch.chdir(tmp_path)

    def refuse(*a, **k):
        raise AssertionError("FlowEnsembleTrainer constructed with VPC_FLOW_SMALL unset")

    monkeypatch.setattr(harness, "FlowEnsembleTrainer", refuse)
    out = vpc_amd.train_sweep((loader, None), cfgs, 50, 12, 36, 10, 1, 10, "toy", TP, "exp", 1, 1, max_epochs=1,
                              reg_type="kl_reg", models=build(), verbose=False)
    assert len(out) == 6


# ------------------------------------------------------------------------------------------------ refusals
def _refusal_cases():
    """Per entry: the argument names in ABI order, a valid call on small buffers (M = 4 rows, N = 8, K = 8, G = 2, d = 4,
    B = 2, R = 4), the outputs, and the bad arguments.  Buffers are 16-byte aligned NaN-filled device arrays."""
    nan = lambda n: torch.full((n,), float("nan"), device="cuda")
    buf = {k: nan(256) for k in ("x", "w", "bias", "y", "dy", "dx", "dw", "db", "t", "eps", "z", "zlp", "dt", "xin", "mask",
                                 "mask_p", "Y", "G", "gz", "gzlp", "params", "grad", "m", "v", "lossf", "accum")}
    buf["out8"] = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    buf["scratch"] = torch.full((64,), float("nan"), dtype=torch.float64, device="cuda")
    buf["members"] = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = lambda k: ctypes.c_void_p(buf[k].data_ptr())
    G, M, N, K = 2, 4, 8, 8
    cases = {
        "vpc_rows_fwd_multi": (
            dict(x=p("x"), ldx=K, x_stride=32, w=p("w"), bias=p("bias"), wb_stride=128, y=p("y"), ldy=N, y_stride=32, G=G, M=M,
                 N=N, K=K, act=0, act_split=0, order=0, stream=None),
            [("x", None, ERR_ARG), ("y", None, ERR_ARG), ("G", 0, ERR_ARG), ("G", 4097, ERR_ARG), ("M", 129, ERR_SHAPE),
             ("N", dict(N=1025, ldy=1025), ERR_SHAPE), ("x_stride", 28, ERR_ARG), ("y_stride", 6, ERR_ARG), ("wb_stride", 70, ERR_ARG),
             ("order", 2, ERR_ARG)]),
        "vpc_rows_bwd_multi": (
            dict(dy=p("dy"), lddy=N, dy_stride=32, y_gate=None, ldyg=N, yg_stride=0, gate=0, gate_split=0, w=p("w"), x=p("x"),
                 ldx=K, x_stride=32, x_out=None, ldxo=K, xo_stride=0, act_prev=0, dx=p("dx"), lddx=K, dx_stride=32, dw=p("dw"),
                 db=p("db"), wb_stride=128, G=G, M=M, N=N, K=K, accumulate=0, order=0, stream=None),
            [("dy", None, ERR_ARG), ("G", 0, ERR_ARG), ("G", 4097, ERR_ARG), ("M", 129, ERR_SHAPE),
             ("N", dict(N=1025, lddy=1025), ERR_SHAPE), ("dy_stride", 28, ERR_ARG), ("dx_stride", 6, ERR_ARG), ("x_stride", 34, ERR_ARG), ("wb_stride", 60, ERR_ARG)]),
        "vpc_flow_multi_prep": (
            dict(x=p("x"), x_stride=8, mask=p("mask"), mask_stride=0, mask_p=p("mask_p"), mask_p_stride=8, xin=p("xin"),
                 xin_stride=32, eps=p("eps"), eps_stride=40, members=p("members"), G=G, draw=1, R=4, B=2, d=4, offset=0,
                 offset_eps=1 << 40, stream=None),
            [("x", None, ERR_ARG), ("members", None, ERR_ARG), ("G", 0, ERR_ARG), ("G", 4097, ERR_ARG), ("x_stride", 7, ERR_ARG),
             ("xin_stride", 31, ERR_ARG), ("eps_stride", 39, ERR_ARG), ("mask_p", None, ERR_ARG)]),
        "vpc_flow_fwd_multi": (
            dict(t=p("t"), ldt=100, t_stride=400, eps=p("eps"), z=p("z"), zlp=p("zlp"), stride10=40, G=G, R=4, B=2, stream=None),
            [("t", None, ERR_ARG), ("z", None, ERR_ARG), ("G", 0, ERR_ARG), ("G", 4097, ERR_ARG), ("t_stride", 399, ERR_ARG),
             ("stride10", 39, ERR_ARG)]),
        "vpc_flow_bwd_multi": (
            dict(t=p("t"), ldt=100, t_stride=400, eps=p("eps"), dz=p("z"), dz2=p("gz"), dzlp=p("gzlp"), stride10=40, dt=p("dt"),
                 lddt=100, dt_stride=400, G=G, R=4, B=2, stream=None),
            [("dt", None, ERR_ARG), ("G", 0, ERR_ARG), ("G", 4097, ERR_ARG), ("dt_stride", 399, ERR_ARG),
             ("stride10", 39, ERR_ARG)]),
        "vpc_flow_loss_multi": (
            dict(x=p("x"), x_stride=8, mask=p("mask"), mask_stride=8, mask_p=None, mask_p_stride=0, xmq=p("Y"), xmp=None, ldxm=4,
                 xm_stride=8, zq=p("z"), zp=None, zlq=p("zlp"), zlpp=None, gxq=p("G"), gxp=None, ldg=4, g_stride=8, gzq=p("gz"),
                 gzp=None, gzlq=p("gzlp"), gzlpp=None, stride10=20, scratch=p("scratch"), scratch_bytes=512, out8=p("out8"),
                 lossf=p("lossf"), accum=p("accum"), members=p("members"), G=G, B=2, d=4, stage=0,
                 gscale=ctypes.c_float(0.5), gated=1, stream=None),
            [("x", None, ERR_ARG), ("out8", None, ERR_ARG), ("members", None, ERR_ARG), ("G", 0, ERR_ARG), ("G", 4097, ERR_ARG),
             ("xm_stride", 7, ERR_ARG), ("stride10", 19, ERR_ARG), ("scratch_bytes", 64, ERR_ARG)]),
        "vpc_adam_step_multi": (
            dict(params=p("params"), grads=p("grad"), m=p("m"), v=p("v"), row_stride=64, n=50, members=p("members"), G=G,
                 b1=ctypes.c_float(0.9), b2=ctypes.c_float(0.999), eps=ctypes.c_float(1e-8), step=1, stream=None),
            [("params", None, ERR_ARG), ("members", None, ERR_ARG), ("G", 0, ERR_ARG), ("G", 4097, ERR_ARG),
             ("row_stride", 49, ERR_ARG), ("step", 0, ERR_ARG)]),
    }
    return buf, cases


def test_entries_refuse_before_any_launch(E):
    import vpc_amd
    lb = vpc_amd._lib.lib()
    buf, cases = _refusal_cases()
    for name, (valid, bad) in cases.items():
        for arg, value, code in bad:
            args = dict(valid)
            assert arg in args, (name, arg)
            args.update(value if isinstance(value, dict) else {arg: value})  # (a dict: the pitch grows with N)
            assert getattr(lb, name)(*args.values()) == code, (name, arg, value)
    torch.cuda.synchronize()
    for k, t in buf.items():  # nothing was launched: every buffer still holds what it was filled with
        if k != "members":
            assert bool(torch.isnan(t).all()), k
    assert int(buf["members"].sum()) == 0


def test_step_refuses_before_counting(fl, E):
    import vpc_amd
    ens = E.FlowEnsembleTrainer(_models(fl, "reg", 2, 12, 36))
    x, m, mp, eps = _data(2, 65, 12, True, 1)
    with pytest.raises(vpc_amd.VpcError, match="130 stacked rows"):
        ens.step(x, m)
    van = E.FlowEnsembleTrainer(_models(fl, "van", 2, 12, 36))
    with pytest.raises(vpc_amd.VpcError, match="129 stacked rows"):
        van.step(*_data(2, 129, 12, False, 1)[:2])
    x, m, mp, eps = _data(2, 17, 12, True, 1)
    for kw in (dict(mask_p=mp), dict(eps=eps)):
        with pytest.raises(vpc_amd.VpcError, match="inject all"):
            ens.step(x, m, **kw)
    with pytest.raises(vpc_amd.VpcError, match="inject all"):
        van.step(x, m, mask_p=mp, eps=eps[:, :1])
    for t in (ens, van):
        assert t.step_count == 0 and t.rng_offset == 0 and t.last_launches == ()
    ens.step(x, m, mask_p=mp, eps=eps)
    assert ens.step_count == 1 and ens.rng_offset > 0
    moved = ens.models[1]
    moved._flat = moved._flat.clone()  # the member leaves the stack
    with pytest.raises(vpc_amd.VpcError, match="member 1 no longer sits"):
        ens.step(x, m, mask_p=mp, eps=eps)
