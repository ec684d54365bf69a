"""MIWEnsembleTrainer (vpc_amd/miw_ensemble.py: vpc_miw_multi_prep -> vpc_miw_small_fwd_multi -> vpc_miw_loss_multi ->
vpc_miw_small_bwd_multi -> vpc_miw_small_tail_multi) on the GPU.  The yardstick: a member is bit-identical to a stand-alone
MIWTrainer on the small path with small_rb = ens.rb whenever blocks_per_member == ceil(R / rb) <= compute units; with fewer
blocks per member only the summation order differs, and the member agrees with the stand-alone step at the bounds
tests/test_miwae_small_gpu.py uses between two summation orders of this math (flat gradient and loss 2e-5, each of the twelve
gradients 2e-4 of its max, parameters after a step 5e-5)."""
import copy

import numpy as np
import pytest
import torch

import miw_ensemble_cases as EC
import miwae_cases as C
import miwae_small_cases as SC
from conftest import load_golden

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 1}
ALL_ROWS = str(1 << 20)  # a VPC_MIW_SMALL above every shape of this file
DEV = "cuda"


@pytest.fixture(scope="module")
def mw():
    import vpc_amd
    from vpc_amd import miwae
    return miwae


@pytest.fixture(scope="module")
def me():
    from vpc_amd import miw_ensemble
    return miw_ensemble


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, ref, tol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = float((got - ref).abs().max() / (ref.abs().max() + 1e-30))
    print(what, f"{err:.3e} (bound {tol:.0e})")
    assert err <= tol, (what, err)


def _model(mw, c):
    cls = mw.Reg_MIWAE if c["reg"] else mw.MIWAE
    model = cls(c["d"], 500, 10, c["L"], TP, c["S"], 1)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c["params"].items()})
    return model.cuda()


def _stack(cases, key):
    return None if cases[0][key] is None else torch.stack([_dev(c[key]) for c in cases])


def _solo(mw, c, rb, **kw):
    tr = mw.MIWTrainer(_model(mw, c), **kw)
    tr.small_rb = rb
    return tr


def _same_state(view, tr, what):
    """Flat gradient, out8, parameters and both Adam moments of a member view against a stand-alone trainer, bit for bit."""
    for name, a, b in (("grad", view.grad, tr.grad), ("out8", view.out8, tr.out8), ("params", view.model._flat, tr.model._flat),
                       ("exp_avg", view.exp_avg, tr.exp_avg), ("exp_avg_sq", view.exp_avg_sq, tr.exp_avg_sq)):
        assert torch.equal(a, b), (what, name, float((a.double() - b.double()).abs().max()))


def _units(R, rb):
    return -(-R // rb)


# ------------------------------------------------------------------------------------------------ 1. edge shapes
@pytest.mark.parametrize("rb", EC.RBS)
@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("shape", SC.EDGE_SHAPES)
def test_edge_shapes_bit_for_bit(mw, me, monkeypatch, shape, kind, rb):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    cases = EC.member_cases(shape, kind)
    R = (2 if kind == "reg" else 1) * shape[0]
    ens = me.MIWEnsembleTrainer([_model(mw, c) for c in cases], lr=1e-3, rb=rb, blocks_per_member=_units(R, rb))
    ens.step(_stack(cases, "x"), _stack(cases, "mask"), mask_p=_stack(cases, "mask_p"), eps=_stack(cases, "eps"),
             alpha=EC.MEMBER_ALPHAS)
    assert (ens.rb, ens.blocks_per_member) == (rb, _units(R, rb))
    for g, c in enumerate(cases):
        tr = _solo(mw, c, rb, lr=1e-3)
        tr.step(_dev(c["x"]), _dev(c["mask"]), mask_p=_dev(c["mask_p"]), eps=_dev(c["eps"]), alpha=EC.MEMBER_ALPHAS[g])
        assert tr.last_path == "small"
        _same_state(ens.trainers[g], tr, (shape, kind, rb, g))
    for g in (1, 2):  # a launch that served every member from member 0 would pass the above only if the members were equal
        assert not torch.equal(ens.grad[g], ens.grad[0]) and not torch.equal(ens.params[g], ens.params[0])
        assert not torch.equal(ens.out8[g], ens.out8[0])


# ------------------------------------------------------------------------------------------------ 2. device draws
@pytest.mark.parametrize("kind", ["reg", "van"])
def test_device_draws_two_steps(mw, me, monkeypatch, kind):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    cases = EC.member_cases(EC.DRAW_SHAPE, kind)
    ens = me.MIWEnsembleTrainer([_model(mw, c) for c in cases], lr=1e-3, seeds=EC.DRAW_SEEDS, rb=1, blocks_per_member=256)
    solo = [_solo(mw, c, 1, lr=1e-3, seed=s) for c, s in zip(cases, EC.DRAW_SEEDS)]
    x, m = _stack(cases, "x"), _stack(cases, "mask")
    for step in range(2):
        ens.step(x, m.bool(), alpha=0.5, p_missingness=EC.DRAW_PMS)
        for g, tr in enumerate(solo):
            tr.step(x[g], m[g].bool(), alpha=0.5, p_missingness=EC.DRAW_PMS[g])
            v = ens.trainers[g]
            assert torch.equal(v.eps, tr.eps), (step, g)
            if kind == "reg":
                assert torch.equal(v.mask_p, tr.mask_p), (step, g)
                assert 0 < float(v.mask_p.sum()) < float(m[g].sum())
            assert v.rng_offset == tr.rng_offset > 0
            _same_state(v, tr, (kind, step, g))
    assert not torch.equal(ens.eps[0], ens.eps[1])


# ------------------------------------------------------------------------------------------------ 3. capped blocks
@pytest.mark.parametrize("shape,rb,blocks", EC.CAPPED)
def test_capped_blocks_agree_at_the_summation_order_bounds(mw, me, monkeypatch, shape, rb, blocks):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    cases = EC.member_cases(shape, "reg", (3, 4))
    R = 2 * shape[0]
    assert blocks < _units(R, rb) and _units(R, rb) % blocks  # every workgroup walks several blocks, not all the same number
    ens = me.MIWEnsembleTrainer([_model(mw, c) for c in cases], lr=1e-3, rb=rb, blocks_per_member=blocks)
    ens.step(_stack(cases, "x"), _stack(cases, "mask"), mask_p=_stack(cases, "mask_p"), eps=_stack(cases, "eps"), alpha=C.ALPHA)
    assert (ens.rb, ens.blocks_per_member) == (rb, blocks)
    for g, c in enumerate(cases):
        tr = _solo(mw, c, rb, lr=1e-3)
        tr.step(_dev(c["x"]), _dev(c["mask"]), mask_p=_dev(c["mask_p"]), eps=_dev(c["eps"]), alpha=C.ALPHA)
        v = ens.trainers[g]
        _close(v.grad, tr.grad, 2e-5, ("flat gradient", g))
        assert abs(v.loss_value() - tr.loss_value()) <= 2e-5 * abs(tr.loss_value())
        for (k, pa), pb in zip(v.model.named_parameters(), tr.model.parameters()):
            _close(pa.grad, pb.grad, 2e-4, ("gradient", g, k))
        _close(v.model._flat, tr.model._flat, 5e-5, ("parameters after the step", g))


# ------------------------------------------------------------------------------------------------ 4. more than eight members
def test_nine_members_under_both_workgroup_orders(mw, me, monkeypatch):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    cases = EC.member_cases(EC.DRAW_SHAPE, "van", tuple(range(20, 29)))
    tr = _solo(mw, cases[8], 1, lr=1e-3)
    c = cases[8]
    tr.step(_dev(c["x"]), _dev(c["mask"]), eps=_dev(c["eps"]), alpha=C.ALPHA)
    runs = []
    for order in (0, 1):
        ens = me.MIWEnsembleTrainer([_model(mw, c) for c in cases], lr=1e-3, rb=1, blocks_per_member=256)
        ens.order = order
        ens.step(_stack(cases, "x"), _stack(cases, "mask"), eps=_stack(cases, "eps"), alpha=C.ALPHA)
        _same_state(ens.trainers[8], tr, ("order", order))
        runs.append((ens.grad.clone(), ens.params.clone(), ens.out8.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0][8], runs[0][0][0])


# ------------------------------------------------------------------------------------------------ 5. five steps, wine shape
@pytest.mark.parametrize("kind", ["reg", "van"])
def test_five_steps_at_the_wine_shape_then_a_short_batch(mw, me, monkeypatch, kind):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    W = EC.WINE_MEMBERS
    c = C.trainer_case(EC.WINE, kind)
    P = 2 if kind == "reg" else 1
    x, m = _dev(c["x"]), _dev(c["mask"]).bool()
    ens = me.MIWEnsembleTrainer([_model(mw, c) for _ in range(4)], lr=W["lr"], seeds=W["seed"])
    for _ in range(5):
        ens.step(x, m, alpha=W["alpha"], p_missingness=W["p_missingness"])
    rb = ens.rb
    assert ens.blocks_per_member == _units(P * 64, rb)  # the default rule keeps the stand-alone grid at G = 4
    solo = [_solo(mw, c, rb, lr=W["lr"][g], seed=W["seed"][g]) for g in range(4)]
    for g, tr in enumerate(solo):
        for _ in range(5):
            tr.step(x, m, alpha=W["alpha"][g], p_missingness=W["p_missingness"][g])
        assert tr.last_path == "small"
    totals = ens.epoch_total(reset=False)
    for g, tr in enumerate(solo):
        assert torch.equal(ens.params[g], tr.model._flat), g
        assert totals[g] == tr.epoch_total(reset=False), g
    assert len(set(totals)) == 4
    xs, ms = x[:EC.SHORT_BATCH], m[:EC.SHORT_BATCH]
    ens.step(xs, ms, alpha=W["alpha"], p_missingness=W["p_missingness"])
    assert ens.blocks_per_member == _units(P * EC.SHORT_BATCH, ens.rb)
    for g, tr in enumerate(solo):
        tr.small_rb = ens.rb
        tr.step(xs, ms, alpha=W["alpha"][g], p_missingness=W["p_missingness"][g])
        _same_state(ens.trainers[g], tr, ("short batch", g))
        assert ens.trainers[g].rng_offset == tr.rng_offset


# ------------------------------------------------------------------------------------------------ 6. shared data
def test_shared_data_equals_per_member_data(mw, me, monkeypatch):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    cases = EC.member_cases(EC.DRAW_SHAPE, "reg")
    x, m = _dev(cases[0]["x"]), _dev(cases[0]["mask"])
    runs = []
    for per_member in (False, True):
        ens = me.MIWEnsembleTrainer([_model(mw, c) for c in cases], lr=1e-3, seeds=EC.DRAW_SEEDS)
        xx = x.expand(3, *x.shape).contiguous() if per_member else x
        mm = m.expand(3, *m.shape).contiguous() if per_member else m
        ens.step(xx, mm, alpha=EC.MEMBER_ALPHAS)
        runs.append((ens.grad.clone(), ens.params.clone(), ens.out8.clone(), ens.eps.clone(), ens.mask_p.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. the reference's recordings
@pytest.mark.parametrize("kind", ["reg", "van"])
def test_trajectory_vs_reference(mw, me, monkeypatch, kind):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    g = load_golden(f"miwae_traj_{kind}_d14.npz")
    cls = mw.Reg_MIWAE if kind == "reg" else mw.MIWAE

    def load():
        torch.manual_seed(0)
        model = cls(g["x"].shape[1], 500, 10, int(g["L"]), TP, int(g["S"]), 1)
        model.load_state_dict({k[7:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("param0.")})
        return model.cuda()

    ens = me.MIWEnsembleTrainer([load(), load()], lr=1e-3)
    x, m = _dev(g["x"]), _dev(g["mask"]).bool()
    total = 0.0
    for s in range(len(g["losses"])):
        ens.step(x, m, mask_p=_dev(g["mask_p"][s]) if kind == "reg" else None, eps=_dev(g["eps"][s]), alpha=0.5)
        for v in ens.loss_values():
            assert abs(v - g["losses"][s]) <= 1e-4 * abs(g["losses"][s]), (s, v)
        total += g["losses"][s]
    for v in ens.epoch_total():
        assert abs(v - total) <= 1e-4 * abs(total)
    sd = ens.models[0].state_dict()
    for k, v in g.items():
        if k.startswith("param5."):
            _close(sd[k[7:]], torch.from_numpy(v), 5e-5, k)
    assert torch.equal(ens.params[1], ens.params[0]) and torch.equal(ens.exp_avg_sq[1], ens.exp_avg_sq[0])


# ------------------------------------------------------------------------------------------------ 8. launch set
def test_launch_set_does_not_depend_on_G(mw, me, monkeypatch):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    from vpc_amd import _lib
    calls = []
    real = _lib.lib()

    class Spy:  # every library entry the step calls, by name
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("vpc_miw"):
                return fn

            def run(*a):
                calls.append(name)
                return fn(*a)
            return run

    monkeypatch.setattr(me, "lib", lambda: Spy())
    want = ["vpc_miw_multi_prep", "vpc_miw_small_fwd_multi", "vpc_miw_loss_multi", "vpc_miw_small_bwd_multi",
            "vpc_miw_small_tail_multi"]
    for G in (1, 5):
        cases = EC.member_cases(EC.DRAW_SHAPE, "reg", tuple(range(G)))
        ens = me.MIWEnsembleTrainer([_model(mw, c) for c in cases], lr=1e-3)
        ens.step(_stack(cases, "x"), _stack(cases, "mask"), alpha=0.5)  # (first step: the workspaces are made)
        calls.clear()
        ens.step(_stack(cases, "x"), _stack(cases, "mask"), alpha=0.5)
        assert calls == want, (G, calls)
        assert list(ens.last_launches) == want


# ------------------------------------------------------------------------------------------------ 9. train_sweep
def test_train_sweep(mw, me, monkeypatch, tmp_path):
    import vpc_amd as vpc
    d, Ld, S = 12, 10, 20
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(192, d, generator=gen)
    mask = torch.rand(192, d, generator=gen) < 0.7
    loader = [(x[i:i + 64], mask[i:i + 64]) for i in (0, 64, 128)]
    cfgs = [dict(vae_type="reg_MIWAE1", alpha=0.5, p_missingness=30, seed=5), dict(vae_type="vanilla_MIWAE1", seed=1),
            dict(vae_type="reg_MIWAE2", alpha=0.8, p_missingness=50, seed=6), dict(vae_type="vanilla_MIWAE2", seed=2)]
    torch.manual_seed(3)
    base = [(mw.Reg_MIWAE if "reg" in c["vae_type"] else mw.MIWAE)(d, 500, 10, Ld, TP, S, 1) for c in cfgs]
    args = (30, d, 500, 10, 1, Ld, "synth", TP, "exp")
    kw = dict(max_epochs=2, device=torch.device(DEV), verbose=False, save=False)
    monkeypatch.chdir(tmp_path)
    made = []
    cls = me.MIWEnsembleTrainer
    monkeypatch.setattr(vpc.harness, "MIWEnsembleTrainer", lambda ms, **k: made.append(len(ms)) or cls(ms, **k))
    # ---- the small-batch step switched on: two ensembles of two
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    out = vpc.train_sweep((loader, None), cfgs, *args, 20, 10, models=[copy.deepcopy(m) for m in base], **kw)
    assert made == [2, 2]
    for idx in ([0, 2], [1, 3]):
        ens = cls([copy.deepcopy(base[g]).to(DEV) for g in idx], lr=0.001, seeds=[cfgs[g]["seed"] for g in idx])
        for _ in range(2):
            for xb, mb in loader:
                ens.step(xb.to(DEV), mb.to(DEV), alpha=[cfgs[g].get("alpha", 1.0) for g in idx],
                         p_missingness=[cfgs[g].get("p_missingness", 30) for g in idx])
        for k, g in enumerate(idx):
            assert torch.equal(out[g].flatten_parameters(), ens.params[k]), g
            assert not torch.equal(ens.params[k].cpu(), base[g].flatten_parameters().cpu())  # it trained
    # ---- the variable unset: what train_sweep did before, train() alone for every member
    monkeypatch.delenv("VPC_MIW_SMALL", raising=False)
    made.clear()
    out = vpc.train_sweep((loader, None), cfgs, *args, 20, 10, models=[copy.deepcopy(m) for m in base], **kw)
    assert made == []
    for g, c in enumerate(cfgs):
        solo = vpc.train((loader, None), *args, c["vae_type"], 20, 10, alpha=c.get("alpha", 1.0),
                         p_missingness=c.get("p_missingness", 30), seed=c["seed"], model=copy.deepcopy(base[g]), **kw)
        assert torch.equal(out[g].flatten_parameters(), solo.flatten_parameters()), g


# ------------------------------------------------------------------------------------------------ 10. the C entries
@pytest.mark.parametrize("bad", EC.BAD_ENTRY_CASES)
def test_c_entries_refuse_bad_arguments(mw, me, bad):
    from vpc_amd import _lib
    lb, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    G, B, S, d, Ld, rb, blocks = 2, 4, 3, 12, 10, 4, 1
    R = B
    n = me.n_params(d, Ld)
    z = torch.zeros(1 << 18, device="cuda")
    params = torch.full((G, n + 8), 0.25, device="cuda")
    before = params.clone()
    table = np.zeros(G, me.MEMBER_DTYPE)
    table["keep_prob"], table["lr"], table["alpha"] = 0.7, 1e-3, 0.5
    mem = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
    P = ptr(z)
    stride, xs, part_floats = n + 8, B * d, G * blocks * n
    prm, xp = ptr(params), P
    if bad == "d33":
        d = 33
    elif bad == "L17":
        Ld = 17
    elif bad == "short_part":
        part_floats -= 1
    elif bad == "short_stride":
        stride, xs = n - 1, (B - 1) * d  # a parameter row and a data slice, each one row short
    elif bad == "null":
        prm = xp = None
    entries = {
        "prep": lambda: lb.vpc_miw_multi_prep(xp, xs, P, xs, None, P, P, ptr(mem), G, 1, B, S, d, Ld, 0, 1 << 40, st),
        "fwd": lambda: lb.vpc_miw_small_fwd_multi(prm, stride, *[P] * 10, G, R, S, d, Ld, rb, 0, st),
        "loss": lambda: lb.vpc_miw_loss_multi(xp, xs, P, xs, None, *[P] * 6, z.numel() * 4, P, P, P, ptr(mem), G, B, S, d, Ld,
                                              0, st),
        "bwd": lambda: lb.vpc_miw_small_bwd_multi(prm, stride, *[P] * 12, part_floats, G, blocks, R, S, d, Ld, rb, 0, st),
        "tail": lambda: lb.vpc_miw_small_tail_multi(P, part_floats, G, blocks, d, Ld, P, prm, P, P, stride, ptr(mem), 0.9,
                                                    0.999, 1e-8, 1, st),
    }
    # (only the entries that must refuse are called: nothing in this test may reach a launch)
    refused = {"short_part": ("bwd", "tail")}.get(bad, tuple(entries))
    for name in refused:
        assert entries[name]() == 1, (bad, name)  # VPC_ERR_ARG
    if bad in ("d33", "L17"):
        assert me.n_params(12, 10) == 43320 and int(lb.vpc_miw_multi_workspace(G, blocks, d, Ld)) == 0
    torch.cuda.synchronize()
    assert torch.equal(params, before) and not bool(z.any())  # nothing was launched: parameters and scratch untouched


def test_step_refuses_before_it_counts(mw, me, monkeypatch):
    """A step that cannot run raises before it draws, counts or launches: rng_offset, step count and parameters stay."""
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    cases = EC.member_cases(EC.DRAW_SHAPE, "reg", (0, 1))
    ens = me.MIWEnsembleTrainer([_model(mw, c) for c in cases], lr=1e-3)
    before = ens.params.clone()
    x, m = _stack(cases, "x"), _stack(cases, "mask")
    import vpc_amd
    with pytest.raises(vpc_amd.VpcError, match="x and mask agree"):
        ens.step(x, m[:, :3])
    with pytest.raises(vpc_amd.VpcError, match="inject all"):
        ens.step(x, m, eps=_stack(cases, "eps"))
    monkeypatch.setattr(me, "PART_MAX_FLOATS", 1000)
    with pytest.raises(vpc_amd.VpcError, match="partial buffer"):
        ens.step(x, m)
    assert ens.rng_offset == 0 and ens.step_count == 0 and torch.equal(ens.params, before)
