"""The small-batch step of MIWTrainer (csrc/vpc_miw_small.hip: miw_small_fwd -> the loss launches -> miw_small_bwd ->
miw_small_tail) on the GPU:
  1. edge shapes (tests/miwae_small_cases.py) against the float64 oracle with the step's own ReLU gates, the check of
     tests/test_miwae_kernels_gpu.py::test_trainer_step_and_api_vs_oracle: loss 1e-4, each of the twelve gradients 2e-4 of
     its max;
  2. the small path against the launch chain (VPC_MIW_SMALL=0) on the same inputs at the wine shape (64, 20, 12, 10):
     injected draws (flat gradient and out8 2e-5), device draws (mask_p, eps, rng_offset bit-equal), five steps (losses
     1e-4, parameters 5e-5 of their max);
  3. the reference's recorded vectors and trajectories through the small path;
  4. repeatability and the workspace rule across a batch-size change;
  5. the fall-back to the chain and the argument guards of the C entries;
  6. more row blocks than compute units (the persistent walk of the backward kernel) and RB = 4, against the chain."""
import math

import numpy as np
import pytest
import torch

import miwae_cases as C
import miwae_oracle as O
import miwae_small_cases as SC
from conftest import load_golden

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 1}
WINE = (64, 20, 12, 10)
ALL_ROWS = str(1 << 20)  # a VPC_MIW_SMALL above every shape of this file


@pytest.fixture(scope="module")
def mw():
    import vpc_amd
    from vpc_amd import miwae
    return miwae


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


def _inputs(c):
    return _dev(c["x"]), _dev(c["mask"]), _dev(c["mask_p"]), _dev(c["eps"])


def _step_gates(tr, c):
    """The ReLU gates the step took, per pass and chain, keyed as tests/miwae_oracle.run takes them."""
    B, BS = c["B"], c["B"] * c["S"]
    g = lambda a, b, r: {0: (a[r] > 0).cpu(), 2: (b[r] > 0).cpu()}
    gates = {"enc_q": g(tr.h1, tr.h2, slice(0, B)), "dec_q": g(tr.g1, tr.g2, slice(0, BS))}
    if c["reg"]:
        gates.update({"enc_p": g(tr.h1, tr.h2, slice(B, None)), "dec_p": g(tr.g1, tr.g2, slice(BS, None))})
    return gates


# ------------------------------------------------------------------------------------------------ 1. edge shapes
@pytest.mark.parametrize("rb", [1, 2, 4])
@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("shape", SC.EDGE_SHAPES)
def test_edge_shapes_vs_oracle(mw, monkeypatch, shape, kind, rb):
    """Every workgroup shape, forced (the trainer's own choice at these sizes is rb = 1; its rule runs in
    test_more_row_blocks_than_compute_units)."""
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    c = SC.edge_case(shape, kind)
    x, m, mp, eps = _inputs(c)
    model = _model(mw, c)
    tr = mw.MIWTrainer(model, lr=1e-3)
    tr.small_rb = rb
    tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    assert tr.last_path == "small"
    p, xo, mo, mpo, epo = C.oracle_inputs(c)
    stats = O.new_gate_stats()
    lo = O.run(p, xo, mo, mpo, epo, C.ALPHA, gates=_step_gates(tr, c), stats=stats)[0]
    ref = dict(zip(O.KEYS, torch.autograd.grad(lo, [p[k] for k in O.KEYS])))
    print(f"{shape} {kind}: {stats['in_band']} of {stats['units']} units inside the kink band, "
          f"{stats['mismatch_outside']} gate mismatches outside it")
    assert stats["in_band"] <= C.band_limit(stats["units"])
    assert stats["mismatch_outside"] == 0
    print("loss", tr.loss_value(), lo.item())
    assert abs(tr.loss_value() - lo.item()) <= 1e-4 * abs(lo.item()), (tr.loss_value(), lo.item())
    for k, prm in model.named_parameters():
        lo_ptr, hi_ptr = tr.grad.data_ptr(), tr.grad.data_ptr() + 4 * tr.grad.numel()
        assert lo_ptr <= prm.grad.data_ptr() and prm.grad.data_ptr() + 4 * prm.grad.numel() <= hi_ptr
        _close(prm.grad, ref[k], 2e-4, (shape, kind, k))


# ------------------------------------------------------------------------------------------------ 2. small path vs chain
def _two_trainers(mw, c, **kw):
    return [mw.MIWTrainer(_model(mw, c), lr=1e-3, **kw) for _ in range(2)]


def _both(monkeypatch, trs, fn):
    """fn(trainer) on the small path (trs[0]), then on the chain (trs[1])."""
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    fn(trs[0])
    assert trs[0].last_path == "small"
    monkeypatch.setenv("VPC_MIW_SMALL", "0")
    fn(trs[1])
    assert trs[1].last_path == "chain"


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_paths_agree_on_injected_draws(mw, monkeypatch, kind):
    c = C.trainer_case(WINE, kind)
    x, m, mp, eps = _inputs(c)
    trs = _two_trainers(mw, c)
    _both(monkeypatch, trs, lambda tr: tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA))
    _close(trs[0].grad, trs[1].grad, 2e-5, "flat gradient, small vs chain")
    a, b = trs[0].out8.cpu(), trs[1].out8.cpu()
    for i in range(8):  # (MIWAE's Reg-only entries are the literal 0.0 on any path: no pass, no term)
        assert abs(a[i] - b[i]) <= 2e-5 * abs(b[i]), (i, float(a[i]), float(b[i]))
    assert abs(trs[0].loss_value() - trs[1].loss_value()) <= 2e-5 * abs(trs[1].loss_value())


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_paths_draw_the_same_bits(mw, monkeypatch, kind):
    c = C.trainer_case(WINE, kind)
    x, m, _, _ = _inputs(c)
    trs = _two_trainers(mw, c, seed=11)
    _both(monkeypatch, trs, lambda tr: tr.step(x, m.bool(), alpha=0.5, p_missingness=30))
    assert trs[0].rng_offset == trs[1].rng_offset > 0
    assert torch.equal(trs[0].eps, trs[1].eps)
    if kind == "reg":
        assert torch.equal(trs[0].mask_p, trs[1].mask_p)
        assert 0 < float(trs[0].mask_p.sum()) < float(m.sum())


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_paths_agree_over_five_steps(mw, monkeypatch, kind):
    c = C.trainer_case(WINE, kind)
    x, m, _, _ = _inputs(c)
    trs = _two_trainers(mw, c, seed=5)
    losses = {}

    def run(tr):
        ls = losses.setdefault(id(tr), [])
        for _ in range(5):
            tr.step(x, m.bool(), alpha=0.5, p_missingness=30)
            ls.append(tr.loss_value())

    _both(monkeypatch, trs, run)
    for a, b in zip(losses[id(trs[0])], losses[id(trs[1])]):
        assert abs(a - b) <= 1e-4 * abs(b), (a, b)
    _close(trs[0].model._flat, trs[1].model._flat, 5e-5, "parameters after five steps, small vs chain")
    assert trs[0].step_count == trs[1].step_count == 5
    assert abs(trs[0].epoch_total() - trs[1].epoch_total()) <= 1e-4 * abs(trs[1].epoch_total())


# (kind, B, S, rb): more row blocks than compute units, so a workgroup of the persistent backward walks several blocks with
# its accumulators, operand hand-over and re-staging carried across them.  rb = None is the trainer's own rule (RB = 4 here).
MANY_BLOCKS = [
    ("reg", 300, 2, 1),      # 600 blocks of one row
    ("van", 601, 2, 2),      # 301 blocks, the last with one live row
    ("reg", 1100, 1, None),  # R = 2 200: RB = 4, 550 blocks, S = 1
    ("van", 1101, 1, None),  # R = 1 101: RB = 4, 276 blocks, the last with one live row
]


@pytest.mark.parametrize("kind,B,S,rb", MANY_BLOCKS)
def test_more_row_blocks_than_compute_units(mw, monkeypatch, kind, B, S, rb):
    """Against the chain on the same inputs: flat gradient and loss at the bounds of test_paths_agree_on_injected_draws,
    each of the twelve gradients 2e-4 of its own max, the updated parameters 5e-5."""
    from vpc_amd import _lib
    c = C.model_case(B, S, 12, 10, kind == "reg", 7)
    x, m, mp, eps = _inputs(c)
    trs = _two_trainers(mw, c)
    trs[0].small_rb = rb
    R = (2 if kind == "reg" else 1) * B
    RB = rb if rb else mw.small_rows_per_workgroup(R, S)
    cus = _lib.max_blocks() // 2
    assert RB == (rb or 4) and -(-R // RB) > cus, (R, RB, cus)
    assert (R % RB != 0) == (kind == "van")  # the vanilla cases end on a ragged block
    _both(monkeypatch, trs, lambda tr: tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA))
    _close(trs[0].grad, trs[1].grad, 2e-5, "flat gradient, small vs chain")
    assert abs(trs[0].loss_value() - trs[1].loss_value()) <= 2e-5 * abs(trs[1].loss_value())
    for (k, pa), pb in zip(trs[0].model.named_parameters(), trs[1].model.parameters()):  # each tensor on its own max, the
        _close(pa.grad, pb.grad, 2e-4, ("gradient", k))                                   # project's per-gradient bound
    _close(trs[0].model._flat, trs[1].model._flat, 5e-5, "parameters after the step")


# ------------------------------------------------------------------------------------------------ 3. reference goldens
def _load_model(mw, g, cls, prefix="param."):
    torch.manual_seed(0)
    model = cls(g["x"].shape[1], 500, 10, int(g["L"]), TP, int(g["S"]), 1)
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(prefix)})
    return model.cuda()


@pytest.mark.parametrize("name", ["miwae_reg_d14", "miwae_van_d14"])
def test_step_vs_reference(mw, monkeypatch, name):
    """One step from the recorded parameters: the loss and every gradient of the reference."""
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    g = load_golden(name + ".npz")
    reg = "reg" in name
    x, m = _dev(g["x"]), _dev(g["mask"])
    mp = _dev(g["mask_p"]) if reg else None
    eps = _dev(g["eps"])
    for alpha, lk, gk in ([(a, f"loss.a{a}", f"a{a}") for a in (1.0, 0.5, 0.0)] if reg else [(0.0, "loss", "v")]):
        model = _load_model(mw, g, mw.Reg_MIWAE if reg else mw.MIWAE)
        tr = mw.MIWTrainer(model, lr=1e-3)
        tr.step(x, m, mask_p=mp, eps=eps, alpha=alpha)
        assert tr.last_path == "small"
        assert abs(tr.loss_value() - g[lk]) <= 1e-4 * abs(g[lk]), (alpha, tr.loss_value(), float(g[lk]))
        for k, p in model.named_parameters():
            _close(p.grad, torch.from_numpy(g[f"grad.{gk}.{k}"]), 2e-4, (alpha, k))


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_trajectory_vs_reference(mw, monkeypatch, kind):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    g = load_golden(f"miwae_traj_{kind}_d14.npz")
    model = _load_model(mw, g, mw.Reg_MIWAE if kind == "reg" else mw.MIWAE, "param0.")
    tr = mw.MIWTrainer(model, lr=1e-3)
    x, m = _dev(g["x"]), _dev(g["mask"]).bool()
    total = 0.0
    for s in range(len(g["losses"])):
        tr.step(x, m, mask_p=_dev(g["mask_p"][s]) if kind == "reg" else None, eps=_dev(g["eps"][s]), alpha=0.5)
        assert tr.last_path == "small"
        assert abs(tr.loss_value() - g["losses"][s]) <= 1e-4 * abs(g["losses"][s]), (s, tr.loss_value())
        total += g["losses"][s]
    assert abs(tr.epoch_total() - total) <= 1e-4 * abs(total)
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith("param5."):
            _close(sd[k[7:]], torch.from_numpy(v), 5e-5, k)


# ------------------------------------------------------------------------------------------------ 4. repeatability
@pytest.mark.parametrize("kind", ["reg", "van"])
def test_device_draw_runs_repeat_bit_for_bit(mw, monkeypatch, kind):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    c = C.trainer_case(WINE, kind)
    x, m, _, _ = _inputs(c)
    runs = []
    for _ in range(2):
        tr = mw.MIWTrainer(_model(mw, c), lr=3e-3, seed=11)
        losses = []
        for _s in range(8):
            tr.step(x, m.bool(), alpha=0.5, p_missingness=30)
            assert tr.last_path == "small"
            losses.append(tr.loss_value())
        runs.append((losses, tr.model._flat.clone()))
    assert runs[0][0] == runs[1][0] and all(math.isfinite(v) for v in runs[0][0])
    assert torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_workspace_across_batch_sizes(mw, monkeypatch, kind):
    """Two steps at B = 37, then one at B = 5 on one trainer: bit-equal to a fresh trainer stepped from the same parameters
    and Adam state (d = 12, S = 5)."""
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    big = C.model_case(37, 5, 12, 10, kind == "reg", 12)
    small = C.model_case(5, 5, 12, 10, kind == "reg", 13)
    model = _model(mw, big)
    tr = mw.MIWTrainer(model, lr=1e-3)
    x, m, mp, eps = _inputs(big)
    tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    tr.step(x, m, mask_p=mp, eps=eps.flip(2), alpha=C.ALPHA)
    fresh = _model(mw, big)
    fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
    tr2 = mw.MIWTrainer(fresh, lr=1e-3)
    tr2.exp_avg.copy_(tr.exp_avg)
    tr2.exp_avg_sq.copy_(tr.exp_avg_sq)
    tr2.step_count, tr2.rng_offset = tr.step_count, tr.rng_offset
    x, m, mp, eps = _inputs(small)
    tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    tr2.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    assert tr.last_path == tr2.last_path == "small"
    assert tr.loss_value() == tr2.loss_value() and math.isfinite(tr.loss_value())
    assert torch.equal(tr.grad, tr2.grad)
    assert torch.equal(model._flat, fresh._flat)
    assert torch.equal(tr.exp_avg, tr2.exp_avg) and torch.equal(tr.exp_avg_sq, tr2.exp_avg_sq)


# ------------------------------------------------------------------------------------------------ 5. fall-back and guards
def test_route_predicate(mw):
    r = mw.small_step_route
    assert r(12, 10, 64, 20, 2, 2560) and not r(12, 10, 64, 20, 2, 2559) and not r(12, 10, 64, 20, 2, 0)
    assert r(32, 16, 1, 1, 1, 1) and not r(33, 16, 1, 1, 1, 100) and not r(32, 17, 1, 1, 1, 100)


def test_without_the_variable_the_step_is_the_chain(mw, monkeypatch):
    monkeypatch.delenv("VPC_MIW_SMALL", raising=False)
    assert mw.small_max_rows() == 0 and mw.SMALL_ROWS_MEASURED == 163840
    c = C.model_case(6, 3, 12, 10, True, 3)
    tr = mw.MIWTrainer(_model(mw, c), lr=1e-3)
    x, m, mp, eps = _inputs(c)
    tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    assert tr.last_path == "chain"
    monkeypatch.setenv("VPC_MIW_SMALL", str(mw.SMALL_ROWS_MEASURED))
    tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    assert tr.last_path == "small"


@pytest.mark.parametrize("d,Ld", [(33, 10), (12, 17)])
def test_wide_shapes_keep_the_chain(mw, monkeypatch, d, Ld):
    monkeypatch.setenv("VPC_MIW_SMALL", ALL_ROWS)
    c = C.model_case(6, 3, d, Ld, True, 3)
    tr = mw.MIWTrainer(_model(mw, c), lr=1e-3)
    x, m, mp, eps = _inputs(c)
    tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
    assert tr.last_path == "chain" and math.isfinite(tr.loss_value())


def test_path_switches_on_one_trainer(mw, monkeypatch):
    """small -> chain (a batch over the row limit) -> small on one trainer equals the same three steps on the chain within
    the bounds of the five-step test."""
    c = C.model_case(8, 5, 12, 10, True, 4)
    big = C.model_case(9, 5, 12, 10, True, 5)
    trs = _two_trainers(mw, c)
    ins, inb = _inputs(c), _inputs(big)
    limit = str(2 * 8 * 5)
    paths = []
    for tr, env in ((trs[0], limit), (trs[1], "0")):
        monkeypatch.setenv("VPC_MIW_SMALL", env)
        for x, m, mp, eps in (ins, inb, ins):
            tr.step(x, m, mask_p=mp, eps=eps, alpha=C.ALPHA)
            paths.append(tr.last_path)
    assert paths == ["small", "chain", "small", "chain", "chain", "chain"]
    assert abs(trs[0].loss_value() - trs[1].loss_value()) <= 1e-4 * abs(trs[1].loss_value())
    _close(trs[0].model._flat, trs[1].model._flat, 5e-5, "parameters after small, chain, small")


def test_c_entries_refuse_bad_arguments(mw):
    import vpc_amd
    z = torch.zeros(1 << 16, device="cuda")
    ok = dict(R=4, S=3, d=12, Ld=10, RB=4)
    bad = [dict(ok, d=33), dict(ok, d=0), dict(ok, Ld=17), dict(ok, Ld=0), dict(ok, RB=5), dict(ok, RB=0), dict(ok, S=0),
           dict(ok, R=0)]
    for kw in bad:
        with pytest.raises(vpc_amd.VpcError):
            mw.miw_small_fwd(*[z] * 11, kw["R"], kw["S"], kw["d"], kw["Ld"], kw["RB"])
        with pytest.raises(vpc_amd.VpcError):
            mw.miw_small_bwd(*[z] * 13, kw["R"], kw["S"], kw["d"], kw["Ld"], kw["RB"])
    for kw in bad[:6]:
        with pytest.raises(vpc_amd.VpcError):
            mw.miw_small_tail(z, kw["R"], kw["RB"], kw["d"], kw["Ld"], z, z, z, z, 1e-3, 0.9, 0.999, 1e-8, 1)
    # a NULL pointer, a short partial buffer, step 0
    with pytest.raises(vpc_amd.VpcError):
        mw.miw_small_fwd(z, None, *[z] * 9, 4, 3, 12, 10, 4)
    with pytest.raises(vpc_amd.VpcError):
        mw.miw_small_bwd(*[z] * 12, z[:100], 4, 3, 12, 10, 4)
    with pytest.raises(vpc_amd.VpcError):
        mw.miw_small_tail(z[:100], 4, 4, 12, 10, z, z, z, z, 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(vpc_amd.VpcError):
        mw.miw_small_tail(z, 4, 4, 12, 10, z, z, z, z, 1e-3, 0.9, 0.999, 1e-8, 0)
    assert mw.miw_small_workspace(33, 10) == 0 and mw.miw_small_workspace(12, 17) == 0
    assert mw.miw_small_workspace(12, 10) >= 45000
    torch.cuda.synchronize()
    assert not bool(z.any())
