"""ensemble.py on the host: stacking G models into one [G, n] buffer, the validation EnsembleTrainer does before anything
touches the device, and the per-member coefficient table.  CPU only: models are built, nothing is launched."""
import numpy as np
import pytest
import torch

import vpc_amd as vpc
from vpc_amd import ensemble as E
from vpc_amd.fused import loss_coefficients

TP = {"batch_size": 8, "patience": 1}
L = 10


def reg(d=14, rt="kl_reg", Ld=L):
    return vpc.Reg_VAE(d, 500, 10, Ld, TP, "e", rt)


def van(d=14):
    return vpc.vanilla_VAE(d, 500, 10, L, TP, "e")


# ----------------------------------------------------------------------------------------------- stacking
def test_stack_aliases_rows_in_table_order():
    ms = [reg() for _ in range(3)]
    before = [{k: v.clone() for k, v in m.state_dict().items()} for m in ms]
    stack = E.stack_models(ms)
    n = sum(p.numel() for p in ms[0].trainable())
    assert stack.shape == (3, n)
    for g, m in enumerate(ms):
        off = 0
        for p in m.trainable():  # every trainable tensor is a view of row g, in table order
            assert p.data_ptr() == stack[g].data_ptr() + 4 * off
            assert p.is_contiguous()
            off += p.numel()
        assert off == n
        flat = m.flatten_parameters()  # the fast path: row g itself, nothing reallocated
        assert flat.data_ptr() == stack[g].data_ptr() and flat.numel() == n
        assert m.flatten_parameters().data_ptr() == flat.data_ptr()
        sd = m.state_dict()
        assert list(sd) == list(before[g])
        for k, v in sd.items():  # values unchanged by stacking
            assert torch.equal(v, before[g][k]), k
    assert E.stack_models(ms) is stack  # idempotent


def test_stack_rows_are_independent_and_inplace_load_keeps_aliasing():
    ms = [van() for _ in range(2)]
    stack = E.stack_models(ms)
    row1 = stack[1].clone()
    new = {k: torch.full_like(v, 0.25) for k, v in ms[0].state_dict().items()}
    ms[0].load_state_dict(new)  # in place: the tensors stay views of row 0
    assert torch.equal(stack[1], row1)
    assert ms[0].flatten_parameters().data_ptr() == stack[0].data_ptr()
    assert torch.all(stack[0] == 0.25)
    with torch.no_grad():
        stack[1].zero_()
    assert all(torch.all(p == 0) for p in ms[1].trainable())
    assert torch.all(stack[0] == 0.25)


# ----------------------------------------------------------------------------------------------- validation
@pytest.mark.parametrize("models,exc", [
    (lambda: [reg(), van()], TypeError),                                     # mixed classes
    (lambda: [reg(14), reg(16)], vpc.VpcError),                              # obs_dim
    (lambda: [reg(Ld=10), reg(Ld=8)], vpc.VpcError),                         # latent_dim
    (lambda: [reg(rt="kl_reg"), reg(rt="ml_reg")], vpc.VpcError),            # reg_type
    (lambda: [vpc.Reg_VAE_mask(14, 500, 10, L, TP, "e", "kl_reg")] * 2, vpc.VpcError),  # mask-augmented
    (lambda: [vpc.vanilla_VAE(200, 500, 10, L, TP, "e")] * 2, vpc.VpcError),             # wide
    (lambda: [vpc.MIWAE(14, 500, 10, L, TP, 1, 1)], TypeError),              # another family
    (lambda: [], vpc.VpcError),
])
def test_members_are_validated_before_any_device_call(models, exc):
    # (CPU models: a device call would raise VpcError("... got a CPU tensor") instead of the error asked for here - and the
    # TypeError cases could not be mistaken for it)
    with pytest.raises(exc) as ei:
        E.EnsembleTrainer(models())
    assert "CPU tensor" not in str(ei.value)


def test_world_size_and_per_member_lengths():
    ms = [reg(), reg()]
    with pytest.raises(vpc.VpcError, match="single-process"):
        E.EnsembleTrainer(ms, world_size=2)
    with pytest.raises(vpc.VpcError, match="lr"):
        E.EnsembleTrainer(ms, lr=[1e-3, 1e-3, 1e-3])
    with pytest.raises(vpc.VpcError, match="seeds"):
        E.EnsembleTrainer(ms, seeds=[1])
    t = E.MemberTable(ms)
    for kw in (dict(alpha=[1.0]), dict(beta=[1.0, 1.0, 1.0]), dict(p_missingness=[30])):
        with pytest.raises(vpc.VpcError):
            t.update(**kw)
    # nothing was stacked or moved by the refused constructions
    assert all("_stack" not in m.__dict__ for m in ms)


# ----------------------------------------------------------------------------------------------- coefficient table
def _check_rows(t, ms, epoch, alphas, betas, annealing, pms, lrs, seeds):
    assert t.rows.dtype.itemsize == 64
    for g, m in enumerate(ms):
        co = loss_coefficients(m, epoch, alphas[g], betas[g], annealing)
        r = t.rows[g]
        f = np.float32
        assert r["cA"][0] == f(co.cA[0]) and r["cE"][0] == f(co.cE[0])
        assert r["cA"][1] == f(co.cA[1]) and r["cE"][1] == f(co.cE[1])
        for k in ("bq", "bp", "cr", "wml"):
            assert r[k] == f(getattr(co, k)), k
        assert r["keep_prob"] == f(1.0 - pms[g] / 100.0)
        assert r["lr"] == f(lrs[g]) and int(r["seed"]) == seeds[g]
        assert int(r["use_maskB"]) == int(not isinstance(m, vpc.vanilla_VAE) and co.cE[0] != 0.0)


@pytest.mark.parametrize("kind,epoch", [("kl_reg", 3), ("ml_reg", 1400), ("vanilla", 5)])
def test_member_table_rows_equal_loss_coefficients(kind, epoch):
    ms = [van() if kind == "vanilla" else reg(rt=kind) for _ in range(3)]
    alphas, betas, pms, lrs, seeds = (1.0, 0.5, 0.8), (1.0, 0.7, 0.9), (30, 50, 10), (1e-3, 1e-3, 3e-4), (1, 2, 2 ** 40 + 3)
    t = E.MemberTable(ms, lrs, seeds)
    for annealing in (False, True):
        t.update(epoch, alphas, betas, annealing, pms)
        _check_rows(t, ms, epoch, alphas, betas, annealing, pms, lrs, seeds)
        assert t.need_ml == (kind == "ml_reg")


def test_member_table_is_rebuilt_only_when_an_input_changes():
    ms = [reg() for _ in range(2)]
    t = E.MemberTable(ms, 1e-3, None)
    assert [int(s) for s in t.rows["seed"]] == [0, 1]
    assert t.update(1, [1.0, 0.5], 1.0, False, 30) is True and (t.builds, t.version) == (1, 1)
    assert t.update(1, [1.0, 0.5], 1.0, False, 30) is False and (t.builds, t.version) == (1, 1)
    assert t.update(1, (1.0, 0.5), 1.0, False, (30, 30)) is False and t.builds == 1   # the same values, spelled differently
    # a new epoch without annealing: rebuilt (an input changed), but no row changed - nothing to upload
    assert t.update(2, [1.0, 0.5], 1.0, False, 30) is False and (t.builds, t.version) == (2, 1)
    # with annealing every epoch changes bq / bp
    assert t.update(2, [1.0, 0.5], 1.0, True, 30) is True and (t.builds, t.version) == (3, 2)
    assert t.update(3, [1.0, 0.5], 1.0, True, 30) is True and (t.builds, t.version) == (4, 3)
    assert t.update(3, [1.0, 0.6], 1.0, True, 30) is True and t.version == 4
    assert t.update(3, [1.0, 0.6], 1.0, True, [30, 40]) is True and t.version == 5


def test_member_table_refuses_members_that_disagree_on_the_ml_term():
    t = E.MemberTable([reg(rt="ml_reg") for _ in range(2)])
    with pytest.raises(vpc.VpcError, match="ml_reg"):
        t.update(1400, [0.5, 0.0])
