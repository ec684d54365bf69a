"""The rules the ensemble host code states once (ensemble.py, harness.py, trainer.py, ops.py): the member-stride slots against
include/vpc.h, the shared-or-per-member shape check, the padded row width, the launch count of a chunked forward and the
lock-step walk over per-member loaders with what train_sweep and _gather_passes make of a mismatch.  CPU only: nothing is
launched (train_sweep's trainer is stubbed)."""
import os
import re
import types

import pytest
import torch

import vpc_amd as vpc
from vpc_amd import ensemble as E
from vpc_amd import harness as H
from vpc_amd import ops
from vpc_amd.trainer import padded_width

TP = {"batch_size": 8, "patience": 1}
L = 10


@pytest.mark.parametrize("prefix", ["MS", "RM"])
def test_stride_slots_mirror_the_header(prefix):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vpc.h")).read()
    body = re.search(r"enum\s*\{\s*(VPC_%s_X\s*=\s*0[^}]*)\}" % prefix, text).group(1)
    names = [n.split("=")[0].strip() for n in body.split(",")]
    assert names[0] == f"VPC_{prefix}_X" and names[-1] == f"VPC_{prefix}_COUNT" and len(names) == 10
    for value, name in enumerate(names):  # (an enum that starts at 0 and counts on)
        assert getattr(ops, name[len("VPC_"):]) == value, name
    assert ops.MS_PART == ops.MS_LOSS  # the evaluation's per-tile sums travel in the loss slot (include/vpc.h)
    assert ops.stride_vector(ops.MS_COUNT, {ops.MS_IMG: 64, ops.MS_PART: 5}) == [0, 0, 0, 0, 64, 0, 0, 5, 0]


def test_shared_or_per_member():
    G, tail = 3, (5, 4)
    assert E._shared_or_per_member(torch.zeros(5, 4), "x", G, tail) == 0
    assert E._shared_or_per_member(torch.zeros(3, 5, 4), "x", G, tail) == 20
    assert E._shared_or_per_member((3, 5, 4), "x", G, tail) == 20 and E._shared_or_per_member((5, 4), "x", G, tail) == 0
    assert E._shared_or_per_member(torch.zeros(3, 7, 4), "x", G, (None, 4)) == 28  # None: any number of rows
    # the member axis is a matter of the shape: a view expanded over the members (stride 0) is per member all the same
    assert E._shared_or_per_member(torch.zeros(5, 4).expand(3, 5, 4), "x", G, tail) == 20
    for shape in ((2, 5, 4), (5, 3), (1, 3, 5, 4), (4,)):
        with pytest.raises(vpc.VpcError, match=r"eps_q: expected \[5, 4\] or \[3, 5, 4\], got") as ei:
            E._shared_or_per_member(torch.zeros(*shape), "eps_q", G, tail)
        assert str(shape) in str(ei.value)


@pytest.mark.parametrize("G, calls", [(3, 5), (6, 2)])  # (fewer members than calls, and more)
def test_injected_eps_planes(G, calls):
    """EnsembleEvaluator._draws on the host: per member and call the plane handed to a forward launch is that member's eps of
    that call, zero-padded to LP columns, whether eps is shared, per member, or a shared eps expanded over the members without
    a copy (member stride 0, the member axis still there)."""
    R, Ld, LP = 4, 3, E.LP
    ev = types.SimpleNamespace(dev=torch.device("cpu"), lay=types.SimpleNamespace(L=Ld), rng_offset=7)
    shared = torch.randn(calls, R, Ld, generator=torch.Generator().manual_seed(0))
    per = torch.randn(G, calls, R, Ld, generator=torch.Generator().manual_seed(1))

    def planes(eps):  # -> [G, calls, R, LP] as the kernel of call c reads member g: plane c + g * member stride
        draws, stride = E.EnsembleEvaluator._draws(ev, eps, R, calls)
        assert len(draws) == calls and all(off == 0 for off, _ in draws) and ev.rng_offset == 7  # no counter is used
        assert all(p.shape == (R, LP) and p.is_contiguous() for _, p in draws)
        return torch.stack([torch.stack([p.as_strided((R, LP), (LP, 1), p.storage_offset() + g * stride) for _, p in draws])
                            for g in range(G)])

    want = torch.zeros(G, calls, R, LP)
    want[..., :Ld] = shared
    assert torch.equal(planes(shared), want)
    assert torch.equal(planes(shared.expand(G, calls, R, Ld)), want)
    want[..., :Ld] = per
    assert torch.equal(planes(per), want)
    assert torch.equal(planes(per.transpose(0, 1).contiguous().transpose(0, 1)), want)  # (any strides of the input)
    draws, stride = E.EnsembleEvaluator._draws(ev, None, R, calls)
    assert [d[1] for d in draws] == [None] * calls and stride == 0
    assert ([d[0] for d in draws], ev.rng_offset) == E.forward_draw_offsets(7, R, calls)


@pytest.mark.parametrize("d", [1, 4, 5, 12, 13, 128])
def test_padded_width(d):
    assert padded_width(d) == (d if d % 4 == 0 else 4 * ((d + 3) // 4))
    assert padded_width(d) % 4 == 0 and 0 <= padded_width(d) - d < 4
    assert padded_width(d, mask_augm=True) == d


def test_forward_launches():
    assert E.forward_launches(10, 4, 0) == 1
    assert E.forward_launches(10, 4, 8) == 5
    assert E.forward_launches(10, 4, 1) == 10


# ----------------------------------------------------------------------------------------------- lock-step loaders
def _loader(sizes, d=14, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, d, generator=g), torch.rand(n, d, generator=g) < 0.7) for n in sizes]


def test_lock_step():
    a, b = _loader([16, 16, 7]), _loader([16, 16, 7], seed=1)
    steps = list(H._lock_step([a, b], lambda bt: bt[0].shape))
    assert len(steps) == 3 and all(s[0] is a[i] and s[1] is b[i] for i, s in enumerate(steps))
    assert [s[0] for s in H._lock_step([a], lambda bt: bt[0].shape)] == a  # one loader: its batches, one by one
    seen = []
    with pytest.raises(vpc.VpcError, match="same number of batches"):
        for s in H._lock_step([a, b[:2]], lambda bt: bt[0].shape):
            seen.append(s)
    assert len(seen) == 2  # the steps both loaders have are yielded first
    with pytest.raises(vpc.VpcError, match="equal batch shapes"):
        list(H._lock_step([a, _loader([16, 7, 16])], lambda bt: bt[0].shape))


def test_gather_passes_gives_none_on_a_mismatch():
    a, dev = _loader([16, 16, 7]), torch.device("cpu")
    x, mk, ranges = H._gather_passes([a, _loader([16, 16, 7], seed=1)], 2, 14, dev)
    assert tuple(x.shape) == (2, 78, 14) and mk.shape == x.shape
    assert ranges == [[(0, 16), (16, 32), (32, 39)], [(39, 55), (55, 71), (71, 78)]]
    assert H._gather_passes([a, a[:2]], 2, 14, dev) is None
    assert H._gather_passes([a, _loader([16, 7, 16])], 2, 14, dev) is None
    assert H._gather_passes([[]], 2, 14, dev) is None  # a loader without a batch


def test_train_sweep_refuses_loaders_that_differ(monkeypatch):
    steps = []

    class StubTrainer:
        def __init__(self, models, lr=None, seeds=None):
            self.G = len(models)

        def step(self, x, mask, **kw):
            steps.append((tuple(x.shape), tuple(mask.shape)))

        def epoch_total(self):
            return [0.0] * self.G

    monkeypatch.setattr(H, "EnsembleTrainer", StubTrainer)
    cfgs = [dict(vae_type="reg_vae1", seed=1), dict(vae_type="reg_vae1", alpha=0.5, seed=2)]
    a = _loader([16, 16, 7])

    def sweep(other):
        ms = [vpc.Reg_VAE(14, 500, 10, L, TP, "e", "kl_reg") for _ in cfgs]
        return vpc.train_sweep(None, cfgs, 30, 14, 500, 10, 1, L, "synth", TP, "e", 20, 10, max_epochs=1,
                               device=torch.device("cpu"), reg_type="kl_reg", verbose=False, save=False, models=ms,
                               loaders=[(a, None), (other, None)])

    assert len(sweep(list(a))) == 2
    assert steps == [((2, 16, 14),) * 2, ((2, 16, 14),) * 2, ((2, 7, 14),) * 2]  # one step per batch, members stacked
    with pytest.raises(vpc.VpcError, match="per-member loaders must have the same number of batches"):
        sweep(a[:2])
    with pytest.raises(vpc.VpcError, match="per-member loaders must yield equal batch shapes at every step"):
        sweep([a[0], a[2], a[1]])
