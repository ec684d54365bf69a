"""The host rules of the MIWAE ensemble step (vpc_amd/miw_ensemble.py) that need no GPU: what an ensemble may hold (raised
before anything touches the device), how harness.train_sweep groups MIWAE-path members with VPC_MIW_SMALL set and unset, the
size rule of the partial buffer and the (rb, blocks_per_member) default rule."""
import pytest
import torch

import miw_ensemble_cases as EC
import vpc_amd as vpc
from vpc_amd import harness
from vpc_amd import miw_ensemble as E
from vpc_amd import miwae

TP = {"batch_size": 64, "patience": 1}


def _m(cls=None, d=12, Ld=10, S=20):
    return (cls or miwae.Reg_MIWAE)(d, 500, 10, Ld, TP, S, 1)  # on the CPU: validation comes before the device


# ------------------------------------------------------------------------------------------------ validation
def test_validation_comes_first_and_says_why():
    with pytest.raises(TypeError, match="members of one ensemble share a class: Reg_MIWAE and MIWAE"):
        E.MIWEnsembleTrainer([_m(), _m(miwae.MIWAE)])
    with pytest.raises(vpc.VpcError, match=r"share \(obs_dim, latent_dim, num_samples\): \(12, 10, 20\) and \(12, 10, 5\)"):
        E.MIWEnsembleTrainer([_m(), _m(S=5)])
    with pytest.raises(vpc.VpcError, match=r"share \(obs_dim, latent_dim, num_samples\)"):
        E.MIWEnsembleTrainer([_m(), _m(d=13)])
    with pytest.raises(vpc.VpcError, match="single-process"):
        E.MIWEnsembleTrainer([_m(), _m()], world_size=2)
    with pytest.raises(vpc.VpcError, match="obs_dim <= 32 and latent_dim <= 16"):
        E.MIWEnsembleTrainer([_m(d=33), _m(d=33)])
    with pytest.raises(vpc.VpcError, match="obs_dim <= 32 and latent_dim <= 16"):
        E.MIWEnsembleTrainer([_m(Ld=17)])
    with pytest.raises(vpc.VpcError, match="at least one member"):
        E.MIWEnsembleTrainer([])
    with pytest.raises(TypeError, match="supports MIWAE and Reg_MIWAE members, got Linear"):
        E.MIWEnsembleTrainer([torch.nn.Linear(2, 2)])
    with pytest.raises(vpc.VpcError, match="rb = 3"):
        E.MIWEnsembleTrainer([_m()], rb=3)
    with pytest.raises(vpc.VpcError, match="blocks_per_member = 0"):
        E.MIWEnsembleTrainer([_m()], blocks_per_member=0)
    with pytest.raises(vpc.VpcError, match="2 values for 3 members"):
        E.MIWEnsembleTrainer([_m(), _m(), _m()], lr=[1e-3, 2e-3])


def test_member_record_matches_the_header():
    assert E.MEMBER_DTYPE.itemsize == 24 and E.MEMBER_DTYPE.names == ("seed", "alpha", "keep_prob", "lr", "reserved")
    assert [E.MEMBER_DTYPE.fields[k][1] for k in E.MEMBER_DTYPE.names] == [0, 8, 12, 16, 20]
    assert len(E.LAUNCHES) == 5


# ------------------------------------------------------------------------------------------------ train_sweep's grouping
def _groups(monkeypatch, rows):
    if rows is None:
        monkeypatch.delenv("VPC_MIW_SMALL", raising=False)
    else:
        monkeypatch.setenv("VPC_MIW_SMALL", str(rows))
    models = [_m(getattr(miwae, cls), d, Ld, S) for _, cls, d, Ld, S in EC.SWEEP_MIX]
    cfgs = harness._sweep_configs([dict(vae_type=vt) for vt, *_ in EC.SWEEP_MIX], models)
    loader = [(torch.rand(64, 12), torch.ones(64, 12, dtype=torch.bool))]
    keys = harness._family_groups(cfgs, models, (loader, None), None, 12, 500, 10, 10, 30, "synth", TP, 1, 20, 10, "e", "ml_reg")
    out = {}
    for g, k in keys.items():
        assert k[0] == "miw"
        out.setdefault((k[1].__name__,) + tuple(k[2:]), []).append(g)
    return out


def test_sweep_groups_with_the_small_step_on(monkeypatch):
    assert _groups(monkeypatch, 1 << 20) == EC.SWEEP_GROUPS
    # the limit is small_step_route's: P * B * S decoder rows of the FIRST batch.  2 * 64 * 20 = 2 560 for the Reg members,
    # 1 280 for the vanilla ones
    assert _groups(monkeypatch, 2559) == {("MIWAE", 12, 10, 20): [1, 3, 5]}
    assert _groups(monkeypatch, 1279) == {}


def test_sweep_groups_without_the_variable(monkeypatch):
    assert _groups(monkeypatch, None) == {} and _groups(monkeypatch, 0) == {}


def test_sweep_key():
    loader = [(torch.rand(64, 12), torch.ones(64, 12))]
    assert E.sweep_key(_m(), "reg_MIWAE1", loader, 12, 2560) == ("miw", miwae.Reg_MIWAE, 12, 10, 20)
    assert E.sweep_key(_m(), "reg_MIWAE1", loader, 12, 2559) is None and E.sweep_key(_m(), "reg_MIWAE1", [], 12, 1 << 20) is None
    assert E.sweep_key(_m(d=33), "reg_MIWAE1", [(torch.rand(4, 33), torch.ones(4, 33))], 33, 1 << 20) is None
    assert E.sweep_key(torch.nn.Linear(2, 2), "reg_MIWAE1", loader, 12, 1 << 20) is None
    van = _m(miwae.MIWAE)
    assert E.sweep_key(van, "vanilla_MIWAE1", loader, 12, 1 << 20) == ("miw", miwae.MIWAE, 12, 10, 20)
    assert E.sweep_key(van, "vanilla_MIWAE1_with_drop", loader, 12, 1 << 20) is None


class _CountingLoader:
    """A loader that counts how often it is iterated (one with a generator of its own would be advanced by every look)."""

    def __init__(self):
        self.looks = 0

    def __iter__(self):
        self.looks += 1
        return iter([(torch.rand(64, 12), torch.ones(64, 12, dtype=torch.bool))])


def test_nothing_is_built_or_read_with_the_small_step_off(monkeypatch):
    """VPC_MIW_SMALL unset, or a 'with_drop' name: no throw-away model, no look at the loader."""
    built = []
    real = harness.model_loader
    monkeypatch.setattr(harness, "model_loader", lambda *a, **k: built.append(a) or real(*a, **k))
    names = ["reg_MIWAE1", "reg_MIWAE2", "vanilla_MIWAE1_with_drop", "vanilla_MIWAE2_with_drop"]
    cfgs = harness._sweep_configs([dict(vae_type=vt) for vt in names])
    args = (12, 500, 10, 10, 30, "synth", TP, 1, 20, 10, "e", "ml_reg")
    for env in (None, "0"):
        monkeypatch.delenv("VPC_MIW_SMALL", raising=False) if env is None else monkeypatch.setenv("VPC_MIW_SMALL", env)
        loader = _CountingLoader()
        assert harness._family_groups(cfgs, None, (loader, None), None, *args) == {}
        assert built == [] and loader.looks == 0
        models = [_m(), _m(), _m(miwae.MIWAE), _m(miwae.MIWAE)]
        assert harness._family_groups(cfgs, models, (loader, None), None, *args) == {} and loader.looks == 0
    monkeypatch.setenv("VPC_MIW_SMALL", str(1 << 20))
    loader = _CountingLoader()
    keys = harness._family_groups(cfgs, None, (loader, None), None, *args)
    assert sorted(keys) == [0, 1] and len(built) == 2 and loader.looks == 2  # the two with_drop runs: neither built nor read


# ------------------------------------------------------------------------------------------------ the partial buffer
def test_partial_buffer_size_rule():
    n = E.n_params(12, 10)
    assert n == 43320  # MiwOff of the wine shape
    assert n == sum(p.numel() for p in _m().parameters())
    assert E.n_params(32, 16) == sum(p.numel() for p in _m(d=32, Ld=16).parameters())
    assert E.partial_floats(64, 32, n) == 64 * 32 * n == 88719360  # 355 MB
    assert E.partial_floats(1, 1, n) == n
    assert E.partial_floats(64, 4, n) * 4 < 45e6 and E.PART_MAX_FLOATS == 1 << 28
    # the whole-chip stand-alone grid for 64 members (128 blocks each) passes the limit; the default rule's 4 blocks do not
    assert E.partial_floats(64, 128, n) > E.PART_MAX_FLOATS > E.partial_floats(64, E.default_blocks(64, 128, 256)[1], n)


# ------------------------------------------------------------------------------------------------ the default rule
def test_default_rule():
    d = E.default_blocks
    # (G, R) at 256 compute units: rb from all G * R rows of the launch, blocks = ceil(256 / G) up to the member's row blocks
    assert d(1, 128, 256) == (1, 128) and d(1, 64, 256) == (1, 64)  # one member: the stand-alone step's own choice and grid
    assert d(2, 128, 256) == (1, 128) and d(4, 128, 256) == (2, 64) and d(4, 64, 256) == (1, 64)
    assert d(8, 128, 256) == (4, 32) and d(8, 64, 256) == (2, 32)
    assert d(64, 128, 256) == (4, 4) and d(64, 64, 256) == (4, 4)
    assert d(300, 128, 256) == (4, 1) and d(3, 5, 256) == (1, 5) and d(3, 1, 256) == (1, 1)
    assert d(64, 128, 256, rb=1) == (1, 4) and d(2, 10, 256, rb=4) == (4, 3)
    for G in (1, 2, 3, 8, 9, 64, 100):
        for R in (1, 5, 37, 74, 128, 1000):
            rb, blocks = d(G, R, 256)
            assert rb in (1, 2, 4) and 1 <= blocks <= min(-(-R // rb), 256)
            # bit-equality with the stand-alone step holds where the rule keeps every row block its own workgroup
            if G * -(-R // rb) <= 256:
                assert blocks == -(-R // rb)
