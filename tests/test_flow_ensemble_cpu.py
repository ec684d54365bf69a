"""The host rules of the flow ensemble step (vpc_amd/flow_ensemble.py) that need no GPU: what an ensemble may hold (raised
before anything touches the device), the member record against include/vpc.h, how harness.train_sweep groups flow members with
VPC_FLOW_SMALL set and unset, and the size rule of the workspaces."""
import os
import re

import pytest
import torch

import vpc_amd as vpc
from vpc_amd import flow, harness
from vpc_amd import flow_ensemble as E
from vpc_amd import miwae

TP = {"batch_size": 64, "patience": 1}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vpc.h")


def _m(cls=None, d=12, H=36):
    return (cls or flow.REG_VAEFlow)(d, H, 10, 10, TP)  # on the CPU: validation comes before the device


# ------------------------------------------------------------------------------------------------ validation
def test_validation_comes_first_and_says_why(monkeypatch):
    def no_cuda(*a, **k):
        raise AssertionError("a CUDA call before the refusal")

    monkeypatch.setattr(torch.cuda, "current_stream", no_cuda)
    monkeypatch.setattr(E, "stack_models", no_cuda)
    with pytest.raises(TypeError, match="supports VAEFlow and REG_VAEFlow members, got Reg_MIWAE"):
        E.FlowEnsembleTrainer([_m(), miwae.Reg_MIWAE(12, 500, 10, 10, TP, 20, 1)])
    with pytest.raises(TypeError, match="members of one ensemble share a class: REG_VAEFlow and VAEFlow"):
        E.FlowEnsembleTrainer([_m(), _m(flow.VAEFlow)])
    with pytest.raises(vpc.VpcError, match=r"share \(obs_dim, hid_dim\): \(12, 36\) and \(12, 37\)"):
        E.FlowEnsembleTrainer([_m(), _m(H=37)])
    with pytest.raises(vpc.VpcError, match=r"share \(obs_dim, hid_dim\): \(12, 36\) and \(13, 36\)"):
        E.FlowEnsembleTrainer([_m(), _m(d=13)])
    with pytest.raises(vpc.VpcError, match="hid_dim <= 1024.*hid_dim 1025"):
        E.FlowEnsembleTrainer([_m(H=1025)])
    with pytest.raises(vpc.VpcError, match=r"2 \* obs_dim <= 1024.*obs_dim 513"):
        E.FlowEnsembleTrainer([_m(d=513, H=4)])  # 2 * obs_dim = 1026
    with pytest.raises(vpc.VpcError, match="single-process"):
        E.FlowEnsembleTrainer([_m(), _m()], world_size=2)
    with pytest.raises(vpc.VpcError, match="at least one member"):
        E.FlowEnsembleTrainer([])
    one = _m(H=4)
    with pytest.raises(vpc.VpcError, match="4097 members: one ensemble holds 4096"):
        E.FlowEnsembleTrainer([one] * 4097)
    with pytest.raises(vpc.VpcError, match="order = 2"):
        E.FlowEnsembleTrainer([_m()], order=2)
    with pytest.raises(vpc.VpcError, match="2 values for 3 members"):
        E.FlowEnsembleTrainer([_m(), _m(), _m()], lr=[1e-3, 2e-3])
    E.validate_members([_m(d=512, H=1024)])  # the limits themselves pass


def test_member_record_matches_the_header():
    src = open(HEADER).read()
    body = re.search(r"typedef struct VpcFlowMember \{(.*?)\} VpcFlowMember;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.match(r"\s*(.*?)\s*(\w+)(\[(\d+)\])?$", f).groups() for f in body.split(";") if f.strip()]
    sizes = {"unsigned long long": 8, "float": 4, "int": 4}
    names = tuple(f[1] for f in fields)
    assert names == E.MEMBER_DTYPE.names == ("seed", "alpha", "beta", "keep_prob", "lr", "reserved")
    off = 0
    for ctype, name, _, count in fields:
        dt, o = E.MEMBER_DTYPE.fields[name][:2]
        assert o == off and dt.itemsize == sizes[ctype] * int(count or 1), name
        off += dt.itemsize
    assert off == E.MEMBER_DTYPE.itemsize == 32
    assert len(E.LAUNCHES) == 21 and "#define VPC_FLOW_MULTI_MAX_MEMBERS 4096" in src and E.MAX_MEMBERS == 4096


# ------------------------------------------------------------------------------------------------ train_sweep's grouping
# (vae_type, class, hid_dim): reg_flow1-3, vanilla_flow1-2, a with_drop pair, a flow member of another hid_dim, two MIWAE members
MIX = [("reg_flow1", "REG_VAEFlow", 36), ("vanilla_flow1", "VAEFlow", 36), ("reg_flow2", "REG_VAEFlow", 36),
       ("vanilla_flow4_with_drop", "VAEFlow", 36), ("vanilla_flow2", "VAEFlow", 36), ("reg_flow3", "REG_VAEFlow", 36),
       ("vanilla_flow4_with_drop", "VAEFlow", 36), ("reg_flow1", "REG_VAEFlow", 40), ("reg_MIWAE1", None, 0),
       ("reg_MIWAE2", None, 0)]
ARGS = (12, 36, 10, 10, 30, "synth", TP, 1, 20, 10, "e", "ml_reg")


def _mix_models():
    return [miwae.Reg_MIWAE(12, 500, 10, 10, TP, 20, 1) if cls is None else _m(getattr(flow, cls), 12, H) for _, cls, H in MIX]


def _groups(monkeypatch, rows, B=64):
    monkeypatch.delenv("VPC_MIW_SMALL", raising=False)
    if rows is None:
        monkeypatch.delenv("VPC_FLOW_SMALL", raising=False)
    else:
        monkeypatch.setenv("VPC_FLOW_SMALL", str(rows))
    models = _mix_models()
    cfgs = harness._sweep_configs([dict(vae_type=vt) for vt, *_ in MIX], models)
    loader = [(torch.rand(B, 12), torch.ones(B, 12, dtype=torch.bool))]
    keys = harness._family_groups(cfgs, models, (loader, None), None, *ARGS)
    out = {}
    for g, k in keys.items():
        assert k[0] == "flow"
        out.setdefault((k[1].__name__,) + tuple(k[2:]), []).append(g)
    return out


def test_sweep_groups_with_the_small_step_on(monkeypatch):
    assert _groups(monkeypatch, 128) == {("REG_VAEFlow", 12, 36): [0, 2, 5], ("VAEFlow", 12, 36): [1, 4]}
    # the limit is small_step_route's: R = P * B stacked rows of the FIRST batch, at most 128
    assert _groups(monkeypatch, 127) == {("VAEFlow", 12, 36): [1, 4]}
    assert _groups(monkeypatch, 128, B=65) == {("VAEFlow", 12, 36): [1, 4]}  # REG: R = 130
    assert _groups(monkeypatch, 100000, B=129) == {}  # vanilla: R = 129
    assert _groups(monkeypatch, 100000, B=128) == {("VAEFlow", 12, 36): [1, 4]}


def test_sweep_groups_without_the_variable(monkeypatch):
    assert _groups(monkeypatch, None) == {} and _groups(monkeypatch, 0) == {}


def test_sweep_key():
    loader = [(torch.rand(64, 12), torch.ones(64, 12))]
    assert E.sweep_key(_m(), "reg_flow1", loader, 12, 128) == ("flow", flow.REG_VAEFlow, 12, 36)
    assert E.sweep_key(_m(), "reg_flow1", loader, 12, 127) is None and E.sweep_key(_m(), "reg_flow1", [], 12, 128) is None
    assert E.sweep_key(_m(flow.VAEFlow), "vanilla_flow1", loader, 12, 64) == ("flow", flow.VAEFlow, 12, 36)
    assert E.sweep_key(_m(flow.VAEFlow), "vanilla_flow4_with_drop", loader, 12, 128) is None
    assert E.sweep_key(torch.nn.Linear(2, 2), "reg_flow1", loader, 12, 128) is None
    assert E.sweep_key(_m(H=1025), "reg_flow1", loader, 12, 128) is None
    assert E.MIN_GROUP >= 2


class _CountingLoader:
    """A loader that counts how often it is iterated."""

    def __init__(self):
        self.looks = 0

    def __iter__(self):
        self.looks += 1
        return iter([(torch.rand(64, 12), torch.ones(64, 12, dtype=torch.bool))])


def test_nothing_is_built_or_read_with_the_small_step_off(monkeypatch):
    built = []
    real = harness.model_loader
    monkeypatch.setattr(harness, "model_loader", lambda *a, **k: built.append(a) or real(*a, **k))
    monkeypatch.delenv("VPC_MIW_SMALL", raising=False)
    models = _mix_models()
    cfgs = harness._sweep_configs([dict(vae_type=vt) for vt, *_ in MIX], models)
    for env in (None, "0"):
        monkeypatch.delenv("VPC_FLOW_SMALL", raising=False) if env is None else monkeypatch.setenv("VPC_FLOW_SMALL", env)
        loader = _CountingLoader()
        assert harness._family_groups(cfgs, models, (loader, None), None, *ARGS) == {}
        assert built == [] and loader.looks == 0
        assert E.sweep_key(models[0], "reg_flow1", loader, 12) is None and loader.looks == 0
    monkeypatch.setenv("VPC_FLOW_SMALL", "128")
    loader = _CountingLoader()
    keys = harness._family_groups(cfgs, models, (loader, None), None, *ARGS)
    assert sorted(keys) == [0, 1, 2, 4, 5] and built == []
    assert loader.looks == 6  # the six flow members without with_drop, the one of another hid_dim included


# ------------------------------------------------------------------------------------------------ the workspaces
def test_workspace_size_rule():
    # the wine shape, REG at B = 64 (R = 128): 128 rows x (24 xin + 6 x 10 + 2 x 100 + 12 x 500 + 2 x 12) = 128 x 6308, every
    # slice a multiple of 4 already, and mask_p 64 x 12
    assert E.workspace_floats(1, 128, 64, 12, 500, True) == 128 * 6308 + 768 == 808192
    assert E.workspace_floats(64, 128, 64, 12, 500, True) == 64 * 808192 < E.WORKSPACE_MAX_FLOATS == 1 << 28
    assert E.workspace_floats(1, 128, 128, 12, 500, False) == 128 * 6308
    # (5, 37, 17) REG, R = 34: xin 340; six [34][10] = 6 x 340; t, dt 2 x 3400; twelve [34][37] = 1258 -> 1260 each; Y, G
    # 170 -> 172 each; mask_p 85 -> 88
    assert E.workspace_floats(1, 34, 17, 5, 37, True) == 340 + 2040 + 6800 + 12 * 1260 + 2 * 172 + 88 == 24732
    assert E.workspace_floats(3, 34, 17, 5, 37, True) == 3 * 24732
    assert E.workspace_floats(4096, 128, 64, 12, 500, True) > E.WORKSPACE_MAX_FLOATS  # the member limit alone does not bound it
