"""Row-tiled fp32 step: encoder forward, fused decoder and encoder backward as three phases of ONE launch
(csrc/vpc_step_f32.hip, vpc_step_f32, FusedTrainer._step_f32).

The phases are the text of the three kernels, so everything a step leaves behind - draws, loss terms, gradient, parameters,
Adam moments, and the h1 / h2 / mean / logvar / dmean / dlogvar workspaces of both passes - must be bit-identical to the three
launches.  VPC_STEP_F32=1 takes the one launch at any batch size, with the encoder backward in the throughput shape (128-row
tiles); the three launches it is compared with run that shape too (VPC_TILE=128), so the partial blocks - and with them the
gradient's summation order - are the same.  Steps that are not eligible keep the three launches with the switch on.
Host only (no GPU): the entry point refuses, before it launches anything, phases that would not share one grid and bad arguments.
"""
import ctypes as C
import os

import pytest
import torch

L = 10
DEV = "cuda"
TP = {"batch_size": 64, "patience": 100}
WS = ("h1", "h2", "mean", "logvar", "dmean", "dlogvar")


def _data(B, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, d, generator=g).to(DEV), (torch.rand(B, d, generator=g) < 0.7).to(DEV)


class _Recorder:
    """Stands in for the loaded library: records every vpc_* symbol fetched, hands out the real one."""

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        if name.startswith("vpc_"):
            self.names.append(name)
        return getattr(self.real, name)


def _record(monkeypatch, fn):
    from vpc_amd import _lib
    rec = _Recorder(_lib.lib())
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "_lib", rec)
        fn()
    return rec.names


def _state(tr, planes=2):
    st = {"mask_p": tr.mask_p_buf.clone(), "eps": tr.eps_buf[:planes].clone(), "out9": tr.out9.clone(),
          "grad": tr.grad.clone(), "flat": tr.model._flat.clone(), "exp_avg": tr.exp_avg.clone(),
          "exp_avg_sq": tr.exp_avg_sq.clone(), "rng_offset": tr.rng_offset}
    for name in WS:
        for p, t in enumerate(getattr(tr, name)):
            st[f"{name}{p}"] = t.clone()
    return st


def _same(a, b, skip=()):
    assert a.keys() == b.keys()
    for k in a:
        if k in skip:
            continue
        u, v = a[k], b[k]
        ok = (u == v) if k == "rng_offset" else torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u,
                                                            v.view(torch.int32) if v.dtype == torch.float32 else v)
        assert ok, k


ONE = ("vpc_step_f32",)
THREE = ("vpc_encoder_fwd_draw_f32", "vpc_decoder_fused_draw_f32", "vpc_encoder_bwd")


def _env(monkeypatch, one):
    """The switch on: nothing else selects a shape.  Off: the three launches in the shape the one launch runs."""
    monkeypatch.setenv("VPC_STEP_F32", "1" if one else "0")
    monkeypatch.setenv("VPC_DRAW_FUSED", "1")
    monkeypatch.setenv("VPC_STEP_SMALL", "0")
    if one:
        monkeypatch.delenv("VPC_TILE", raising=False)
    else:
        monkeypatch.setenv("VPC_TILE", "128")


def _two_steps(vpc, monkeypatch, one, d, B, graph=False, data=None, **kw):
    """Two consecutive steps of a fresh Reg_VAE trainer (seed 5); the state after each, and the symbols each step fetched."""
    _env(monkeypatch, one)
    torch.manual_seed(0)
    tr = vpc.FusedTrainer(vpc.Reg_VAE(d, 500, 10, L, TP, "exp", "kl_reg").to(DEV), seed=5)
    x, mask = data if data is not None else _data(B, d, seed=B + d)
    out = []
    for i in range(2):
        step = (lambda: tr.step_graph(x, mask, alpha=0.8, beta=0.9)) if graph else \
               (lambda: tr.step(x, mask, alpha=0.8, beta=0.9, **kw))
        names = _record(monkeypatch, step)
        if not graph:
            assert all((n in names) == one for n in ONE), names
            assert all((n in names) != one for n in THREE), names
            assert tr.dominant_launch() == ("step_fused" if one else "decoder_fused")
        out.append(_state(tr))
    return out


def _big_B():
    from vpc_amd import _lib
    return 128 * _lib.num_cus() + 129


@pytest.mark.gpu
@pytest.mark.parametrize("d,B", [(128, 300), (128, 257), (72, 300), (128, None)],
                         ids=["d128_b300", "d128_b257", "d72_b300", "d128_two_tiles_per_wg"])
def test_one_launch_equals_three(d, B, monkeypatch):
    """(128, 300): three workgroups, the last tile ragged; (128, 257): a one-row tile; d = 72: column tiles that can hold
    out-of-range columns; 128 x CUs + 129 rows: two workgroups run two tiles in every phase, one of them a one-row tile."""
    import vpc_amd as vpc
    B = _big_B() if B is None else B
    new = _two_steps(vpc, monkeypatch, True, d, B)
    old = _two_steps(vpc, monkeypatch, False, d, B)
    for a, b in zip(new, old):
        _same(a, b)
    from vpc_amd import _lib
    assert _lib.lib().vpc_encoder_fwd_last_form() == 3  # VPC_ENC_FWD_SWEEP_DRAW, from either path


@pytest.mark.gpu
def test_one_launch_sharded(monkeypatch):
    """Rows 300..599 of a global batch of 600 (the draws' counters are those of the global rows)."""
    import vpc_amd as vpc
    x, mask = _data(600, 128, seed=3)
    kw = dict(data=(x[300:], mask[300:]), global_batch=600, row_lo=300, update=False)
    new = _two_steps(vpc, monkeypatch, True, 128, 300, **kw)
    old = _two_steps(vpc, monkeypatch, False, 128, 300, **kw)
    for a, b in zip(new, old):
        _same(a, b)


@pytest.mark.gpu
def test_one_launch_graph_replay(monkeypatch):
    """step_graph (an eager step that captures, then a replay: the Philox offsets live on the device and reach both drawing
    phases through `state`) against two eager steps of the one launch and against the replayed three launches."""
    import vpc_amd as vpc
    g = _two_steps(vpc, monkeypatch, True, 128, 300, graph=True)
    e = _two_steps(vpc, monkeypatch, True, 128, 300)
    h = _two_steps(vpc, monkeypatch, False, 128, 300, graph=True)
    for a, b, c in zip(g, e, h):
        _same(a, b)
        _same(a, c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["vanilla", "mask_augm", "bf16x3", "d64", "d100", "mask_p_injected", "eps_injected", "ml_reg"])
def test_ineligible_steps_keep_three_launches(case, monkeypatch):
    """One pass, the mask-augmented encoder, another precision, d <= 64, d % 8 != 0, an injected draw, the ml_reg sample (a third
    eps plane): the three launches stay with the switch on, and the step gives what it gives with the switch off."""
    import vpc_amd as vpc
    monkeypatch.setenv("VPC_DRAW_FUSED", "1")
    monkeypatch.setenv("VPC_STEP_SMALL", "0")
    monkeypatch.delenv("VPC_TILE", raising=False)
    d = {"d64": 64, "d100": 100, "mask_augm": 64}.get(case, 128)
    B = 300
    x, mask = _data(B, d, seed=9)
    gen = torch.Generator().manual_seed(1)
    inj = {}
    if case == "mask_p_injected":
        inj = dict(mask_p=mask & (torch.rand(B, d, generator=gen) < 0.7).to(DEV))
    if case == "eps_injected":
        inj = dict(eps_q=torch.randn(B, L, generator=gen).to(DEV), eps_p=torch.randn(B, L, generator=gen).to(DEV))
    kw = dict(alpha=0.8, beta=0.9, epoch=1400 if case == "ml_reg" else 1)
    res = []
    for env in ("1", "0"):
        monkeypatch.setenv("VPC_STEP_F32", env)
        torch.manual_seed(0)
        if case == "vanilla":
            m = vpc.vanilla_VAE(d, 500, 10, L, TP, "exp")
        elif case == "mask_augm":
            m = vpc.Reg_VAE_mask(d, 500, 10, L, TP, "exp", "kl_reg")
        else:
            m = vpc.Reg_VAE(d, 500, 10, L, TP, "exp", "ml_reg" if case == "ml_reg" else "kl_reg")
        tr = vpc.FusedTrainer(m.to(DEV), seed=5, precision="bf16x3" if case == "bf16x3" else "f32")
        for i in range(2):
            names = _record(monkeypatch, lambda: tr.step(x, mask, **inj, **kw))
            assert "vpc_step_f32" not in names, names
            assert "vpc_encoder_bwd" in names, names
            assert tr.dominant_launch() == "decoder_fused"
        if case == "ml_reg":
            assert tr.coefficients(1400, 0.8, 0.9, False).ml_on
        st = _state(tr, 1 if case == "vanilla" else 3 if case == "ml_reg" else 2)
        if case == "eps_injected":  # injected eps fills the L columns it has: the pad columns of eps_buf are not written
            st["eps"] = st["eps"][:, :, :L].contiguous()
        res.append(st)
    skip = ("mask_p",) if case in ("mask_p_injected", "vanilla") else ()  # (mask_p_buf is not written)
    _same(res[0], res[1], skip=skip)


@pytest.mark.gpu
def test_default_selection(monkeypatch):
    """Switch unset: 300 rows keep the three launches (encoder_bwd runs the small-batch shape there), 128 x CUs + 129 rows take
    the one launch."""
    import vpc_amd as vpc
    for k in ("VPC_STEP_F32", "VPC_TILE", "VPC_ENC_SWEEP", "VPC_DEC8"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VPC_STEP_SMALL", "0")
    for B, fused, one in ((300, "1", False), (_big_B(), None, True)):
        if fused is None:
            monkeypatch.delenv("VPC_DRAW_FUSED", raising=False)
        else:
            monkeypatch.setenv("VPC_DRAW_FUSED", fused)
        torch.manual_seed(0)
        tr = vpc.FusedTrainer(vpc.Reg_VAE(128, 500, 10, L, TP, "exp", "kl_reg").to(DEV), seed=5)
        x, mask = _data(B, 128, seed=1)
        names = _record(monkeypatch, lambda: tr.step(x, mask))
        assert ("vpc_step_f32" in names) == one, names
        assert ("vpc_encoder_bwd" in names) != one and ("vpc_decoder_fused_draw_f32" in names) != one, names
        assert "vpc_reduce_step_adam" in names, names
        assert tr.dominant_launch() == ("step_fused" if one else "decoder_fused")
        assert torch.isfinite(tr.out9).all()


# ------------------------------------------------------------------------------------------------------------ host only
def _host_call(monkeypatch, B=300, d=128, Ld=L, force=0, **over):
    """vpc_step_f32 on host buffers that are never dereferenced: every case here is refused before anything is launched."""
    from vpc_amd import _lib
    monkeypatch.delenv("VPC_TILE", raising=False)
    keep = []

    def buf(n=64):
        b = C.create_string_buffer(n + 16)
        keep.append(b)
        return (C.addressof(b) + 15) & ~15

    def arr(n=2):
        a = (C.c_void_p * n)(*[buf() for _ in range(n)])
        keep.append(a)
        return a

    co = _lib.VpcLossCoef((1.0, 1.0), (0.0, 0.0), 1.0, 1.0, 1.0)
    nbE, nbD = C.c_int(-1), C.c_int(-1)
    a = dict(x=buf(), enc_img=buf(), dec_img=buf(), mask_in=buf(), mask_p_out=buf(), maskB=arr(), co=co, h1=arr(), h2=arr(),
             mean=arr(), logvar=arr(), eps=arr(), dmean=arr(), dlogvar=arr(), inv_B=1.0 / max(B, 1), x_logvar=0.0, partE=buf(),
             partD=buf(), loss=buf(), nbE=C.byref(nbE), nbD=C.byref(nbD), B=B, d=d, L=Ld, keep=0.7, seed=5, off_mask=0,
             off_eps=0, state=None, elem_lo=0, rows_global=B, row_lo=0, force=force, stream=None)
    a.update(over)
    rc = _lib.lib().vpc_step_f32(*a.values())
    assert (nbE.value, nbD.value) == (-1, -1)  # nothing was reported: nothing was launched
    return rc


def test_entry_refuses_mismatched_grids(monkeypatch):
    """encoder_bwd runs the small-batch shape (64-row tiles, the passes over blockIdx.y) while all (tile, pass) pairs fit in two
    rounds of workgroups; the two drawing kernels run 128-row tiles at every B: no common grid, return code 4."""
    from vpc_amd import _lib
    ncu = _lib.num_cus()
    assert _lib.ERR_PHASES == 4
    for B in (1, 300, 64 * ncu):
        assert _host_call(monkeypatch, B=B) == 4, B


@pytest.mark.parametrize("over,code", [
    (dict(x=None), 1), (dict(enc_img=None), 1), (dict(dec_img=None), 1), (dict(mask_in=None), 1), (dict(mask_p_out=None), 1),
    (dict(h1=None), 1), (dict(eps=None), 1), (dict(dmean=None), 1), (dict(partE=None), 1), (dict(partD=None), 1),
    (dict(loss=None), 1), (dict(co=None), 1), (dict(B=0), 1), (dict(elem_lo=-8), 1), (dict(row_lo=1), 1),
    (dict(rows_global=299), 1),
    (dict(d=64), 2), (dict(d=100), 2), (dict(d=136), 2), (dict(L=16), 2), (dict(elem_lo=4), 2),
], ids=lambda v: "-".join(f"{k}_{w}" for k, w in v.items()) if isinstance(v, dict) else str(v))
def test_entry_refuses_bad_arguments(over, code, monkeypatch):
    """1: a null pointer, a bad count, a row shard outside its global array; 2: a shape the kernels do not exist for (d outside
    (64, 128] or d % 8 != 0, L > 15, a shard that starts inside a Philox group) - with force_shape on, so that the shape check
    is not what refuses."""
    assert _host_call(monkeypatch, force=1, **over) == code


def test_entry_refuses_misaligned_pointers(monkeypatch):
    from vpc_amd import _lib
    b = C.create_string_buffer(128)
    base = (C.addressof(b) + 15) & ~15
    assert _host_call(monkeypatch, force=1, x=base + 4) == 2       # x rows are read as 16-byte vectors
    assert _host_call(monkeypatch, force=1, mask_in=base + 2) == 2  # mask words
    assert _host_call(monkeypatch, force=1, mask_p_out=base + 1) == 2
