"""fp32 encoder forward, both passes of a tile in one sweep over the weights (csrc/vpc_enc_sweep_body.h, enc_fwd_sweep_kernel,
layer_fwd2_b of vpc_device.h) against the pass-loop kernels (enc_fwd_kernel / enc_fwd_draw_kernel).

The same trainer from one seed with VPC_ENC_SWEEP=1 and =0 must agree bit for bit in everything a step leaves behind - the
draws, the loss terms, the gradient, the parameters, both Adam moments, the Philox offset and the encoder's h1 / h2 / mean /
logvar workspaces - after each of two steps, in the drawing form (VPC_DRAW_FUSED=1: vpc_encoder_fwd_draw_f32) and in the
non-drawing form (VPC_DRAW_FUSED=0 or an injected mask_p: vpc_encoder_fwd), on the smallest shapes at which the kernel can go
wrong.  Which kernel form ran is read back from the library (vpc_encoder_fwd_last_form); steps the sweep is not eligible for
keep the pass loop - and their entry points - with the switch on.
"""
import pytest
import torch

L = 10
DEV = "cuda"
TP = {"batch_size": 64, "patience": 100}
PASSES, PASSES_DRAW, SWEEP, SWEEP_DRAW = 0, 1, 2, 3  # VPC_ENC_FWD_* of include/vpc.h


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
    return rec.names, int(_lib.lib().vpc_encoder_fwd_last_form())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _state(tr, planes):
    st = {"mask_p": tr.mask_p_buf.clone(), "eps": tr.eps_buf[:planes].clone(), "out9": tr.out9.clone(),
          "grad": tr.grad.clone(), "flat": tr.model._flat.clone(), "exp_avg": tr.exp_avg.clone(),
          "exp_avg_sq": tr.exp_avg_sq.clone(), "rng_offset": tr.rng_offset}
    for name in ("mean", "logvar", "h1", "h2"):
        for p, t in enumerate(getattr(tr, name)):
            st[f"{name}{p}"] = t.clone()
    return st


def _same(a, b, skip=()):
    assert a.keys() == b.keys()
    for k in a:
        if k in skip:
            continue
        ok = (a[k] == b[k]) if k == "rng_offset" else torch.equal(_bits(a[k]), _bits(b[k]))
        assert ok, k


def _two_steps(vpc, monkeypatch, sweep, draw, make, x, mask, planes=2, graph=False, expect_form=None, expect_names=(), **kw):
    """Two consecutive steps of a fresh trainer with VPC_ENC_SWEEP = sweep; the throughput shape is forced (VPC_TILE=128: the
    8-wave kernels, two passes in one workgroup) and VPC_DRAW_FUSED picks the drawing / non-drawing entry point.  Returns the
    state after each step."""
    monkeypatch.setenv("VPC_TILE", "128")
    monkeypatch.setenv("VPC_DRAW_FUSED", "1" if draw else "0")
    monkeypatch.setenv("VPC_ENC_SWEEP", "1" if sweep else "0")
    tr = make()
    out = []
    for i in range(2):
        step = (lambda: tr.step_graph(x, mask, **kw)) if graph else (lambda: tr.step(x, mask, **kw))
        names, form = _record(monkeypatch, step)
        if not graph:  # (a replay launches nothing through the library)
            assert form == expect_form, (form, names)
            for n in expect_names:
                assert n in names, names
        out.append(_state(tr, planes))
    return out


def _reg_vae(vpc, d, seed=5, precision="f32", cls="Reg_VAE"):
    def make():
        torch.manual_seed(0)
        m = getattr(vpc, cls)(d, 500, 10, L, TP, "exp", "kl_reg") if cls.startswith("Reg") else getattr(vpc, cls)(d, 500, 10, L, TP, "exp")
        return vpc.FusedTrainer(m.to(DEV), seed=seed, precision=precision)
    return make


def _big_B(vpc):
    return 128 * vpc._lib.num_cus() + 129


@pytest.mark.gpu
@pytest.mark.parametrize("draw", [True, False], ids=["draw", "nodraw"])
@pytest.mark.parametrize("shape", ["d128_b300", "d128_b257", "d72_b300", "two_tiles_per_wg"])
def test_sweep_equals_pass_loop(shape, draw, monkeypatch):
    """(128, 300): two full tiles and a 44-row remainder; (128, 257): a last tile of one row; d = 72: column groups past d;
    128 x CUs + 129 rows: some workgroups run two tiles (the next-tile prefetch under the sweep) and the last tile has one row."""
    import vpc_amd as vpc
    d, B = {"d128_b300": (128, 300), "d128_b257": (128, 257), "d72_b300": (72, 300),
            "two_tiles_per_wg": (128, _big_B(vpc))}[shape]
    x, mask = _data(B, d, seed=B % 1000 + d)
    entry = "vpc_encoder_fwd_draw_f32" if draw else "vpc_encoder_fwd"
    new = _two_steps(vpc, monkeypatch, True, draw, _reg_vae(vpc, d), x, mask, expect_form=SWEEP_DRAW if draw else SWEEP,
                     expect_names=(entry,), alpha=0.8, beta=0.9)
    old = _two_steps(vpc, monkeypatch, False, draw, _reg_vae(vpc, d), x, mask, expect_form=PASSES_DRAW if draw else PASSES,
                     expect_names=(entry,), alpha=0.8, beta=0.9)
    for a, b in zip(new, old):
        _same(a, b)


@pytest.mark.gpu
def test_default_selection(monkeypatch):
    """Without the switch the drawing entry point takes the sweep and the non-drawing one keeps the pass loop."""
    import vpc_amd as vpc
    from vpc_amd import _lib
    x, mask = _data(300, 128, seed=17)
    monkeypatch.setenv("VPC_TILE", "128")
    monkeypatch.delenv("VPC_ENC_SWEEP", raising=False)
    for draw, form in ((True, SWEEP_DRAW), (False, PASSES)):
        monkeypatch.setenv("VPC_DRAW_FUSED", "1" if draw else "0")
        _reg_vae(vpc, 128)().step(x, mask, alpha=0.8, beta=0.9)
        assert int(_lib.lib().vpc_encoder_fwd_last_form()) == form


@pytest.mark.gpu
@pytest.mark.parametrize("draw", [True, False], ids=["draw", "nodraw"])
def test_sweep_sharded(draw, monkeypatch):
    """Rows 300..599 of a global batch of 600 (the draw counters start at element 300 d)."""
    import vpc_amd as vpc
    d, B, Bg = 128, 300, 600
    x, mask = _data(Bg, d, seed=3)
    kw = dict(alpha=0.8, beta=0.9, update=False, global_batch=Bg, row_lo=B)
    new = _two_steps(vpc, monkeypatch, True, draw, _reg_vae(vpc, d), x[B:], mask[B:], expect_form=SWEEP_DRAW if draw else SWEEP, **kw)
    old = _two_steps(vpc, monkeypatch, False, draw, _reg_vae(vpc, d), x[B:], mask[B:], expect_form=PASSES_DRAW if draw else PASSES, **kw)
    for a, b in zip(new, old):
        _same(a, b)


@pytest.mark.gpu
def test_sweep_injected_mask_p(monkeypatch):
    """An injected mask_p: the non-drawing form reads both masks (mask_p_buf is not written)."""
    import vpc_amd as vpc
    d, B = 128, 300
    x, mask = _data(B, d, seed=9)
    mask_p = mask & (torch.rand(B, d, generator=torch.Generator().manual_seed(1)) < 0.7).to(DEV)
    kw = dict(alpha=0.8, beta=0.9, mask_p=mask_p)
    new = _two_steps(vpc, monkeypatch, True, True, _reg_vae(vpc, d), x, mask, expect_form=SWEEP, expect_names=("vpc_encoder_fwd",), **kw)
    old = _two_steps(vpc, monkeypatch, False, True, _reg_vae(vpc, d), x, mask, expect_form=PASSES, expect_names=("vpc_encoder_fwd",), **kw)
    for a, b in zip(new, old):
        _same(a, b, skip=("mask_p",))


@pytest.mark.gpu
def test_sweep_graph_replay(monkeypatch):
    """step_graph (one eager step that captures, then a replay: the Philox offset lives on the device) with the sweep against
    the same pair with the pass loop, and against two eager steps."""
    import vpc_amd as vpc
    d, B = 128, 300
    x, mask = _data(B, d, seed=11)
    kw = dict(alpha=0.8, beta=0.9)
    g = _two_steps(vpc, monkeypatch, True, True, _reg_vae(vpc, d), x, mask, graph=True, **kw)
    h = _two_steps(vpc, monkeypatch, False, True, _reg_vae(vpc, d), x, mask, graph=True, **kw)
    e = _two_steps(vpc, monkeypatch, True, True, _reg_vae(vpc, d), x, mask, expect_form=SWEEP_DRAW, **kw)
    for a, b, c in zip(g, h, e):
        _same(a, b)
        _same(a, c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["vanilla", "mask_augmented", "bf16x3", "d64"])
def test_ineligible_steps_keep_pass_loop(case, monkeypatch):
    """One pass, the mask-augmented encoder input, another precision, d <= 64: the pass-loop kernels stay with the switch on
    (the library reports the form it launched, through the entry point the step used before), and the step gives what it gives
    with the switch off."""
    import vpc_amd as vpc
    d, B = (64 if case == "d64" else 128 if case != "mask_augmented" else 60), 300
    x, mask = _data(B, d, seed=13)
    cls = {"vanilla": "vanilla_VAE", "mask_augmented": "Reg_VAE_mask"}.get(case, "Reg_VAE")
    make = _reg_vae(vpc, d, precision="bf16x3" if case == "bf16x3" else "f32", cls=cls)
    planes = 1 if case == "vanilla" else 2
    res = [_two_steps(vpc, monkeypatch, sweep, False, make, x, mask, planes=planes, expect_form=PASSES,
                      expect_names=("vpc_encoder_fwd",), alpha=0.8, beta=0.9) for sweep in (True, False)]
    for a, b in zip(*res):
        _same(a, b, skip=("mask_p",) if case == "vanilla" else ())
