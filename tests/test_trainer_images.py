"""The trainers' shared plumbing (trainer.py) and the one freshness rule of the packed weight images (images.py):
the launch sequence of a steady-state step on every path, and the bf16 whole-step image following parameter writes made
outside the trainer."""
import weakref

import pytest
import torch

import vpc_amd as vpc
from vpc_amd import _lib
from vpc_amd import eddi as ed
from vpc_amd import notmiwae as nm

pytestmark = pytest.mark.gpu


def _data(B, d, seed, float_mask=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, d, generator=g)
    m = torch.rand(B, d, generator=g) < 0.7
    return x.cuda(), (m.float() if float_mask else m).cuda()


def _fused(prec, B):
    torch.manual_seed(0)
    m = vpc.Reg_VAE(128, 500, 10, 10, {"batch_size": B, "patience": 1}, "exp", "kl_reg").cuda()
    tr = vpc.FusedTrainer(m, seed=3, precision=prec)
    x, mk = _data(B, 128, 4)
    return lambda: tr.step(x, mk, alpha=0.9, beta=0.8)


def _nm(prec):
    torch.manual_seed(12)
    m = nm.REG_notMIWAE_v2(128, 128, 10, 10, {"batch_size": 96, "patience": 1}, 20, 1).cuda()
    tr = nm.NMTrainer(m, lr=1e-3, seed=5, precision=prec)
    x, mk = _data(96, 128, 5, float_mask=True)
    return lambda: tr.step(x, mk, alpha=0.5, p_missingness=50)


def _eddi():
    torch.manual_seed(3)
    m = ed.Reg_EDDI(100, 500, 20, 10, {"batch_size": 256, "patience": 1}, "exp", "kl_reg").cuda()
    tr = ed.EDDITrainer(m, seed=9)
    x, mk = _data(256, 100, 6)
    return lambda: tr.step(x, mk, alpha=0.5, p_missingness=30)


def _eddi_small(d):
    torch.manual_seed(3)
    m = ed.Reg_EDDI(d, 500, 10, 10, {"batch_size": 5, "patience": 1}, "exp", "kl_reg").cuda()
    tr = ed.EDDITrainer(m, seed=9)
    x, mk = _data(5, d, 6)
    return lambda: tr.step(x, mk, alpha=0.5, p_missingness=30)


def _wide():
    torch.manual_seed(7)
    m = vpc.Reg_VAE(200, 500, 10, 10, {"batch_size": 96, "patience": 1}, "exp", "kl_reg").cuda()
    tr = vpc.WideTrainer(m, seed=2)
    x, mk = _data(96, 200, 8)
    return lambda: tr.step(x, mk, alpha=0.8, beta=0.9)


def _miw():
    torch.manual_seed(0)
    m = vpc.Reg_MIWAE(12, 500, 10, 10, {"batch_size": 64, "patience": 1}, 20, 1).cuda()
    tr = vpc.MIWTrainer(m, lr=1e-3, seed=1)
    x, mk = _data(64, 12, 0)
    return lambda: tr.step(x, mk, alpha=0.5, p_missingness=30)


def _flow():
    torch.manual_seed(0)
    m = vpc.REG_VAEFlow(12, 500, 10, 10, {"batch_size": 64, "patience": 1}).cuda()
    tr = vpc.FlowTrainer(m, lr=1e-3, seed=1)
    x, mk = _data(64, 12, 0)
    return lambda: tr.step(x, mk, alpha=0.5, p_missingness=30)


def _mnist():
    torch.manual_seed(0)
    m = vpc.Reg_EDDI_mnist(784, 500, 20, 10, {"batch_size": 64, "patience": 1}, "exp", "kl_reg").cuda()
    tr = vpc.EDDIMnistTrainer(m, lr=1e-3, seed=1)
    g = torch.Generator().manual_seed(0)
    x, mk = torch.rand(64, 28, 28, generator=g).cuda(), (torch.rand(64, 28, 28, generator=g) < 0.7).cuda()
    return lambda: tr.step(x, mk, epoch=1, alpha=0.5, p_missingness=30)


_SMALL = ["vpc_step_small_max_rows"]
_FUSED3 = ["vpc_draw_step", "vpc_encoder_fwd", "vpc_decoder_fused", "vpc_encoder_bwd"]
_GEMM_BWD = ["vpc_linear_wgrad", "vpc_linear_dgrad"] * 3
_WIDE_FWD = ["vpc_nm_mul"] + ["vpc_linear_fwd"] * 3 + ["vpc_nm_sample"] + ["vpc_linear_fwd"] * 3
_SWD = ["vpc_linear_wgrad_scratch", "vpc_linear_wgrad", "vpc_linear_dgrad"]
_WIDE_BWD = _SWD * 3 + ["vpc_nm_sample_bwd"] + _SWD * 2 + _SWD[:2]  # decoder, rsample, encoder of one pass
# (path, VPC_TILE, step factory, the vpc_* symbols the 3rd step fetches in order: launches and the host-side queries)
LAUNCHES = [
    ("fused_f32_b64", None, lambda: _fused("f32", 64),
     _SMALL + ["vpc_step_small_draw_f32", "vpc_reduce_step_adam"]),
    ("fused_f32_tile128_b300", "128", lambda: _fused("f32", 300),
     _SMALL + _FUSED3 + ["vpc_reduce_step_adam"]),
    ("fused_bf16_pair_tile64_b300", "64", lambda: _fused("bf16", 300),
     _SMALL + ["vpc_step_fused_applicable", "vpc_pack_weights_bf16"] + _FUSED3 + ["vpc_reduce_step_adam"]),
    ("fused_bf16_step_tile128_b300", "128", lambda: _fused("bf16", 300),
     _SMALL + ["vpc_step_fused_applicable", "vpc_draw_step", "vpc_step_workspace_floats", "vpc_step_fused_bf16",
               "vpc_reduce_step_adam_bf16c"]),
    ("nm_bf16_fused_tail", None, lambda: _nm("bf16"),
     ["vpc_nm_prep", "vpc_nmenc_fwd", "vpc_nm_fused_bwd_step"]),
    ("nm_f32_gemm", None, lambda: _nm("f32"),
     ["vpc_nm_prep"] + ["vpc_linear_fwd"] * 3 + ["vpc_nm_sample"] + ["vpc_linear_fwd"] * 3 + ["vpc_nm_loss"] + _GEMM_BWD +
     ["vpc_nm_sample_bwd"] + _GEMM_BWD[:-1] + ["vpc_linear_wgrad_reduce", "vpc_adam_step"]),
    ("eddi", None, _eddi,
     ["vpc_pack_weights", "vpc_draw_step", "vpc_eddi_fold", "vpc_eddi_front_fwd"] + ["vpc_linear_fwd"] * 3 +
     ["vpc_decoder_fused", "vpc_reduce_partials", "vpc_loss_finalize"] + _GEMM_BWD +
     ["vpc_linear_wgrad_reduce", "vpc_eddi_front_scratch", "vpc_eddi_front_bwd", "vpc_adam_step"]),
    # the small-batch step at B = 5: obs_dim % 4 == 0 draws inside the kernel, else the chain's draw launch on the unpadded rows
    ("eddi_small_b5_d12", None, lambda: _eddi_small(12),
     _SMALL + ["vpc_step_small_eddi_draw_f32", "vpc_reduce_step_adam_eddi"]),
    ("eddi_small_b5_d14", None, lambda: _eddi_small(14),
     _SMALL + ["vpc_draw_step", "vpc_step_small_eddi_f32", "vpc_reduce_step_adam_eddi"]),
    ("wide", None, _wide,
     ["vpc_draw_mask", "vpc_fill_normal"] + _WIDE_FWD * 2 + ["vpc_loss_fwd_bwd", "vpc_loss_finalize"] + _WIDE_BWD * 2 +
     ["vpc_adam_step"]),
    # the three rows below were recorded with this test's _Recorder on the commit before the trainers moved onto the shared
    # chain walkers (config-file shapes: B = 64; wine d = 12; MNIST d = 784).  The lists hold C ABI calls: vpc_flow_loss is two
    # kernel launches (29 calls = the 30 launches of the flow step), and the MNIST step's 40 launches are these 35 calls (the
    # scratch query is host-side) plus torch's own copy kernels between them.
    ("miw_reg_b64", None, _miw,
     ["vpc_nm_prep"] + ["vpc_linear_fwd"] * 3 + ["vpc_miw_sample"] + ["vpc_linear_fwd"] * 3 + ["vpc_miw_loss"] + _GEMM_BWD +
     ["vpc_miw_sample_bwd"] + _GEMM_BWD[:-1] + ["vpc_linear_wgrad_reduce", "vpc_adam_step"]),
    ("flow_reg_b64", None, _flow,
     ["vpc_flow_prep"] + ["vpc_linear_fwd"] * 3 + ["vpc_flow_fwd"] + ["vpc_linear_fwd"] * 5 + ["vpc_flow_loss"] +
     ["vpc_linear_wgrad", "vpc_linear_dgrad"] * 5 + ["vpc_flow_bwd"] + _GEMM_BWD[:-1] +
     ["vpc_linear_wgrad_reduce", "vpc_adam_step"]),
    ("eddi_mnist_reg_b64", None, _mnist,
     ["vpc_draw_mask", "vpc_fill_normal", "vpc_eddiw_fold", "vpc_eddiw_front_fwd"] + ["vpc_linear_fwd"] * 4 + ["vpc_nm_sample"] +
     ["vpc_linear_fwd"] * 4 + ["vpc_loss_fwd_bwd", "vpc_loss_finalize"] + ["vpc_linear_wgrad", "vpc_linear_dgrad"] * 4 +
     ["vpc_nm_sample_bwd"] + ["vpc_linear_wgrad", "vpc_linear_dgrad"] * 4 +
     ["vpc_linear_wgrad_reduce", "vpc_eddiw_front_scratch", "vpc_eddiw_front_bwd", "vpc_adam_step"]),
]


class _Recorder:
    """Stands in for the loaded library: records every vpc_* symbol fetched, hands out the real one."""

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        if name.startswith("vpc_"):
            self.names.append(name)
        return getattr(self.real, name)


@pytest.mark.parametrize("path,tile,make,expected", LAUNCHES, ids=[p[0] for p in LAUNCHES])
def test_steady_state_launch_sequence(path, tile, make, expected, monkeypatch):
    """A steady-state step issues the same launches as before the trainers shared one base class, on every path.  The
    EDDI step re-packs the decoder image lazily at its start (the previous step's Adam left it stale)."""
    if tile:
        monkeypatch.setenv("VPC_TILE", tile)
    else:
        monkeypatch.delenv("VPC_TILE", raising=False)
    step = make()
    step()
    step()
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    step()
    monkeypatch.undo()
    assert rec.names == expected


# ---- the eager path of the GEMM-backed families: model.forward_loss under grad, then backward, through the encoder /
# decoder autograd Functions.  The chain-backed six: B = 8, d = 12, latent 10, K = S = 3 (the flows: hid_dim 64).  The dense
# classes at the three ways a model is wide, and the point-net classes (the mnist pair fed as [B, 4, 5]): B = 5.
_TP5 = {"batch_size": 5, "patience": 1}
_EAGER_B5 = {  # name -> (constructor, input shape, bool masks)
    "Reg_VAE_d129": (lambda: vpc.Reg_VAE(129, 500, 10, 10, _TP5, "exp", "kl_reg"), (5, 129), False),
    "vanilla_VAE_mask_d65": (lambda: vpc.vanilla_VAE_mask(65, 500, 10, 10, _TP5, "exp"), (5, 65), False),
    "Reg_VAE_d14_L16": (lambda: vpc.Reg_VAE(14, 500, 10, 16, _TP5, "exp", "kl_reg"), (5, 14), False),
    "Reg_EDDI": (lambda: vpc.Reg_EDDI(14, 500, 10, 10, _TP5, "exp", "kl_reg"), (5, 14), False),
    "vanilla_EDDI": (lambda: vpc.vanilla_EDDI(14, 500, 10, 10, _TP5, "exp"), (5, 14), False),
    "Reg_EDDI_mnist": (lambda: vpc.Reg_EDDI_mnist(20, 500, 4, 3, _TP5, "exp", "kl_reg"), (5, 4, 5), True),
    "vanilla_EDDI_mnist": (lambda: vpc.vanilla_EDDI_mnist(20, 500, 4, 3, _TP5, "exp"), (5, 4, 5), False),
}


def _eager_model(name):
    torch.manual_seed(0)
    if name in _EAGER_B5:
        return _EAGER_B5[name][0]().cuda()
    if "Flow" in name:
        return getattr(vpc, name)(12, 64, 10, 10, {"batch_size": 8, "patience": 1}).cuda()
    return getattr(vpc, name)(12, 500, 10, 10, {"batch_size": 8, "patience": 1}, 3, 1).cuda()


def _eager_data(name=None):
    _, shape, bool_masks = _EAGER_B5.get(name, (None, (8, 12), False))
    g = torch.Generator().manual_seed(2)
    x, m = torch.rand(*shape, generator=g), torch.rand(*shape, generator=g) < 0.7
    mp = m & (torch.rand(*shape, generator=torch.Generator().manual_seed(3)) < 0.7)
    return x.cuda(), (m if bool_masks else m.float()).cuda(), (mp if bool_masks else mp.float()).cuda()


def _eager_full(name):
    model = _eager_model(name)
    x, m, mp = _eager_data(name)

    def run():
        model.zero_grad()
        _, ret = model.forward_loss(x, m, mp if model.regularised else None, epoch=1, alpha=0.5)
        ret[1].backward()
    return run


def _eager_z_only(name):
    model = _eager_model(name)
    x, m, _ = _eager_data(name)

    def run():
        model.zero_grad()
        model.encoder(x, m)[0].sum().backward()
    return run


_PN_BWD = lambda p: [f"vpc_{p}_front_scratch", f"vpc_{p}_front_bwd"]  # noqa: E731
_ENC_FWD = {"nm": ["vpc_nm_mul"] + ["vpc_linear_fwd"] * 3 + ["vpc_nm_sample"],
            "miw": ["vpc_nm_mul"] + ["vpc_linear_fwd"] * 3 + ["vpc_miw_sample"],
            "flow": ["vpc_flow_prep"] + ["vpc_linear_fwd"] * 3 + ["vpc_flow_fwd"],
            "wide": ["vpc_nm_mul"] + ["vpc_linear_fwd"] * 3 + ["vpc_nm_sample"],
            "eddi": ["vpc_eddi_fold", "vpc_eddi_front_fwd"] + ["vpc_linear_fwd"] * 3 + ["vpc_nm_sample"],
            "eddiw": ["vpc_eddiw_fold", "vpc_eddiw_front_fwd"] + ["vpc_linear_fwd"] * 4 + ["vpc_nm_sample"]}
_DEC_FWD = {"nm": ["vpc_linear_fwd"] * 3, "miw": ["vpc_linear_fwd"] * 3 + ["vpc_miw_heads"], "flow": ["vpc_linear_fwd"] * 5,
            "wide": ["vpc_linear_fwd"] * 3, "eddi": ["vpc_decoder_fwd"], "eddiw": ["vpc_linear_fwd"] * 4}
_ENC_BWD = {"nm": ["vpc_nm_sample_bwd"] + _SWD * 2 + _SWD[:2], "miw": ["vpc_miw_sample_bwd"] + _SWD * 2 + _SWD[:2],
            "flow": ["vpc_flow_bwd"] + _SWD * 2 + _SWD[:2], "wide": ["vpc_nm_sample_bwd"] + _SWD * 2 + _SWD[:2],
            "eddi": ["vpc_nm_sample_bwd"] + _SWD * 3 + _PN_BWD("eddi"),  # (the trunk's input, the aggregate, takes a gradient)
            "eddiw": ["vpc_nm_sample_bwd"] + _SWD * 4 + _PN_BWD("eddiw")}
_DEC_BWD = {"nm": _SWD * 3, "miw": ["vpc_miw_heads_bwd"] + _SWD * 3, "flow": _SWD * 5, "wide": _SWD * 3,
            "eddi": ["vpc_decoder_bwd", "vpc_reduce_partials"], "eddiw": _SWD * 4}
_LOSS = {f: [f"vpc_{f}_loss_scratch", f"vpc_{f}_loss"] for f in ("nm", "miw", "flow")}
_LOSS.update({f: ["vpc_loss_fwd_bwd", "vpc_loss_finalize"] for f in ("wide", "eddi", "eddiw")})


def _eager_expected(f, passes, flow_order=False):
    """Forward of `passes` (encoder, decoder) pairs, the loss, then the backward of the passes from the last one down.  The
    regularised flow runs both encoders before both decoders (flow.REG_VAEFlow.forward), and autograd mirrors that; so does
    Reg_VAE.forward, which the wide dense classes and Reg_EDDI run pass by pass."""
    if flow_order:
        return _ENC_FWD[f] * 2 + _DEC_FWD[f] * 2 + _LOSS[f] + _DEC_BWD[f] * 2 + _ENC_BWD[f] * 2
    return (_ENC_FWD[f] + _DEC_FWD[f]) * passes + _LOSS[f] + (_DEC_BWD[f] + _ENC_BWD[f]) * passes


# recorded with _Recorder on the commit before the encoder / decoder Functions of a family became the one pair (the first eight
# rows before the MNAR, MIWAE and flow classes moved, the others before the wide and point-net classes did; the lists hold C ABI
# calls, host-side scratch queries included); the *_z_only rows backpropagate through the encoder's first output alone
EAGER = [
    ("REG_notMIWAE_v2", _eager_full, _eager_expected("nm", 2)),
    ("notMIWAE_myversion", _eager_full, _eager_expected("nm", 1)),
    ("Reg_MIWAE", _eager_full, _eager_expected("miw", 2)),
    ("MIWAE", _eager_full, _eager_expected("miw", 1)),
    ("REG_VAEFlow", _eager_full, _eager_expected("flow", 2, flow_order=True)),
    ("VAEFlow", _eager_full, _eager_expected("flow", 1)),
    ("Reg_MIWAE", _eager_z_only, _ENC_FWD["miw"] + _ENC_BWD["miw"]),
    ("REG_VAEFlow", _eager_z_only, _ENC_FWD["flow"] + _ENC_BWD["flow"]),
    ("Reg_VAE_d129", _eager_full, _eager_expected("wide", 2, flow_order=True)),
    ("vanilla_VAE_mask_d65", _eager_full, _eager_expected("wide", 1)),
    ("Reg_VAE_d14_L16", _eager_full, _eager_expected("wide", 2, flow_order=True)),
    ("Reg_EDDI", _eager_full, _eager_expected("eddi", 2, flow_order=True)),
    ("vanilla_EDDI", _eager_full, _eager_expected("eddi", 1)),
    ("Reg_EDDI_mnist", _eager_full, _eager_expected("eddiw", 2)),
    ("vanilla_EDDI_mnist", _eager_full, _eager_expected("eddiw", 1)),
    ("Reg_VAE_d129", _eager_z_only, _ENC_FWD["wide"] + _ENC_BWD["wide"]),
    ("Reg_EDDI", _eager_z_only, _ENC_FWD["eddi"] + _ENC_BWD["eddi"]),
    ("Reg_EDDI_mnist", _eager_z_only, _ENC_FWD["eddiw"] + _ENC_BWD["eddiw"]),
]


@pytest.mark.parametrize("name,make,expected", EAGER, ids=[f"{e[0]}_{e[1].__name__[7:]}" for e in EAGER])
def test_eager_launch_sequence(name, make, expected, monkeypatch):
    """forward_loss under grad and backward issue the C ABI calls they issued when every family had its own pair of
    autograd Functions, in the same order (second run of a model: its chains are built)."""
    run = make(name)
    run()
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    run()
    monkeypatch.undo()
    assert rec.names == expected


@pytest.mark.parametrize("n", [1, 2, 3])
def test_joined_column_blocks(n):
    """chainfamily._joined: the n adjacent column blocks of one [.., n W] buffer give that buffer back, in place; blocks of
    different buffers, a gap between blocks, a row pitch wider than n W or another dtype give None."""
    from vpc_amd.chainfamily import _joined
    B, K, W = 3, 4, 5
    buf = torch.arange(B * K * n * W, dtype=torch.float32, device="cuda").view(B, K, n * W)
    parts = [buf[..., i * W:(i + 1) * W] for i in range(n)]
    G = _joined(parts, B * K, W)
    assert G is not None and G.data_ptr() == buf.data_ptr() and torch.equal(G, buf.view(B * K, n * W))
    assert _joined([p.clone() for p in parts], B * K, W) is None or n == 1
    wide = torch.zeros(B, K, (n + 1) * W, device="cuda")
    assert _joined([wide[..., i * W:(i + 1) * W] for i in range(n)], B * K, W) is None
    assert _joined([p.double() for p in parts], B * K, W) is None
    if n > 1:
        assert _joined(parts[::-1], B * K, W) is None
        assert _joined([buf[:, 0, i * W:(i + 1) * W] for i in range(n)], B, W) is None  # rows K * n W apart


def test_nm_encoder_one_output_gradient():
    """Backpropagation through z alone (no gradient arrives for the heads) gives the encoder gradients of the two-output run
    whose heads gradient is zero, bit for bit."""
    model = _eager_model("REG_notMIWAE_v2")
    x, m, _ = _eager_data()
    grads = []
    for both in (False, True):
        model.zero_grad()
        torch.manual_seed(1)
        z, mean, _ = model.encoder(x, m)
        if both:
            torch.autograd.backward([z, mean], [torch.ones_like(z), torch.zeros_like(mean)])
        else:
            z.sum().backward()
        grads.append([p.grad.clone() for p in model.seq_encoder.parameters()] + [model.q_mu[0].weight.grad.clone(),
                                                                                  model.q_logstd[0].bias.grad.clone()])
    assert all(g.abs().max() > 0 for g in grads[0])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


@pytest.mark.parametrize("name", ["Reg_VAE_d129", "Reg_EDDI", "Reg_EDDI_mnist"])
def test_encoder_one_output_gradient(name):
    """The same for a wide dense class and a point-net class of either width: every parameter the encoder reads, the point-net
    front-end's four tensors included, gets the two-output run's gradient, bit for bit."""
    model = _eager_model(name)
    x, m, _ = _eager_data(name)
    grads = []
    for both in (False, True):
        model.zero_grad()
        torch.manual_seed(1)
        z, mean, _ = model.encoder(x, m)
        if both:
            torch.autograd.backward([z, mean], [torch.ones_like(z), torch.zeros_like(mean)])
        else:
            z.sum().backward()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    want = {k for k, p in model.named_parameters() if p.requires_grad and not k.startswith("seq_decoder")}
    assert set(grads[0]) == set(grads[1]) == want
    assert all(g.abs().max() > 0 for g in grads[0].values())
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in want)


def _reg_vae(B):
    return vpc.Reg_VAE(128, 500, 10, 10, {"batch_size": B, "patience": 1}, "exp", "kl_reg").cuda()


@pytest.mark.parametrize("write", ["torch", "data", "load_state_dict"])
def test_fused_bf16_whole_step_follows_outside_writes(write, monkeypatch):
    """FusedTrainer(precision="bf16") on the whole-step kernel: a parameter write between steps reaches the compact bf16
    image - through the version counters (`p.mul_()` under no_grad, load_state_dict) or through invalidate_image() (a
    `.data` write).  The steps that follow are bit-equal to those of a fresh trainer built on the written weights with
    the same optimiser state."""
    monkeypatch.setenv("VPC_TILE", "128")
    B = 300
    x, mk = _data(B, 128, 4)
    kw = dict(alpha=0.9, beta=0.8)
    torch.manual_seed(0)
    m = _reg_vae(B)
    tr = vpc.FusedTrainer(m, seed=3, precision="bf16")
    for _ in range(3):
        tr.step(x, mk, **kw)
    assert tr._used_step_fused
    before = m._flat.clone()
    if write == "torch":
        with torch.no_grad():
            m.seq_decoder[2].weight.mul_(0.5)
    elif write == "data":
        m.seq_encoder[0].weight.data.mul_(0.5)
        tr.invalidate_image()
    else:
        sd = m.state_dict()
        sd["seq_decoder.4.weight"] = sd["seq_decoder.4.weight"] * 0.5
        m.load_state_dict(sd)
    assert not torch.equal(before, m._flat)
    m2 = _reg_vae(B)
    m2.load_state_dict(m.state_dict())
    tr2 = vpc.FusedTrainer(m2, seed=3, precision="bf16")
    tr2.exp_avg.copy_(tr.exp_avg)
    tr2.exp_avg_sq.copy_(tr.exp_avg_sq)
    tr2.step_count, tr2.rng_offset = tr.step_count, tr.rng_offset
    for i in range(3):
        tr.step(x, mk, **kw)
        tr2.step(x, mk, **kw)
        assert tr.loss_value() == tr2.loss_value(), (write, i)
    assert torch.equal(m._flat, m2._flat)
    assert torch.equal(tr.exp_avg_sq, tr2.exp_avg_sq)


def test_trainers_are_freed_by_reference_count(monkeypatch):
    """No trainer sits in a reference cycle (the images' pack functions hold none): one that holds a captured graph goes
    when its last reference does, not in a garbage collection that may run while another graph is being captured."""
    monkeypatch.setenv("VPC_TILE", "128")
    x, mk = _data(300, 128, 4)
    for prec in ("f32", "bf16"):
        tr = vpc.FusedTrainer(_reg_vae(300), seed=3, precision=prec)
        for _ in range(2):
            tr.step_graph(x, mk)
        ref = weakref.ref(tr)
        del tr
        assert ref() is None, prec
    xf, mf = _data(96, 128, 5, float_mask=True)
    for prec in ("f32", "bf16"):
        tr = nm.NMTrainer(nm.REG_notMIWAE_v2(128, 128, 10, 10, {"batch_size": 96, "patience": 1}, 20, 1).cuda(),
                          precision=prec)
        tr.step(xf, mf)
        for _ in range(2):
            tr.step_graph(xf, mf)
        ref = weakref.ref(tr)
        del tr
        assert ref() is None, prec
