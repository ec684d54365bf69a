"""FlatParams (images.py), the one flat-buffer mixin under every model class: buffer size and aliasing, idempotence, the
re-flatten after a parameter's storage is replaced, state_dict keys, and the named views of each segment.  The literal key
lists and name -> shape tables below were written from the per-class code this mixin replaced (layer sizes of the reference:
VAE 100 / 50, EDDI point-net K -> 100 -> 50, MNIST 500 / 500 / 200, MNAR and MIWAE 128, flow hid_dim and 100 contexts).
CPU only: models are built, nothing is launched."""
import pytest
import torch

import vpc_amd as vpc
from vpc_amd import notmiwae as nm

TP = {"batch_size": 8, "patience": 1}
D, L, K, H = 6, 10, 4, 16  # obs_dim, latent_dim, EDDI emb_dim, flow hid_dim


def _lin(prefix, idx):
    return [f"{prefix}.{i}.{k}" for i in idx for k in ("weight", "bias")]


def _mlp(names, dims):
    """{W1: (out, in), b1: (out,), ..} for names = (W1, b1, ..) and dims = [(in, out), ..]."""
    out = {}
    for (w, b), (k, n) in zip(zip(names[0::2], names[1::2]), dims):
        out[w], out[b] = (n, k), (n,)
    return out


VAE_KEYS = ["prior_mean", "prior_std"] + _lin("seq_encoder", (0, 2, 4)) + _lin("seq_decoder", (0, 2, 4))
EDDI_KEYS = ["type_pars1", "type_bias1", "prior_mean", "prior_std"] + _lin("pnp_encoder1", (0,)) + \
    _lin("pnp_encoder2", (0, 2, 4)) + _lin("seq_decoder", (0, 2, 4))
MNIST_KEYS = ["type_pars1", "type_bias1", "prior_mean", "prior_std"] + _lin("pnp_encoder1", (0,)) + \
    _lin("pnp_encoder2", (0, 2, 4, 6)) + _lin("seq_decoder", (0, 2, 4, 6))
NM_KEYS = ["W", "b"] + _lin("seq_encoder", (0, 2)) + _lin("q_mu", (0,)) + _lin("q_logstd", (0,)) + \
    _lin("seq_decoder", (0, 2)) + _lin("x_mean", (0,)) + _lin("x_logvar", (0,))
MIW_KEYS = _lin("seq_encoder", (0, 2, 4)) + _lin("seq_decoder", (0, 2, 4))
FLOW_KEYS = ["prior_mean", "prior_std"] + [f"flow.flows.{i}.unnormalized_pdf" for i in range(3)] + \
    _lin("seq_encoder", (0, 2, 4)) + ["encoder_mean.weight", "encoder_mean.bias", "encoder_logvar.weight",
                                      "encoder_logvar.bias"] + _lin("seq_decoder", (0, 2, 4, 6)) + \
    _lin("decoder_mean", (0,)) + _lin("decoder_logvar", (0,))

W6 = ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "W5", "b5", "W6", "b6")
NM_ENC = {"We1": (128, D), "be1": (128,), "We2": (128, 128), "be2": (128,), "Wmu": (L, 128), "Wls": (L, 128), "bmu": (L,),
          "bls": (L,), "Wh": (2 * L, 128), "bh": (2 * L,)}
NM_DEC = {"Wd1": (128, L), "bd1": (128,), "Wd2": (128, 128), "bd2": (128,), "Wxm": (D, 128), "Wxl": (D, 128), "bxm": (D,),
          "bxl": (D,), "Wx": (2 * D, 128), "bx": (2 * D,)}
NM_VIEWS = {"wb": {"W": (D,), "b": (D,)}, "enc": NM_ENC, "dec": NM_DEC}
FRONT = {"E": (D, K), "tb": (D, 1), "Wp": (K, 2 + K), "cp": (K,)}
E4 = ("We1", "be1", "We2", "be2", "We3", "be3", "We4", "be4")
D4 = ("Wd1", "bd1", "Wd2", "bd2", "Wd3", "bd3", "Wd4", "bd4")

# (id, factory, state_dict keys, {segment: {name: shape}} in flat order)
CASES = [
    ("Reg_VAE", lambda: vpc.Reg_VAE(D, 500, 10, L, TP, "e", "kl_reg"), VAE_KEYS,
     {"enc": _mlp(W6[:6], [(D, 100), (100, 50), (50, 2 * L)]), "dec": _mlp(W6[6:], [(L, 50), (50, 100), (100, D)])}),
    ("vanilla_VAE_mask", lambda: vpc.vanilla_VAE_mask(D, 500, 10, L, TP, "e"), VAE_KEYS,
     {"enc": _mlp(W6[:6], [(2 * D, 100), (100, 50), (50, 2 * L)]), "dec": _mlp(W6[6:], [(L, 50), (50, 100), (100, D)])}),
    ("Reg_EDDI", lambda: vpc.Reg_EDDI(D, 500, K, L, TP, "e", "kl_reg"), EDDI_KEYS,
     {"enc": _mlp(W6[:6], [(K, 100), (100, 50), (50, 2 * L)]), "dec": _mlp(W6[6:], [(L, 50), (50, 100), (100, D)]),
      "front": FRONT}),
    ("Reg_EDDI_mnist", lambda: vpc.Reg_EDDI_mnist(D, 500, K, L, TP, "e", "kl_reg"), MNIST_KEYS,
     {"front": FRONT, "enc": _mlp(E4, [(K, 500), (500, 500), (500, 200), (200, 2 * L)]),
      "dec": _mlp(D4, [(L, 200), (200, 500), (500, 500), (500, D)])}),
    ("REG_notMIWAE_v2", lambda: nm.REG_notMIWAE_v2(D, 128, 10, L, TP, 3, 1), NM_KEYS + ["logits.0.weight", "logits.0.bias"],
     NM_VIEWS),
    ("notMIWAE_myversion", lambda: nm.notMIWAE_myversion(D, 128, 10, L, TP, 3, 1), NM_KEYS, NM_VIEWS),
    ("Reg_MIWAE", lambda: vpc.Reg_MIWAE(D, 500, 10, L, TP, 3, 1), MIW_KEYS,
     {"enc": _mlp(("We1", "be1", "We2", "be2", "Wh", "bh"), [(D, 128), (128, 128), (128, 2 * L)]),
      "dec": _mlp(("Wd1", "bd1", "Wd2", "bd2", "Wx", "bx"), [(L, 128), (128, 128), (128, 3 * D)])}),
    ("REG_VAEFlow", lambda: vpc.REG_VAEFlow(D, H, 10, L, TP), FLOW_KEYS,
     {"enc": _mlp(("We1", "be1", "We2", "be2", "We3", "be3"), [(2 * D, H), (H, H), (H, 100)]),
      "dec": _mlp(D4 + ("Wm", "bm"), [(L, H), (H, H), (H, H), (H, H), (H, D)])}),
]
# names that join adjacent entries into one GEMM operand: not tensors of their own
ALIASES = {"Wh": ("Wmu", "Wls"), "bh": ("bmu", "bls"), "Wx": ("Wxm", "Wxl"), "bx": ("bxm", "bxl")}


@pytest.mark.parametrize("name,make,keys,views", CASES, ids=[c[0] for c in CASES])
def test_flat_buffer(name, make, keys, views):
    torch.manual_seed(0)
    m = make()
    assert [k for k in m.state_dict()] == keys
    before = [p.detach().clone() for p in m.trainable()]
    flat = m.flatten_parameters()
    ps = m.trainable()
    assert flat.numel() == sum(p.numel() for p in ps)
    assert [k for k in m.state_dict()] == keys
    off = 0
    for i, (p, b) in enumerate(zip(ps, before)):  # every trainable tensor aliases its slice
        assert torch.equal(p, b)
        with torch.no_grad():
            p.reshape(-1)[0] = 1000.0 + i
        assert flat[off].item() == 1000.0 + i
        off += p.numel()
    assert m.flatten_parameters() is flat  # idempotent
    if name == "REG_VAEFlow":  # the tensors that never get a gradient stay outside the buffer
        inside = {p.data_ptr() for p in ps}
        outside = [p for p in m.parameters() if p.data_ptr() not in inside]
        assert len(outside) == 11 and len(ps) == 16
    # replacing a parameter's storage (what .to() / re-assignment do to all of them; the steady-state check looks at the first
    # and the last): the next call builds a new buffer with equal contents and drops the packed images
    for i in (len(ps) - 1, 0):
        gen, old = m._img_gen, m.flatten_parameters()
        ps[i].data = ps[i].data.clone()
        flat2 = m.flatten_parameters()
        assert flat2 is not old and torch.equal(flat2, flat) and m._img_gen > gen
        assert m.flatten_parameters() is flat2
        assert ps[i].data_ptr() == flat2.data_ptr() + 4 * sum(p.numel() for p in ps[:i])
    # the named views of every segment, on a plain CPU buffer laid out like the flat one
    buf = torch.arange(flat2.numel(), dtype=torch.float32)
    lo = 0
    for which, table in views.items():
        joined = {k: parts for k, parts in ALIASES.items() if parts[0] in table}  # (MIWAE's Wh / Wx are tensors of their own)
        n = sum(torch.Size(s).numel() for k, s in table.items() if k not in joined)
        v = m._segment_views(buf[lo:lo + n], which)
        assert {k: tuple(t.shape) for k, t in v.items()} == table
        o = lo
        for k, shp in table.items():
            if k not in joined:
                assert torch.equal(v[k].reshape(-1), buf[o:o + v[k].numel()])
                o += v[k].numel()
        for k, (a, b) in joined.items():
            if k in table:
                assert torch.equal(v[k], torch.cat([v[a], v[b]], 0)) and v[k].data_ptr() == v[a].data_ptr()
        lo += n
    assert lo == flat2.numel()
    with pytest.raises(vpc._lib.VpcError):  # no CPU fallback: the parameter views are for the kernels
        m._views()
