"""The trainers' device draws, pinned to the draw-counter rule ("The draw-counter rule") with every Philox
offset written out as a literal.

After each of two consecutive steps the trainer's mask_p buffer and the consumed planes of its eps buffer must hold, bit
for bit, what ops.draw_step (ops.draw_mask / ops.fill_normal where only one kind is drawn) produces from the same seed at
the literal offsets, and the trainer's rng_offset must equal the literal total.  A mask draw over n = B_global * row_width
elements takes (n + 7) // 8 + 1 counters and comes first; the eps planes take planes * B_global * (pitch // 4)."""
import pytest
import torch

import vpc_amd as vpc
from vpc_amd import eddi_mnist as em
from vpc_amd import ops

pytestmark = pytest.mark.gpu
L = 10
TP = {"batch_size": 64, "patience": 100}
DEV = "cuda"
KEEP = 0.7  # 1 - p_missingness / 100 at the default p_missingness = 30


def data(B, d, seed=0, lead=()):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*lead, B, d, generator=g)
    mask = torch.rand(*lead, B, d, generator=g) < 0.7
    return x.to(DEV), mask.to(DEV)


def padded_u8(mask, dk):
    """The mask as the step's kernels see it: 0 / 1 bytes, zero columns up to dk."""
    out = torch.zeros(*mask.shape[:-1], dk, dtype=torch.uint8, device=mask.device)
    out[..., :mask.shape[-1]] = mask.to(torch.uint8)
    return out


def expected(mask_u8, planes, B, pitch, seed, off_mask, off_eps):
    """(mask_p, eps) of the stand-alone draw launches at the given offsets (None: that kind is not drawn)."""
    mp = torch.empty_like(mask_u8) if off_mask is not None else None
    eps = torch.empty(planes, B, pitch, device=DEV) if off_eps is not None else None
    shard = (B, B, 0, pitch)
    if mp is not None and eps is not None:
        ops.draw_step(mask_u8, mp, KEEP, eps, seed, off_mask, off_eps, None, 0, shard)
    elif mp is not None:
        ops.draw_mask(mask_u8, mp, KEEP, seed, off_mask, 0)
    else:
        ops.fill_normal(eps, seed, off_eps, None, shard)
    return mp, eps


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check(got_mask, got_eps, mask_u8, planes, B, pitch, seed, off_mask, off_eps, what):
    mp, eps = expected(mask_u8, planes, B, pitch, seed, off_mask, off_eps)
    if mp is not None:
        assert torch.equal(got_mask, mp), (what, "mask_p")
    if eps is not None:
        assert same_bits(got_eps[:planes], eps), (what, "eps")


# (reg_type or None for vanilla, d, dk, planes, epoch, [(offset_mask, offset_eps, rng_offset after the step)] for two steps)
FUSED_B48 = {
    # mask (48 * 16 + 7) // 8 + 1 = 97, eps 2 * 48 * 4 = 384
    "kl_d13": ("kl_reg", 13, 16, 2, 1, [(0, 97, 481), (481, 578, 962)]),
    # mask (48 * 12 + 7) // 8 + 1 = 73, eps 384
    "kl_d12": ("kl_reg", 12, 12, 2, 1, [(0, 73, 457), (457, 530, 914)]),
    # wml != 0: the third plane, eps 3 * 48 * 4 = 576
    "ml_d12": ("ml_reg", 12, 12, 3, 1400, [(0, 73, 649), (649, 722, 1298)]),
    # no mask draw, one plane: eps 48 * 4 = 192
    "van_d12": (None, 12, 12, 1, 1, [(None, 0, 192), (None, 192, 384)]),
}
# B = 4112: mask (4112 * 16 + 7) // 8 + 1 = 8225 / (4112 * 12 + 7) // 8 + 1 = 6169, eps 2 * 4112 * 4 = 32896
FUSED_LARGE = {
    "kl_d13": ("kl_reg", 13, 16, 2, 1, [(0, 8225, 41121), (41121, 49346, 82242)]),
    "kl_d12": ("kl_reg", 12, 12, 2, 1, [(0, 6169, 39065), (39065, 45234, 78130)]),
}


def fused_model(rt, d):
    torch.manual_seed(0)
    m = vpc.Reg_VAE(d, 500, 10, L, TP, "exp", rt) if rt else vpc.vanilla_VAE(d, 500, 10, L, TP, "exp")
    return m.to(DEV)


def run_fused(case, B, seed=5):
    rt, d, dk, planes, epoch, steps = case
    tr = vpc.FusedTrainer(fused_model(rt, d), seed=seed)
    x, mask = data(B, d)
    mu8 = padded_u8(mask, dk)
    for i, (om, oe, total) in enumerate(steps):
        tr.step(x, mask, epoch=epoch)
        check(tr.mask_p_buf if rt else None, tr.eps_buf, mu8, planes, B, 16, seed, om, oe, f"step {i}")
        assert tr.rng_offset == total, (i, tr.rng_offset)
    return tr


@pytest.mark.parametrize("name", list(FUSED_B48))
def test_fused_in_kernel_draw(name):
    """B = 48: the N-split step makes its draws inside the launch."""
    assert ops.step_small_max_rows() >= 48
    tr = run_fused(FUSED_B48[name], 48)
    assert tr.dominant_launch() == "step_small"


@pytest.mark.parametrize("name", list(FUSED_LARGE))
def test_fused_separate_draw_launch(name):
    """B = step_small_max_rows() + 16 (4112 on the MI355X's 256 CUs): the vpc_draw_step launch in front of the row-tiled kernels."""
    B = ops.step_small_max_rows() + 16
    assert B == 4112, "the literal offsets of this test are those of 16 x 256 CUs + 16 rows"
    tr = run_fused(FUSED_LARGE[name], B)
    assert tr.dominant_launch() == "decoder_fused"


def test_fused_mask_injected_eps_drawn():
    B, d, seed = 48, 12, 5
    tr = vpc.FusedTrainer(fused_model("kl_reg", d), seed=seed)
    x, mask = data(B, d)
    mask_p = mask & (torch.rand(B, d, device=DEV) < 0.7)
    for i, (oe, total) in enumerate([(0, 384), (384, 768)]):
        tr.step(x, mask, mask_p)
        check(None, tr.eps_buf, None, 2, B, 16, seed, None, oe, f"step {i}")
        assert tr.rng_offset == total, (i, tr.rng_offset)


def test_fused_eps_injected_mask_drawn():
    B, d, seed = 48, 12, 5
    tr = vpc.FusedTrainer(fused_model("kl_reg", d), seed=seed)
    x, mask = data(B, d)
    eq, ep = torch.randn(B, L, device=DEV), torch.randn(B, L, device=DEV)
    for i, (om, total) in enumerate([(0, 73), (73, 146)]):
        tr.step(x, mask, None, eq, ep)
        check(tr.mask_p_buf, None, padded_u8(mask, d), 2, B, 16, seed, om, None, f"step {i}")
        assert tr.rng_offset == total, (i, tr.rng_offset)


def test_eddi_trainer():
    """d = 14 is not padded on this path: mask (48 * 14 + 7) // 8 + 1 = 85, eps 2 * 48 * 4 = 384."""
    B, d, seed = 48, 14, 5
    torch.manual_seed(0)
    tr = vpc.EDDITrainer(vpc.Reg_EDDI(d, 500, 10, L, TP, "exp", "kl_reg").to(DEV), seed=seed)
    x, mask = data(B, d)
    for i, (om, oe, total) in enumerate([(0, 85, 469), (469, 554, 938)]):
        tr.step(x, mask)
        check(tr.mask_p_buf, tr.eps_buf, padded_u8(mask, d), 2, B, 16, seed, om, oe, f"step {i}")
        assert tr.rng_offset == total, (i, tr.rng_offset)


def test_eddi_mnist_trainer():
    """Always three planes at pitch 4 * ceil(10 / 4) = 12: mask (16 * 784 + 7) // 8 + 1 = 1569, eps 3 * 16 * 3 = 144."""
    B, d, seed = 16, 784, 5
    torch.manual_seed(0)
    tr = em.EDDIMnistTrainer(em.Reg_EDDI_mnist(d, 500, 20, L, TP, "exp", "kl_reg").to(DEV), seed=seed)
    x, mask = data(B, d)
    for i, (om, oe, total) in enumerate([(0, 1569, 1713), (1713, 3282, 3426)]):
        tr.step(x, mask)
        # two launches on this path (draw_mask, then fill_normal): the same counters as the one draw_step launch
        check(tr.mask_p_buf, tr.eps_pad, padded_u8(mask, d), 3, B, 12, seed, om, oe, f"step {i}")
        assert tr.rng_offset == total, (i, tr.rng_offset)


def test_ensemble_trainer():
    """Every member draws with its own seed at the shared offsets: mask 73, eps 384 as the stand-alone step at B = 48, d = 12."""
    G, B, d, seeds = 2, 48, 12, (3, 7)
    assert ops.step_small_max_rows() >= B
    torch.manual_seed(0)
    ms = [vpc.Reg_VAE(d, 500, 10, L, TP, "exp", "kl_reg").to(DEV) for _ in range(G)]
    ens = vpc.EnsembleTrainer(ms, seeds=seeds)
    x, mask = data(B, d, lead=(G,))
    for i, (om, oe, total) in enumerate([(0, 73, 457), (457, 530, 914)]):
        ens.step(x, mask)
        for g in range(G):
            check(ens.mask_p_buf[g], ens.eps_buf[g], padded_u8(mask[g], d), 2, B, 16, seeds[g], om, oe, f"step {i} member {g}")
        assert ens.rng_offset == total, (i, ens.rng_offset)
