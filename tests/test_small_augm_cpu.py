"""Host arithmetic of the small-batch one-kernel step of the mask-augmented classes (Reg_VAE_mask / vanilla_VAE_mask at
B <= ops.step_small_max_rows(): vpc_step_small_aug_f32 / vpc_step_small_aug_draw_f32).  No GPU: the pitch rule, the kernel
instantiation chosen per obs_dim, the refusals of the C entries (made before any launch) and the wide models' routing."""
import ctypes

import pytest

import vpc_amd as vpc
from vpc_amd import harness, ops
from vpc_amd.trainer import padded_width

L = 10
TP = {"batch_size": 64, "patience": 1}
OK, ERR_ARG, ERR_SHAPE = 0, 1, 2


@pytest.mark.parametrize("d", [1, 3, 4, 5, 8, 12, 13, 14, 16, 33, 63, 64])
def test_pitch_rule(d):
    """x / mask / mask_p rows of the new path are padded to 4 * ceil(d / 4) columns, the plain models' rule; padded_width keeps
    describing the row-tiled path of the mask-augmented classes, which takes its rows unpadded."""
    assert ops.small_aug_pitch(d) == 4 * -(-d // 4) == padded_width(d, False)
    assert 0 <= ops.small_aug_pitch(d) - d <= 3 and ops.small_aug_pitch(d) % 4 == 0
    assert padded_width(d, True) == d


@pytest.mark.parametrize("d,pair", [(1, (1, 1)), (8, (1, 1)), (9, (2, 1)), (16, (2, 1)), (17, (4, 2)), (32, (4, 2)),
                                    (33, (8, 4)), (64, (8, 4))])
def test_tile_pair(d, pair):
    """(encoder-input tiles, decoder-output tiles) of the instantiation that serves obs_dim d - and the weight images of the
    mask-augmented layout have exactly that geometry: W1 rows of 64 dwords up to 4 input tiles and 128 above, W6 of 16 DT rows."""
    assert ops.small_aug_tiles(d) == pair
    dti, dt = pair
    lay = vpc._lib.layout(d, L, True)
    assert lay.enc_img == 112 * (128 if dti > 4 else 64) + 128 + 64 * 128 + 32 * 64
    assert lay.dec_img == 64 * 16 + 112 * 64 + 16 * dt * 128


def test_wide_models_never_reach_the_new_entries():
    assert ops.small_aug_tiles(65) is None and ops.small_aug_tiles(0) is None
    for m in (vpc.Reg_VAE_mask(65, 500, 10, L, TP, "e", "kl_reg"), vpc.vanilla_VAE_mask(65, 500, 10, L, TP, "e")):
        assert m._wide
        assert harness.trainer_class_for(m) is vpc.WideTrainer
        with pytest.raises(vpc.VpcError):
            vpc.FusedTrainer(m)
    assert not vpc.Reg_VAE_mask(64, 500, 10, L, TP, "e", "kl_reg")._wide


def test_c_entries_refuse_before_any_launch():
    """Host buffers and no device: every refusal is returned by the argument checks."""
    l = vpc._lib.lib()
    host = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(host))
    ptrs = (ctypes.c_void_p * 2)(p.value, p.value)
    co = vpc._lib.VpcLossCoef([1.0], [0.0], 1.0)
    nb = ctypes.byref(ctypes.c_int())

    def both(d, d_real, x=p, coef=co):
        head = (x, p, p, 1, ptrs, None, coef, ptrs, None, 1.0, 0.0, p, p, p, nb, 16, d, d_real, L)
        a = l.vpc_step_small_aug_f32(*head, None)
        b = l.vpc_step_small_aug_draw_f32(*head, None, 0.7, p, 256, 0, 0, 0, None, 0, 16, 16, 0, 16, None)
        assert a == b
        return a

    assert both(16, 0) == ERR_SHAPE      # d_real < 1
    assert both(12, 13) == ERR_SHAPE     # d_real > d
    assert both(16, 12) == ERR_SHAPE     # d - d_real > 3
    assert both(14, 14) == ERR_SHAPE     # d % 4 != 0
    assert both(68, 65) == ERR_SHAPE     # 2 * d_real > 128
    assert both(16, 14, x=ctypes.c_void_p(p.value + 4)) == ERR_ARG   # x not 16-byte aligned
    assert both(16, 14, x=None) == ERR_ARG
    assert both(16, 14, coef=None) == ERR_ARG
