"""The loss-coefficient record (VpcLossCoef of include/vpc.h, _lib.VpcLossCoef) and the draw-counter rule
(trainer.draw_counters): layouts, bytes and counters against literal numbers.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import vpc_amd as vpc
from vpc_amd import ensemble as E
from vpc_amd._lib import VpcLossCoef
from vpc_amd.fused import loss_coefficients
from vpc_amd.trainer import draw_counters

TP = {"batch_size": 64, "patience": 100}


def test_record_layout():
    assert ctypes.sizeof(VpcLossCoef) == 32
    offs = {name: getattr(VpcLossCoef, name).offset for name, _ in VpcLossCoef._fields_}
    assert offs == dict(cA=0, cE=8, bq=16, bp=20, cr=24, wml=28)


def test_member_row_layout():
    assert E.MEMBER_DTYPE.itemsize == 64
    offs = {k: E.MEMBER_DTYPE.fields[k][1] for k in ("cA", "cE", "bq", "bp", "cr", "wml", "keep_prob", "lr", "seed", "use_maskB")}
    assert offs == dict(cA=0, cE=8, bq=16, bp=20, cr=24, wml=28, keep_prob=32, lr=36, seed=40, use_maskB=48)


def model(kind):
    if kind == "vanilla":
        return vpc.vanilla_VAE(14, 500, 10, 10, TP, "exp")
    return vpc.Reg_VAE(14, 500, 10, 10, TP, "exp", kind)


# (kind, epoch, alpha, beta, beta_annealing) -> cA, cE, bq, bp, cr, wml; 2800 = MAX_EPOCH
VALUES = [
    (("kl_reg", 3, 0.5, 0.7, False), ([0.5, 0.5], [0.5, 0.0], 0.35, 0.35, 0.5, 0.0)),
    (("kl_reg", 1400, 0.8, 0.6, True), ([1.0 - 0.8, 0.8], [0.8, 0.0], (1.0 - 0.8) * 0.3, 0.8 * 0.3, 0.8, 0.0)),
    (("ml_reg", 1400, 0.5, 0.7, False), ([1.0, 0.0], [0.0, 0.0], 0.7, 0.0, 0.0, 0.25)),
    (("ml_reg", 700, 0.5, 1.0, True), ([1.0, 0.0], [0.0, 0.0], 0.25, 0.0, 0.0, 0.125)),
    (("vanilla", 5, 0.5, 0.7, False), ([1.0, 0.0], [0.0, 0.0], 0.7, 0.0, 0.0, 0.0)),
    (("vanilla", 1400, 0.5, 0.7, True), ([1.0, 0.0], [0.0, 0.0], 0.35, 0.0, 0.0, 0.0)),
]


@pytest.mark.parametrize("args,want", VALUES)
def test_coefficients_against_literals(args, want):
    co = loss_coefficients(model(args[0]), *args[1:])
    got = np.frombuffer(bytes(co), np.float32)
    cA, cE, bq, bp, cr, wml = want
    assert np.array_equal(got, np.array(cA + cE + [bq, bp, cr, wml], np.float32))
    assert co.ml_on == (wml != 0.0) and co.maskB_on == (cE[0] != 0.0)
    assert loss_coefficients(model(args[0]), *args[1:]) is co  # one record per distinct set of hyperparameters


@pytest.mark.parametrize("kind,epoch", [("kl_reg", 3), ("ml_reg", 1400), ("vanilla", 5)])
@pytest.mark.parametrize("annealing", [False, True])
def test_record_bytes_are_the_head_of_the_member_row(kind, epoch, annealing):
    ms = [model(kind) for _ in range(3)]
    alphas, betas = (1.0, 0.5, 0.8), (1.0, 0.7, 0.9)
    t = E.MemberTable(ms, 1e-3, (1, 2, 3))
    t.update(epoch, alphas, betas, annealing, (30, 50, 10))
    raw = t.rows.view(np.uint8).reshape(3, 64)
    for g, m in enumerate(ms):
        co = loss_coefficients(m, epoch, alphas[g], betas[g], annealing)
        assert (kind == "ml_reg") == (co.wml != 0.0)
        assert raw[g, :32].tobytes() == bytes(co)


def test_draw_counters_against_literals():
    # B = Bg = 64, dk = 16, pitch 16, 2 planes, mask drawn: (64 * 16 + 7) // 8 + 1 = 129, then 2 * 64 * 4 = 512
    dr = draw_counters(0, True, 2, 64, 64, 0, 16, 16)
    assert (dr.offset_mask, dr.offset_eps, dr.next_offset) == (0, 129, 641)
    assert dr.elem_lo == 0 and dr.eps_shard == (64, 64, 0, 16)
    # the same without a mask draw
    dr = draw_counters(0, False, 2, 64, 64, 0, 16, 16)
    assert (dr.offset_mask, dr.offset_eps, dr.next_offset) == (0, 0, 512)
    # the second half of a global batch of 128, dk = 12: (128 * 12 + 7) // 8 + 1 = 193
    dr = draw_counters(1000, True, 2, 64, 128, 64, 16, 12)
    assert (dr.offset_mask, dr.offset_eps, dr.next_offset) == (1000, 1193, 1193 + 2 * 128 * 4)
    assert dr.elem_lo == 768 and dr.eps_shard == (64, 128, 64, 16)
    # 3 planes at pitch 12, B = 16 (the EDDI-mnist form): 3 * 16 * 3 = 144
    dr = draw_counters(7, False, 3, 16, 16, 0, 12, 784)
    assert (dr.offset_eps, dr.next_offset - dr.offset_eps) == (7, 144)
    # only mask_p is drawn
    dr = draw_counters(5, True, 0, 48, 48, 0, 16, 12)
    assert (dr.offset_mask, dr.offset_eps, dr.next_offset) == (5, 78, 78)


def test_rows_outside_the_global_batch_are_refused():
    from vpc_amd.trainer import _FlatAdamTrainer
    tr = _FlatAdamTrainer.__new__(_FlatAdamTrainer)
    tr.world_size, tr.rank = 2, 1
    assert tr._batch_rows(64) == (128, 64)
    assert tr._batch_rows(64, 256, 100) == (256, 100)
    for gb, lo in ((64, None), (128, 65), (128, -1)):
        with pytest.raises(ValueError, match="global batch"):
            tr._batch_rows(64, gb, lo)
