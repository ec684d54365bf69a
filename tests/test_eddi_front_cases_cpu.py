"""Soundness of tests/eddi_front_cases.py (no GPU): the cases reach every instantiation of the narrow front-end's backward kernel
and both sides of every boundary of its dispatch, the STRIDE row count makes the grid-stride loops iterate as the GPU test
says, the near-kink entries taken out of the masks are few, and fp32 arithmetic on these inputs (the reference's own unfolded
expression in fp32 torch, with autograd) stays under one fifth of the bound the GPU test holds the kernels to - so inputs and
float64 oracle alone sit well inside it and the rest is the kernels' own summation order."""
import numpy as np
import pytest

import eddi_front_cases as fc


def test_variant_restates_the_dispatch():
    assert fc.variant(1, 1) == (1, 10) and fc.variant(64, 10) == (1, 10) and fc.variant(65, 10) == (2, 10)
    assert fc.variant(64, 11) == (1, 16) and fc.variant(64, 16) == (1, 16) and fc.variant(64, 17) == (1, 20)
    assert fc.variant(128, 20) == (2, 20) and fc.variant(128, 21) == (2, 32) and fc.variant(128, 32) == (2, 32)
    for bad in ((0, 10), (129, 10), (14, 0), (14, 33)):
        with pytest.raises(ValueError):
            fc.variant(*bad)


def test_cases_reach_every_instantiation_and_boundary():
    assert {fc.variant(d, K) for d, K in fc.STRIDE} == fc.VARIANTS and len(fc.STRIDE) == len(fc.VARIANTS) == 8
    assert {fc.variant(d, K) for d, K, *_ in fc.EDGE} == fc.VARIANTS
    shapes = {(d, K) for d, K, *_ in fc.EDGE}
    assert shapes == set(fc.EDGE_SHAPES)
    for K in fc.EDGE_K:  # both sides of the T boundary at every K
        assert (64, K) in shapes and (65, K) in shapes and fc.variant(64, K)[0] == 1 and fc.variant(65, K)[0] == 2
    for lo, hi in ((10, 11), (16, 17), (20, 21)):  # both sides of every KP boundary at every d
        for d in fc.EDGE_D:
            assert (d, lo) in shapes and (d, hi) in shapes and fc.variant(d, lo)[1] < fc.variant(d, hi)[1]
    # K strictly inside a bucket (rows of the accumulators masked off by k < K) in every bucket, both T
    for T, d in ((1, 63), (2, 127)):
        inside = {fc.variant(d, K)[1] for K in fc.EDGE_K if K not in fc.KPS and fc.variant(d, K)[0] == T}
        assert inside == set(fc.KPS)
    for d, K in fc.EDGE_SHAPES:  # every sub-case of every shape, one of them with normal x
        sub = [(B, two, xd) for d_, K_, B, two, xd in fc.EDGE if (d_, K_) == (d, K)]
        assert sorted((B, two) for B, two, _ in sub) == sorted((B, two) for B in fc.EDGE_B for two in (False, True))
        assert [xd for _, _, xd in sub].count("normal") == 1


@pytest.mark.parametrize("cus", [fc.CPU_CUS, 304, 64])
def test_stride_rows_iterate_the_loops(cus):
    B = fc.stride_rows(cus)
    assert B % (24 * cus) == 3 and B % (12 * cus) == 3
    assert fc.loop_trips(B, cus) == ((1, 2), (2, 3))       # one mask: forward 1 - 2 rows per wave, backward 2 - 3
    assert fc.loop_trips(2 * B, cus) == ((2, 3), (4, 5))   # stacked
    # stacked: wave w walks rows w, w + W, ...: every wave has rows of both passes, and the pass boundary B is no multiple of W
    # (B >= the wave count, so every wave has a row below B and one of the B >= waves consecutive rows from B on)
    for waves in (24 * cus, 12 * cus):
        assert B >= waves and B % waves != 0
    # the largest row count a test gave these kernels before (513, or 2 x 200) never reached a second iteration here
    assert fc.loop_trips(513, cus) == ((0, 1), (0, 1))


def _masks_follow_the_rules(c):
    B, d = c.B, c.d
    assert not c.m[0, :d - 1].any() and not (c.m2 & ~c.m).any()
    assert not c.m[B - 1, :d - 1].any() and not c.m2[B - 1, :d - 1].any() and c.m[B - 1, d - 1] == c.m2[B - 1, d - 1]
    if B > 2:
        assert not c.m[0].any() and np.array_equal(c.m[1], ~c.kink[1])


def _check_sound(c, what):
    assert c.removed <= fc.KINK_CAP, (what, c.removed)
    _masks_follow_the_rules(c)
    t32 = fc.torch32(c)
    figs = []
    for got, ref in (list(zip(t32, c.ref)) + ([(fc.stacked32(t32), c.stacked())] if c.npass == 2 else [])):
        e = fc.rel_err(got[0], ref[0])
        figs.append(e / fc.AGG_TOL)
        assert e <= fc.AGG_TOL / fc.SOUND, (what, "agg", e)
        for k in fc.GRAD_KEYS:
            e = fc.rel_err(got[1][k], ref[1][k])
            figs.append(e / fc.GRAD_TOL)
            assert e <= fc.GRAD_TOL / fc.SOUND, (what, k, e)
    return max(figs)


@pytest.mark.parametrize("d,K", fc.EDGE_SHAPES)
def test_edge_inputs_sit_inside_the_bound(d, K):
    worst = 0.0
    for d_, K_, B, two, xd in fc.EDGE:
        if (d_, K_) == (d, K):
            c = fc.edge_case(d, K, B, two, xd)
            worst = max(worst, _check_sound(c, c.what))
    print(f"EDGE d={d} K={K}: fp32 torch worst error / bound {worst:.3f}")


@pytest.mark.parametrize("d,K", fc.STRIDE)
def test_stride_inputs_sit_inside_the_bound(d, K):
    c = fc.stride_case(d, K, fc.CPU_CUS)
    assert c.B == 24 * fc.CPU_CUS + 3 and c.npass == 2
    worst = _check_sound(c, c.what)
    print(f"STRIDE d={d} K={K} B={c.B}: removed {c.removed:.4f}, fp32 torch worst error / bound {worst:.3f}")


def test_fold_bound_is_reachable():
    """The elementwise bound the GPU test holds vpc_eddi_fold to, (K + 2) 2^-24 S, against numpy fp32 arithmetic."""
    for d, K in fc.STRIDE:
        c = fc.stride_case(d, K, fc.CPU_CUS)
        ref, S = fc.fold_ref(c)
        WE = c.Wp[:, 1:1 + K]
        A = c.Wp[:, 0][:, None] + WE @ c.E.T
        C = c.Wp[:, 1 + K][:, None] * c.tb[:, 0][None, :] + c.cp[:, None]
        got = np.stack([A, C]).astype(np.float64)
        assert A.dtype == np.float32 and np.all(np.abs(got - ref) <= (K + 2) * 2.0 ** -24 * S)


def test_rel_err_has_no_floor():
    assert fc.rel_err(np.array([1e-9, 0.0]), np.array([1.02e-9, 0.0])) == pytest.approx(0.02 / 1.02)
    assert fc.rel_err(np.zeros(3), np.zeros(3)) == 0.0 and fc.rel_err(np.array([0.0, 1e-30]), np.zeros(2)) == float("inf")
