"""CPU: what tests/test_miwae_stream_gpu.py relies on - the default chunk rule, the case table against the kernel's
instantiations, the partial buffer's size, the C declarations, and the planted rows of the cases on the float64 oracle."""
import os
import re

import pytest
import torch

import miwae_stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mw():
    import vpc_amd
    from vpc_amd import miwae
    return miwae


@pytest.mark.parametrize("n_cu", [1, 8, 256, 304])
def test_impute_chunk_properties(mw, n_cu):
    for B in (1, 2, 3, 5, 64, 255, 256, 257, 1600):
        last = 0
        for S in list(range(1, 700)) + [700, 701, 4999, 5000, 5001, 100000]:
            c = mw.impute_chunk(B, S, n_cu)
            assert c % 16 == 0 and c >= 16, (B, S, n_cu, c)
            chunks = -(-S // c)
            if B * -(-S // 16) >= n_cu:  # S allows one workgroup per compute unit
                assert B * chunks >= n_cu, (B, S, n_cu, c)
            assert c == 16 or (c - 16) * chunks < S, (B, S, n_cu, c)  # balanced: no smaller multiple keeps the chunk count
            assert c >= last, (B, S, n_cu, c, last)  # monotone in S
            last = c
    assert mw.impute_chunk(1600, 5000, 256) == 2512 and mw.impute_chunk(64, 5000, 256) == 1264
    assert mw.impute_chunk(256, 5000, 256) == 5008 and mw.impute_chunk(5, 700, 256) == 16
    assert mw.impute_chunk(1, 9, 256) == 16


def test_case_table_covers_every_instantiation():
    built = SC.built_instances()
    assert built == {(yt, lt) for yt in range(1, 7) for lt in (1, 2)}
    assert {SC.instance(s[2], s[3]) for s in SC.ALL_SHAPES} == built
    assert all(1 <= s[2] <= 32 and 1 <= s[3] <= 16 for s in SC.ALL_SHAPES)


def test_scratch_formula(mw):
    for B, S, d, Ld in SC.ALL_SHAPES:
        for s_chunk in (1, 15, 16, 17, 48, 112, 700, 10000):
            c16 = -(-s_chunk // 16) * 16
            assert mw.miw_impute_scratch(B, S, d, Ld, s_chunk) == B * -(-S // c16) * (2 + d), (B, S, d, Ld, s_chunk)
    for s_chunk, n in SC.CHUNKS.items():
        B, S, d, Ld = SC.CHUNK_SHAPE
        assert mw.miw_impute_scratch(B, S, d, Ld, s_chunk) == B * n * (2 + d)
    for bad in [(0, 9, 12, 10, 16), (1, 0, 12, 10, 16), (1, 9, 33, 10, 16), (1, 9, 12, 17, 16), (1, 9, 12, 10, 0),
                (1, 9, 0, 10, 16), (1, 9, 12, 0, 16)]:
        assert mw.miw_impute_scratch(*bad) == 0, bad


def test_entries_are_declared_in_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpc.h")).read(), flags=re.S)
    for ret, name in (("long", "vpc_miw_impute_scratch"), ("int", "vpc_miw_impute"), ("int", "vpc_miw_impute_draws")):
        assert re.search(rf"\b{ret}\s+{name}\s*\(", hdr), name


def test_raw_entry_refuses_bad_arguments_without_gpu():
    """VPC_ERR_ARG (1) before any launch: shapes outside the limits, NULL required pointers, a short partial buffer, counters
    past 2^32."""
    import ctypes
    import vpc_amd
    l = vpc_amd._lib.lib()
    host = (ctypes.c_float * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(host))
    n = 2 * 2 * 14

    def call(B=2, S=20, d=12, L=10, sc=16, prm=p, x=p, m=p, part=p, nf=n, xm=p, off=0, row0=0):
        return l.vpc_miw_impute(prm, x, m, None, 1, off, row0, part, nf, xm, None, B, S, d, L, sc, None)

    for kw in (dict(B=0), dict(S=0), dict(d=0), dict(d=33), dict(L=0), dict(L=17), dict(sc=0), dict(prm=None), dict(x=None),
               dict(m=None), dict(part=None), dict(xm=None), dict(nf=n - 1), dict(off=2 ** 32 - 1), dict(row0=-1),
               dict(row0=2 ** 32)):
        assert call(**kw) == 1, kw
    assert l.vpc_miw_impute_draws(None, 2, 20, 10, 1, 0, 0, None) == 1
    assert l.vpc_miw_impute_draws(p, 2, 20, 17, 1, 0, 0, None) == 1
    assert l.vpc_miw_impute_draws(p, 2, 0, 10, 1, 0, 0, None) == 1
    assert l.vpc_miw_impute_draws(p, 2, 20, 10, 1, 2 ** 32 - 1, 0, None) == 1


def test_draw_counter_rule():
    from vpc_amd import trainer
    ctr, comp = trainer.impute_draw_counter(7, 100, 3, 5, 9)
    assert ctr == ((110 << 32) | 22) and comp == 1
    # rows [a, b) of a call and the call on those rows with row0 = a: the same counters
    assert trainer.impute_draw_counter(7, 0, 5, 2, 0) == trainer.impute_draw_counter(7, 5, 0, 2, 0)
    # consecutive calls of a run (the offset advanced by the rows of the call, as eval_miwae does) use disjoint high words
    hi = lambda off, B: {trainer.impute_draw_counter(off, 0, r, 0, 0)[0] >> 32 for r in range(B)}
    assert not hi(0, 16) & hi(16, 8)


@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("shape", SC.ALL_SHAPES)
def test_planted_rows(shape, kind):
    c = SC.stream_case(shape, kind)
    B, S, d, Ld = shape
    assert c["mask"][0].all()
    xm, lse, lo, a_q = SC.reference(shape, kind)
    assert xm.shape == (B, d) and bool(torch.isfinite(xm).all()) and bool(torch.isfinite(a_q).all())
    if B >= 2:
        assert not c["mask"][1].any()
    if S == 1:  # a single sample: weight exactly 1, the imputation is that sample's x_mean
        assert bool((torch.softmax(a_q, 0) == 1).all())
    if shape in SC.SPAN_SHAPES:
        span = float(a_q[:, 2].max() - a_q[:, 2].min())
        assert span > SC.SPAN_NATS, span
        assert float(a_q[:, 2].abs().max()) < 200  # ... at a size whose fp32 rounding (1e-5 nats) stays below the bound on xm
        assert float(torch.softmax(a_q[:, 2], 0).max()) < 0.9  # ... and no single sample takes all the weight


@pytest.mark.parametrize("shape", SC.ALL_SHAPES)
def test_reg_reference_does_not_depend_on_mask_p(shape):
    c = SC.stream_case(shape, "reg")
    assert (SC.other_mask_p(c) != c["mask_p"])[0].all()  # row 0 is fully observed
    a, b = SC.reference(shape, "reg"), SC.reference(shape, "reg", True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
