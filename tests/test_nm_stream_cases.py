"""CPU: what tests/test_nm_stream_gpu.py relies on - the case table against the kernel's instantiations, the partial
buffer's size, the C declarations, the raw entry's refusals (the library loads without a GPU), the planted rows of the
cases on the float64 oracle, the room the fp32 restatement leaves under the GPU bound, and eval_vae_mnar's engine guard."""
import os
import re

import pytest
import torch

import nm_stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(s, k) for s in SC.ALL_SHAPES for k in SC.KINDS]


@pytest.fixture(scope="module")
def nm():
    import vpc_amd
    from vpc_amd import notmiwae
    return notmiwae


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))


def test_case_table_covers_every_instantiation():
    built = SC.built_instances()
    assert built == {(ht, lt, reg) for ht in (1, 2) for lt in (1, 2) for reg in (False, True)}
    assert {SC.instance(s[2], s[3]) + (k == "reg",) for s, k in CASES} == built
    assert all(1 <= s[2] <= 128 and 1 <= s[3] <= 16 for s in SC.ALL_SHAPES)
    assert SC.instance(64, 8) == (1, 1) and SC.instance(65, 9) == (2, 2)  # the two thresholds, from both sides


def test_scratch_formula(nm):
    for B, S, d, Ld in SC.ALL_SHAPES:
        for s_chunk in (1, 15, 16, 17, 48, 112, 700, 10000):
            c16 = -(-min(s_chunk, S) // 16) * 16
            assert nm.nm_impute_scratch(B, S, d, Ld, s_chunk) == B * -(-S // c16) * (2 + d), (B, S, d, Ld, s_chunk)
    for s_chunk, n in SC.CHUNKS.items():
        B, S, d, Ld = SC.CHUNK_SHAPE
        assert nm.nm_impute_scratch(B, S, d, Ld, s_chunk) == B * n * (2 + d)
    for bad in [(0, 9, 12, 10, 16), (1, 0, 12, 10, 16), (1, 9, 129, 10, 16), (1, 9, 12, 17, 16), (1, 9, 12, 10, 0),
                (1, 9, 0, 10, 16), (1, 9, 12, 0, 16), (1, 2 ** 28 + 1, 12, 10, 16)]:
        assert nm.nm_impute_scratch(*bad) == 0, bad
    assert nm.nm_impute_scratch(1, 2 ** 28, 12, 10, 2 ** 28) == 14


def test_entries_are_declared_in_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpc.h")).read(), flags=re.S)
    for ret, name in (("long", "vpc_nm_impute_scratch"), ("int", "vpc_nm_impute")):
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

    def call(B=2, S=20, d=12, L=10, sc=16, prm=p, x=p, m=p, part=p, nf=n, xm=p, off=0, row0=0, reg=1):
        return l.vpc_nm_impute(prm, x, m, None, 1, off, row0, part, nf, xm, None, B, S, d, L, sc, reg, None)

    for kw in (dict(B=0), dict(S=0), dict(S=2 ** 28 + 1), dict(d=0), dict(d=129), dict(L=0), dict(L=17), dict(sc=0),
               dict(prm=None), dict(x=None), dict(m=None), dict(part=None), dict(xm=None), dict(nf=n - 1),
               dict(off=2 ** 32 - 1), dict(off=2 ** 32), dict(row0=-1), dict(row0=2 ** 32), dict(off=2 ** 31, row0=2 ** 31)):
        for reg in (0, 1):
            assert call(reg=reg, **kw) == 1, kw


@pytest.mark.parametrize("shape,kind", CASES)
def test_planted_rows(shape, kind):
    c = SC.stream_case(shape, kind)
    B, S, d, Ld = shape
    assert c["mask"][0].all()
    xm, lse, a, xmean = SC.reference(shape, kind)
    assert xm.shape == (B, d) and a.shape == (B, S) and bool(torch.isfinite(xm).all()) and bool(torch.isfinite(a).all())
    # the port's llh_eval imputation is the softmax of these log-weights on the decoder's means
    assert _rel(torch.sum(torch.softmax(a, 1).unsqueeze(2) * xmean, 1), xm) < 1e-12
    if B >= 2:
        assert not c["mask"][1].any()
    if S == 1:  # a single sample: weight exactly 1, the imputation is that sample's x_mean
        assert bool((torch.softmax(a, 1) == 1).all()) and torch.equal(xm, xmean[:, 0])


@pytest.mark.parametrize("kind", SC.KINDS)
def test_span_row(kind):
    """The three conditions of the span row: the float64 log-weights span at least SPAN_NATS, none is larger than
    SPAN_MAX_ABS (fp32 rounding of a log-weight stays small against the bound on xm), and they ascend with the sample index."""
    c = SC.stream_case(SC.SPAN_SHAPE, kind)
    assert c["mask"][SC.SPAN_ROW, SC.SPAN_COLUMN] == 1 and c["x"][SC.SPAN_ROW, SC.SPAN_COLUMN] == SC.SPAN_X
    a = SC.reference(SC.SPAN_SHAPE, kind)[2][SC.SPAN_ROW]
    span, top = float(a.max() - a.min()), float(a.abs().max())
    print(kind, "span", span, "max |a|", top)
    assert span >= SC.SPAN_NATS, span
    assert top <= SC.SPAN_MAX_ABS, top
    assert bool((a[1:] >= a[:-1]).all()) and float(a[-1] - a[0]) == span


@pytest.mark.parametrize("shape,kind", CASES)
def test_fp32_port_leaves_room_under_the_gpu_bound(shape, kind):
    """The fp32 restatement of the same terms stays within 2e-6 of float64 on xm (the GPU test allows 2e-5)."""
    ref = SC.reference(shape, kind)
    f32 = SC.reference(shape, kind, torch.float32)
    err = _rel(f32[0], ref[0])
    print(shape, kind, "fp32 port xm err", err, "lse err", _rel(f32[1], ref[1]))
    assert err <= 2e-6, err


@pytest.mark.parametrize("shape", SC.ALL_SHAPES)
def test_reg_reference_does_not_depend_on_mask_p(shape):
    c = SC.stream_case(shape, "reg")
    assert (SC.other_mask_p(c) != c["mask_p"])[0].all()  # row 0 is fully observed
    a, b = SC.reference(shape, "reg"), SC.reference(shape, "reg", torch.float64, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_eval_vae_mnar_refuses_an_unknown_engine():
    import vpc_amd
    x = torch.rand(4, 14)
    with pytest.raises(vpc_amd.VpcError, match="engine"):
        vpc_amd.eval_vae_mnar(x, torch.ones(4, 14), 50, 14, 500, 10, 1, 10, "toy", {"batch_size": 128, "patience": 1}, "exp",
                              "reg_notMIWAE1", 100, 8, 1, engine="eager", save=False)
