"""The streaming MNAR imputation (csrc/vpc_nm_impute.hip: nm_impute_kernel, nm_impute_merge_kernel) on the GPU:
  1. every case of tests/nm_stream_cases.py, REG_notMIWAE_v2 and notMIWAE_myversion, against the float64 oracle with
     injected draws: xm within the bound tests/test_notmiwae_gpu.py holds the chain's llh_xm to (2e-5 of the tensor's max),
     lse within 1e-4 of its max, a sentinel margin behind every output, every partial slot written, lse = NULL the same bits;
  2. the reference's own vectors (tests/golden/nm_{reg,van}_d{14,40,128}.npz): llh_xm at S = K; plane b is not read for the
     regularised class;
  3. chunking at S = 700: every chunk length within the same bounds, the scratch count exact, a repeated call bit-equal;
  4. the draws: a seeded call equals the call on miwae.impute_draws' tensor, rows [a, b) equal the call on those rows with
     row0 = a, seed and offset matter;
  5. harness.eval_vae_mnar(engine="stream") on the reference's checkpoints;
  6. the guards."""
import math
import os

import numpy as np
import pytest
import torch

import nm_stream_cases as SC
from conftest import load_golden

pytestmark = pytest.mark.gpu
TP = {"batch_size": 128, "patience": 1}
SENT = 12345.0
MARGIN = 64
XM_TOL, LSE_TOL = 2e-5, 1e-4
CASES = [(s, k) for s in SC.ALL_SHAPES for k in SC.KINDS]


@pytest.fixture(scope="module")
def nm():
    import vpc_amd
    from vpc_amd import notmiwae
    return notmiwae


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _close(got, ref, tol, what):
    err = _err(got, ref)
    print(what, "err", err, "tol", tol)
    assert err <= tol, (what, err)


def _guarded(*shape):
    n = math.prod(shape)
    buf = torch.full((n + MARGIN,), SENT, device="cuda")
    return buf, buf[:n].view(*shape)


def _margin_intact(buf):
    return bool((buf[-MARGIN:] == SENT).all())


_MODELS = {}


def _model(nm, shape, kind):
    if (shape, kind) not in _MODELS:
        c = SC.stream_case(shape, kind)
        cls = nm.REG_notMIWAE_v2 if c["reg"] else nm.notMIWAE_myversion
        model = cls(c["d"], 500, 10, c["L"], TP, c["S"], 1)
        missing = model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c["params"].items()}, strict=False)
        assert not missing.unexpected_keys and all(k.startswith("logits.") for k in missing.missing_keys)
        _MODELS[shape, kind] = model.cuda()
    return _MODELS[shape, kind]


def _inputs(shape, kind):
    c = SC.stream_case(shape, kind)
    return _dev(c["x"]), _dev(c["mask"]), _dev(c["eps"])


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("shape,kind", CASES)
def test_stream_vs_oracle(nm, shape, kind):
    B, S, d, Ld = shape
    x, m, eps = _inputs(shape, kind)
    model = _model(nm, shape, kind)
    flat = model.flatten_parameters()
    s_chunk = nm.impute_chunk(B, S, 256)
    pbuf, part = _guarded(nm.nm_impute_scratch(B, S, d, Ld, s_chunk))
    xbuf, xm = _guarded(B, d)
    lbuf, lse = _guarded(B)
    nm.nm_impute(flat, x, m, eps, 0, 0, 0, part, xm, lse, B, S, d, Ld, s_chunk, model.regularised)
    ref_xm, ref_lse, a, xmean = SC.reference(shape, kind)
    assert _margin_intact(pbuf) and _margin_intact(xbuf) and _margin_intact(lbuf)
    assert not bool((part == SENT).any())  # every partial slot was written
    _close(xm, ref_xm, XM_TOL, (shape, kind, "xm"))
    _close(lse, ref_lse, LSE_TOL, (shape, kind, "lse"))
    if S == 1:  # weight exactly 1: acc / l is the sample's sigmoid(mean head) divided by 1
        _close(xm, xmean[:, 0], XM_TOL, (shape, kind, "xm, S = 1"))
    # lse = NULL: xm alone, the same bits
    xm2 = torch.empty(B, d, device="cuda")
    nm.nm_impute(flat, x, m, eps, 0, 0, 0, part, xm2, None, B, S, d, Ld, s_chunk, model.regularised)
    assert torch.equal(xm2, xm)


# ------------------------------------------------------------------------------------------------ 2. the reference's vectors
@pytest.mark.parametrize("d", [14, 40, 128])
@pytest.mark.parametrize("kind", SC.KINDS)
def test_reference_vectors(nm, kind, d):
    g = load_golden(f"nm_{kind}_d{d}.npz")
    K, Ld = int(g["K"]), int(g["L"])
    cls = nm.REG_notMIWAE_v2 if kind == "reg" else nm.notMIWAE_myversion
    model = cls(d, 500, 10, Ld, TP, K, 1)
    model.load_state_dict({k[6:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("param.")})
    model = model.cuda()
    x, m, eq = _dev(g["x"]), _dev(g["mask"]), _dev(g["eps_q"])
    other = torch.randn(eq.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    eps = torch.stack([eq, other if kind == "reg" else _dev(g["eps_llh"])])
    xm = nm.impute_stream(model, x, m, eps=eps)  # num_samples = model.num_samples = K
    _close(xm, torch.from_numpy(g["llh_xm"]), XM_TOL, (kind, d, "llh_xm"))
    if kind == "reg":  # plane b is not read
        eps2 = torch.stack([eq, torch.full_like(eq, float("nan"))])
        assert torch.equal(nm.impute_stream(model, x, m, eps=eps2), xm)


# ------------------------------------------------------------------------------------------------ 3. chunking
@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("s_chunk", list(SC.CHUNKS))
def test_chunking(nm, s_chunk, kind):
    shape = B, S, d, Ld = SC.CHUNK_SHAPE
    assert nm.nm_impute_scratch(B, S, d, Ld, s_chunk) == B * SC.CHUNKS[s_chunk] * (2 + d)
    x, m, eps = _inputs(shape, kind)
    model = _model(nm, shape, kind)
    ref_xm, ref_lse, _, _ = SC.reference(shape, kind)
    xm, lse = nm.impute_stream(model, x, m, num_samples=S, eps=eps, s_chunk=s_chunk, return_lse=True)
    _close(xm, ref_xm, XM_TOL, (s_chunk, kind, "xm"))
    print((s_chunk, kind, "xm, span row alone", _err(xm[SC.SPAN_ROW], ref_xm[SC.SPAN_ROW])))
    _close(lse, ref_lse, LSE_TOL, (s_chunk, kind, "lse"))
    xm2, lse2 = nm.impute_stream(model, x, m, num_samples=S, eps=eps, s_chunk=s_chunk, return_lse=True)
    assert torch.equal(xm, xm2) and torch.equal(lse, lse2)


# ------------------------------------------------------------------------------------------------ 4. draws
@pytest.mark.parametrize("kind", SC.KINDS)
def test_seed_equals_materialised_draws(nm, kind):
    from vpc_amd import miwae
    shape = B, S, d, Ld = SC.CHUNK_SHAPE
    x, m, _ = _inputs(shape, kind)
    model = _model(nm, shape, kind)
    eps = miwae.impute_draws(B, S, Ld, seed=11, offset=3)
    for s_chunk in (16, 112, None):
        a = nm.impute_stream(model, x, m, num_samples=S, seed=11, offset=3, s_chunk=s_chunk, return_lse=True)
        b = nm.impute_stream(model, x, m, num_samples=S, eps=eps, s_chunk=s_chunk, return_lse=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), s_chunk
    base = nm.impute_stream(model, x, m, num_samples=S, seed=11, offset=3)
    assert not torch.equal(base, nm.impute_stream(model, x, m, num_samples=S, seed=12, offset=3))
    assert not torch.equal(base, nm.impute_stream(model, x, m, num_samples=S, seed=11, offset=4))


@pytest.mark.parametrize("kind", SC.KINDS)
def test_rows_of_a_call_equal_the_call_on_those_rows(nm, kind):
    shape = B, S, d, Ld = (300, 3, 12, 10)
    x, m, _ = _inputs(shape, kind)
    model = _model(nm, shape, kind)
    whole, lse = nm.impute_stream(model, x, m, num_samples=S, seed=5, offset=7, return_lse=True)
    for a, b in ((0, 1), (17, 42), (299, 300)):
        part, lp = nm.impute_stream(model, x[a:b], m[a:b], num_samples=S, seed=5, offset=7, row0=a, return_lse=True)
        assert torch.equal(part, whole[a:b]) and torch.equal(lp, lse[a:b]), (a, b)


# ------------------------------------------------------------------------------------------------ 5. eval_vae_mnar
@pytest.mark.parametrize("kind", SC.KINDS)
def test_eval_vae_mnar_stream_checkpoint_interop(nm, kind, tmp_path, monkeypatch):
    """tests/test_notmiwae_gpu.py::test_eval_vae_mnar_checkpoint_interop with engine="stream": the same checkpoint, the same
    24 rows, valid_k = 4000, M = 3, the reference's file name - and 1e-3 of the golden RMSE, not 1.5 %: the fp32 CPU
    restatement of the estimator deviates from the golden by at most 8.1e-5 (reg) / 4.9e-5 (van) over 16 seeds, so 1e-3 is
    twelve times the Monte-Carlo spread, and a defect of the estimator would not hide under it."""
    import vpc_amd
    g = load_golden(f"nm_eval_{kind}_d14.npz")
    vae_type = "reg_notMIWAE1" if kind == "reg" else "vanilla_notMIWAE1"
    monkeypatch.chdir(tmp_path)
    ck = vpc_amd.checkpoint_path("exp", "toy", vae_type, 50, alpha=0.5, p_missingness=50, reg_type="kl_reg")
    os.makedirs(os.path.dirname(ck))
    torch.save({k[6:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("param.")}, ck)
    x, mask = torch.from_numpy(g["x"]), torch.from_numpy(g["mask"])
    args = (x, mask, 50, 14, 500, 10, int(g["M"]), int(g["L"]), "toy", TP, "exp", vae_type, 100, int(g["valid_k"]), 1)
    kw = dict(alpha=0.5, p_missingness=50, reg_type="kl_reg")
    rmse = vpc_amd.eval_vae_mnar(*args, **kw, engine="stream", seed=1234)
    ref = float(g["rmse"])
    print(kind, "stream", rmse.item(), "golden", ref, "rel", abs(rmse.item() - ref) / ref)
    assert abs(rmse.item() - ref) <= 1e-3 * ref, (rmse.item(), ref)
    fam = "".join(c for c in vae_type if not c.isdigit())
    assert os.listdir(os.path.join("experiments", "exp", "toy", "rest", fam)) == [str(g["result_file"])]
    again = vpc_amd.eval_vae_mnar(*args, **kw, engine="stream", seed=1234, save=False)
    assert again.item() == rmse.item()  # a seed reproduces the run
    # engine="chain" with defaults is the call without engine
    torch.manual_seed(3)
    plain = vpc_amd.eval_vae_mnar(*args, **kw, save=False, max_decoder_rows=40000)
    torch.manual_seed(3)
    chain = vpc_amd.eval_vae_mnar(*args, **kw, save=False, max_decoder_rows=40000, engine="chain")
    assert chain.item() == plain.item()
    with pytest.raises(vpc_amd.VpcError):
        vpc_amd.eval_vae_mnar(*args, **kw, engine="eager", save=False)


# ------------------------------------------------------------------------------------------------ 6. guards
def test_guards(nm):
    import vpc_amd
    shape = B, S, d, Ld = (2, 17, 17, 10)
    x, m, eps = _inputs(shape, "van")
    model = _model(nm, shape, "van")
    for dd, ll in ((129, 10), (12, 17)):
        wide = nm.notMIWAE_myversion(dd, 500, 10, ll, TP, 5, 1).cuda()
        with pytest.raises(vpc_amd.VpcError):
            nm.impute_stream(wide, torch.rand(2, dd, device="cuda"), torch.ones(2, dd, device="cuda"))
    with pytest.raises(vpc_amd.VpcError):
        nm.impute_stream(model, x, m, num_samples=0)
    with pytest.raises(vpc_amd.VpcError):
        nm.impute_stream(model, x, m, num_samples=S, s_chunk=0)
    with pytest.raises(vpc_amd.VpcError):
        nm.impute_stream(model, x, m, num_samples=S, seed=1, offset=2 ** 32)
    with pytest.raises(vpc_amd.VpcError):
        nm.impute_stream(model, x.cpu(), m.cpu(), num_samples=S)
    with pytest.raises(vpc_amd.VpcError):
        nm.impute_stream(model, x, m.cpu(), num_samples=S)
    with pytest.raises(vpc_amd.VpcError):
        nm.impute_stream(model, x, m, num_samples=S, eps=eps.cpu())
    with pytest.raises(vpc_amd.VpcError):
        nm.impute_stream(model, x, m, num_samples=S, eps=eps[:, :, :-1])
    with pytest.raises(vpc_amd.VpcError):
        nm.impute_stream(model, x, m, num_samples=S, missing_process="linear")
    # the raw entry: a partial buffer one float short - nothing is launched, nothing is written
    flat = model.flatten_parameters()
    part = torch.full((4096,), SENT, device="cuda")
    xm = torch.full((B, d), SENT, device="cuda")
    n = nm.nm_impute_scratch(B, S, d, Ld, 16)
    L = vpc_amd._lib
    assert L.lib().vpc_nm_impute(L.ptr(flat), L.ptr(x), L.ptr(m), None, 1, 0, 0, L.ptr(part), n - 1, L.ptr(xm), None, B, S, d,
                                 Ld, 16, 0, L.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((xm == SENT).all()) and bool((part == SENT).all())
