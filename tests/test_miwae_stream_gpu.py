"""The streaming MIWAE imputation (csrc/vpc_miw_impute.hip: miw_impute_kernel, miw_impute_merge_kernel,
miw_impute_draws_kernel) on the GPU:
  1. every case of tests/miwae_stream_cases.py, MIWAE and Reg_MIWAE, against the float64 oracle with injected draws: xm
     within the bound tests/test_miwae_kernels_gpu.py holds the chain's xm_imp to (2e-5 of the tensor's max), for MIWAE
     -mean(lse) within 1e-4 of the oracle's loss, the Reg result against the oracle run with two different mask_p, a sentinel
     margin behind every output;
  2. chunking at S = 700: every chunk length within the same bound, a repeated call bit-equal;
  3. the draws: a seeded call equals the call on impute_draws' tensor, rows [a, b) equal the call on those rows with
     row0 = a, seed and offset matter, moments, the two planes differ;
  4. model.impute(engine=...) and harness.eval_miwae(engine="stream") on the reference's checkpoints;
  5. the guards."""
import math
import os

import numpy as np
import pytest
import torch

import miwae_stream_cases as SC
from conftest import load_golden

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 1}
SENT = 12345.0
MARGIN = 64
XM_TOL, LOSS_TOL = 2e-5, 1e-4


@pytest.fixture(scope="module")
def mw():
    import vpc_amd
    from vpc_amd import miwae
    return miwae


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


def _model(mw, shape, kind):
    if (shape, kind) not in _MODELS:
        c = SC.stream_case(shape, kind)
        cls = mw.Reg_MIWAE if c["reg"] else mw.MIWAE
        model = cls(c["d"], 500, 10, c["L"], TP, c["S"], 1)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c["params"].items()})
        _MODELS[shape, kind] = model.cuda()
    return _MODELS[shape, kind]


def _inputs(shape, kind):
    c = SC.stream_case(shape, kind)
    return _dev(c["x"]), _dev(c["mask"]), _dev(SC.stream_eps(c))


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("shape", SC.ALL_SHAPES)
def test_stream_vs_oracle(mw, shape, kind):
    B, S, d, Ld = shape
    x, m, eps = _inputs(shape, kind)
    flat = _model(mw, shape, kind).flatten_parameters()
    s_chunk = mw.impute_chunk(B, S, 256)
    pbuf, part = _guarded(mw.miw_impute_scratch(B, S, d, Ld, s_chunk))
    xbuf, xm = _guarded(B, d)
    lbuf, lse = _guarded(B)
    mw.miw_impute(flat, x, m, eps, 0, 0, 0, part, xm, lse, B, S, d, Ld, s_chunk)
    ref_xm, ref_lse, lo, a_q = SC.reference(shape, kind)
    assert _margin_intact(pbuf) and _margin_intact(xbuf) and _margin_intact(lbuf)
    assert not bool((part == SENT).any())  # every partial slot was written
    _close(xm, ref_xm, XM_TOL, (shape, kind, "xm"))
    print((shape, kind, "lse err", _err(lse, ref_lse)))
    if kind == "van":
        got = -float(lse.double().mean())
        print((shape, "loss", got, lo.item()))
        assert abs(got - lo.item()) <= LOSS_TOL * abs(lo.item()), (got, lo.item())
    else:  # one stream call, the oracle with two different mask_p
        _close(xm, SC.reference(shape, kind, True)[0], XM_TOL, (shape, kind, "xm, second mask_p"))
    if S == 1:  # weight exactly 1: acc / l is the sample's sigmoid(mean head) divided by 1
        assert bool(torch.isfinite(xm).all()) and _err(lse, a_q[0]) <= LOSS_TOL
    # lse = NULL: xm alone, the same bits
    xm2 = torch.empty(B, d, device="cuda")
    mw.miw_impute(flat, x, m, eps, 0, 0, 0, part, xm2, None, B, S, d, Ld, s_chunk)
    assert torch.equal(xm2, xm)


# ------------------------------------------------------------------------------------------------ 2. chunking
@pytest.mark.parametrize("kind", ["reg", "van"])
@pytest.mark.parametrize("s_chunk", list(SC.CHUNKS))
def test_chunking(mw, s_chunk, kind):
    shape = B, S, d, Ld = SC.CHUNK_SHAPE
    assert mw.miw_impute_scratch(B, S, d, Ld, s_chunk) == B * SC.CHUNKS[s_chunk] * (2 + d)
    x, m, eps = _inputs(shape, kind)
    model = _model(mw, shape, kind)
    ref_xm, ref_lse, lo, _ = SC.reference(shape, kind)
    xm, lse = mw.impute_stream(model, x, m, num_samples=S, eps=eps, s_chunk=s_chunk, return_lse=True)
    _close(xm, ref_xm, XM_TOL, (s_chunk, kind, "xm"))
    if kind == "van":
        got = -float(lse.double().mean())
        assert abs(got - lo.item()) <= LOSS_TOL * abs(lo.item()), (got, lo.item())
    xm2, lse2 = mw.impute_stream(model, x, m, num_samples=S, eps=eps, s_chunk=s_chunk, return_lse=True)
    assert torch.equal(xm, xm2) and torch.equal(lse, lse2)


# ------------------------------------------------------------------------------------------------ 3. draws
def test_seed_equals_materialised_draws(mw):
    shape = B, S, d, Ld = SC.CHUNK_SHAPE
    x, m, _ = _inputs(shape, "van")
    model = _model(mw, shape, "van")
    eps = mw.impute_draws(B, S, Ld, seed=11, offset=3)
    assert eps.shape == (2, B, S, Ld) and bool(torch.isfinite(eps).all())
    for s_chunk in (16, 112, None):
        a = mw.impute_stream(model, x, m, num_samples=S, seed=11, offset=3, s_chunk=s_chunk, return_lse=True)
        b = mw.impute_stream(model, x, m, num_samples=S, eps=eps, s_chunk=s_chunk, return_lse=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), s_chunk
    base = mw.impute_stream(model, x, m, num_samples=S, seed=11, offset=3)
    assert not torch.equal(base, mw.impute_stream(model, x, m, num_samples=S, seed=12, offset=3))
    assert not torch.equal(base, mw.impute_stream(model, x, m, num_samples=S, seed=11, offset=4))


def test_rows_of_a_call_equal_the_call_on_those_rows(mw):
    shape = B, S, d, Ld = (300, 3, 12, 10)
    x, m, _ = _inputs(shape, "reg")
    model = _model(mw, shape, "reg")
    whole, lse = mw.impute_stream(model, x, m, num_samples=S, seed=5, offset=7, return_lse=True)
    for a, b in ((0, 1), (17, 42), (299, 300)):
        part, lp = mw.impute_stream(model, x[a:b], m[a:b], num_samples=S, seed=5, offset=7, row0=a, return_lse=True)
        assert torch.equal(part, whole[a:b]) and torch.equal(lp, lse[a:b]), (a, b)
    eps = mw.impute_draws(B, S, Ld, seed=5, offset=7)
    assert torch.equal(mw.impute_draws(25, S, Ld, seed=5, offset=7, row0=17), eps[:, 17:42])
    assert torch.equal(mw.impute_draws(25, S, Ld, seed=5, offset=24), eps[:, 17:42])  # the rule adds offset and row


def test_draw_moments(mw):
    """The bounds of tests/test_flow_reward_gpu.py on 400 000 values, per plane on 200 000."""
    eps = mw.impute_draws(50, 500, 8, seed=3)
    assert eps.numel() == 400000
    for name, v in (("both", eps), ("a", eps[0]), ("b", eps[1])):
        v = v.double().flatten()
        mean, var, inside = float(v.mean()), float(v.var()), float((v.abs() < 1).double().mean())
        print(name, mean, var, inside)
        assert abs(mean) < 0.02 and abs(var - 1) < 0.03 and abs(inside - 0.6827) < 0.01, (name, mean, var, inside)
    assert not torch.equal(eps[0], eps[1])
    assert float((eps[0] == eps[1]).double().mean()) < 1e-3
    assert abs(float((eps[0].double() * eps[1].double()).mean())) < 0.02  # uncorrelated planes
    # odd latent widths use the same counters: component l of a group does not depend on L
    assert torch.equal(mw.impute_draws(3, 5, 3, seed=3)[..., :3], mw.impute_draws(3, 5, 4, seed=3)[..., :3])


# ------------------------------------------------------------------------------------------------ 4. engines
@pytest.mark.parametrize("kind", ["reg", "van"])
def test_model_impute_engines(mw, kind):
    shape = B, S, d, Ld = (2, 17, 17, 10)
    c = SC.stream_case(shape, kind)
    x, m, eps = _inputs(shape, kind)
    mp = _dev(c["mask_p"])
    model = _model(mw, shape, kind)
    want = mw.impute_stream(model, x, m, num_samples=S, eps=eps)
    got = model.impute(x, m, mp, num_samples=S, engine="stream", eps=eps)
    assert model.last_impute_engine == "stream" and torch.equal(got, want)
    chain = model.impute(x, m, mp, num_samples=S)  # the default: the launch chain, with its own torch draws
    assert model.last_impute_engine == "chain"
    assert chain.shape == (B, d) and bool(torch.isfinite(chain).all())
    import vpc_amd
    with pytest.raises(vpc_amd.VpcError):
        model.impute(x, m, mp, num_samples=S, engine="fused")
    with pytest.raises(vpc_amd.VpcError):
        model.impute(x, m, mp, num_samples=S, eps=eps)  # draws belong to the stream engine


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_eval_miwae_stream_checkpoint_interop(mw, kind, tmp_path, monkeypatch):
    """tests/test_miwae_gpu.py::test_eval_miwae_checkpoint_interop with engine="stream": the same checkpoint, the same two
    batches of 16 + 8 rows, the same interval (the reference's six-seed spread +- 3 sigma), the same file names."""
    import vpc_amd
    g = load_golden(f"miwae_eval_{kind}_d14.npz")
    vae_type = "reg_MIWAE1" if kind == "reg" else "vanilla_MIWAE1"
    monkeypatch.chdir(tmp_path)
    ck = vpc_amd.checkpoint_path("exp", "toy", vae_type, 40, alpha=0.5, p_missingness=30, reg_type="kl_reg")
    assert os.path.basename(ck) == str(g["checkpoint_file"])
    os.makedirs(os.path.dirname(ck))
    torch.save({k[6:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("param.")}, ck)
    x, mask = torch.from_numpy(g["x"]), torch.from_numpy(g["mask"])
    loaders = [([(x[:16], mask[:16]), (x[16:], mask[16:])], "test")]
    args = (loaders, 40, 14, 500, 10, int(g["M"]), int(g["L"]), "toy", TP, "exp", vae_type, 100, int(g["valid_k"]), 1)
    kw = dict(alpha=0.5, p_missingness=30, reg_type="kl_reg")
    res = vpc_amd.eval_miwae(*args, **kw, engine="stream", seed=1234)
    ref = g["rmse"]
    lo, hi = ref.min() - 3 * ref.std() - 1e-3 * ref.mean(), ref.max() + 3 * ref.std() + 1e-3 * ref.mean()
    print(kind, res["test"].item(), ref)
    assert lo <= res["test"].item() <= hi, (res["test"].item(), ref)
    fam = "".join(c for c in vae_type if not c.isdigit())
    assert os.listdir(os.path.join("experiments", "exp", "toy", "rest", fam)) == [str(g["result_file"])]
    again = vpc_amd.eval_miwae(*args, **kw, engine="stream", seed=1234, save=False)
    assert again["test"].item() == res["test"].item()  # a seed reproduces the run
    other = vpc_amd.eval_miwae(*args, **kw, engine="stream", seed=1235, save=False)
    assert other["test"].item() != res["test"].item()  # (the interval is asserted for one seed, as for the chain: over
    # seeds both engines spread wider than the reference's six runs happened to, profiles/miw_impute_notes.md)
    with pytest.raises(vpc_amd.VpcError):
        vpc_amd.eval_miwae(*args, **kw, engine="eager", save=False)


# ------------------------------------------------------------------------------------------------ 5. guards
def test_guards(mw):
    import vpc_amd
    shape = B, S, d, Ld = (2, 17, 17, 10)
    x, m, eps = _inputs(shape, "van")
    model = _model(mw, shape, "van")
    flat = model.flatten_parameters()
    part = torch.full((4096,), SENT, device="cuda")
    xm = torch.full((B, 40), SENT, device="cuda")
    for bad in (dict(d=33), dict(Ld=17), dict(S=0), dict(s_chunk=0), dict(B=0)):
        a = dict(B=B, S=S, d=d, Ld=Ld, s_chunk=16)
        a.update(bad)
        with pytest.raises(vpc_amd.VpcError):
            mw.miw_impute(flat, x, m, None, 1, 0, 0, part, xm, None, a["B"], a["S"], a["d"], a["Ld"], a["s_chunk"])
    # the raw entry: a partial buffer one float short
    n = mw.miw_impute_scratch(B, S, d, Ld, 16)
    L = vpc_amd._lib
    assert L.lib().vpc_miw_impute(L.ptr(flat), L.ptr(x), L.ptr(m), None, 1, 0, 0, L.ptr(part), n - 1, L.ptr(xm), None, B, S, d,
                                  Ld, 16, L.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((xm == SENT).all()) and bool((part == SENT).all())
    # the host entry
    with pytest.raises(vpc_amd.VpcError):
        mw.impute_stream(model, x.cpu(), m.cpu(), num_samples=S)
    with pytest.raises(vpc_amd.VpcError):
        mw.impute_stream(model, x, m.cpu(), num_samples=S)
    with pytest.raises(vpc_amd.VpcError):
        mw.impute_stream(model, x, m, num_samples=S, eps=eps[:, :, :-1])
    with pytest.raises(vpc_amd.VpcError):
        mw.impute_stream(model, x, m, num_samples=S, eps=eps.cpu())
    with pytest.raises(vpc_amd.VpcError):
        mw.impute_stream(model, x, m, num_samples=0)
    with pytest.raises(vpc_amd.VpcError):
        mw.impute_stream(model, x, m, num_samples=S, s_chunk=0)
    with pytest.raises(vpc_amd.VpcError):
        mw.impute_stream(model, x, m, num_samples=S, seed=1, offset=2 ** 32)
    for dd, ll in ((33, 10), (12, 17)):
        wide = mw.MIWAE(dd, 500, 10, ll, TP, 5, 1).cuda()
        with pytest.raises(vpc_amd.VpcError):
            mw.impute_stream(wide, torch.rand(2, dd, device="cuda"), torch.ones(2, dd, device="cuda"))
        with pytest.raises(vpc_amd.VpcError):
            wide.impute(torch.rand(2, dd, device="cuda"), torch.ones(2, dd, device="cuda"), engine="stream")
    with pytest.raises(vpc_amd.VpcError):
        mw.impute_draws(2, 5, 17, seed=1)
    with pytest.raises(vpc_amd.VpcError):
        mw.impute_draws(2, 5, 4, seed=1, device="cpu")
