"""GPU tests of the batched flow evaluation (csrc/vpc_floweval.hip, flow.FlowEvaluator, eval_vae / eval_sweep engine="batched"):
  1. vpc_flow_fwd_tiles against vpc_flow_fwd tile by tile, bit for bit; a tile with no inside draw between splined neighbours;
  2. vpc_flow_eval_tiles against vpc_flow_loss tile by tile (columns 0, 1, 3 bit for bit), columns 2, 4, 5 against float64, a
     tile with nothing unobserved; the argument checks of the three entries;
  3. FlowEvaluator.evaluate against the float64 oracle per tile and through the numpy finalize, chunked against unchunked bit
     for bit, the device draws; the harness engines.
Layouts and references: tests/flow_eval_cases.py (hid 64, 258 rows in 12 ragged tiles of two passes)."""
import os

import numpy as np
import pytest
import torch

import flow_cases as FC
import flow_eval_cases as C
from conftest import load_golden

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 1}
R = C.ROWS
HL = 0.5 * np.log(2 * np.pi)


@pytest.fixture(scope="module")
def fl():
    import vpc_amd
    from vpc_amd import flow
    return flow


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _tabs(tile_row0):
    tab = torch.from_numpy(np.asarray(tile_row0, np.int64).copy())
    return tab, tab.cuda()


def _pitched(a, ld):
    """[n, w] -> the same rows at pitch ld, NaN in the pad columns."""
    t = torch.full((a.shape[0], ld), float("nan"), device="cuda")
    t[:, :a.shape[1]] = a
    return t


# ------------------------------------------------------------------------------------------------ 1. vpc_flow_fwd_tiles
def _fwd_tiles(fl, t, eps, tile_row0, ldt):
    tab, tab_dev = _tabs(tile_row0)
    z, zlp = torch.full((R, 10), 7.0, device="cuda"), torch.full((R, 10), 7.0, device="cuda")
    fl.flow_fwd_tiles(t, eps, z, zlp, R, tab, tab_dev, ldt=ldt)
    return z, zlp


def _fwd_per_tile(fl, t, eps, tile_row0, ldt):
    z, zlp = torch.empty(R, 10, device="cuda"), torch.empty(R, 10, device="cuda")
    for lo, hi in zip(tile_row0[:-1], tile_row0[1:]):
        n = int(hi - lo)
        fl.flow_fwd(t[lo:hi], eps[lo:hi], z[lo:hi], zlp[lo:hi], n, n, ldt=ldt)
    return z, zlp


@pytest.mark.parametrize("ldt", [100, 128])
@pytest.mark.parametrize("sigma", FC.SIGMAS)
def test_fwd_tiles_equals_per_tile_fwd(fl, sigma, ldt):
    inp = FC.flow_inputs(129, 2, sigma)
    t, eps = _pitched(_dev(inp["t"]), ldt) if ldt > 100 else _dev(inp["t"]), _dev(inp["eps"])
    tile_row0 = C.tables()[0]
    z, zlp = _fwd_tiles(fl, t, eps, tile_row0, ldt)
    zr, zlpr = _fwd_per_tile(fl, t, eps, tile_row0, ldt)
    assert _same_bits(z, zr) and _same_bits(zlp, zlpr)
    assert torch.isfinite(z).all() and torch.isfinite(zlp).all()
    # one tile over all rows is vpc_flow_fwd on one pass of 258 rows
    z1, zlp1 = _fwd_tiles(fl, t, eps, np.array([0, R]), ldt)
    z2, zlp2 = torch.empty_like(z1), torch.empty_like(z1)
    fl.flow_fwd(t, eps, z2, zlp2, R, R, ldt=ldt)
    assert _same_bits(z1, z2) and _same_bits(zlp1, zlp2)


@pytest.mark.parametrize("which", ["middle", "last"])
def test_fwd_tiles_predicate_is_per_tile(fl, which):
    """Every |eps| > 1 in the 5-row tile 3 (rows 8 .. 12) or in the 1-row last tile: that tile alone is the identity with
    z_log_prob = -eps^2 / 2 - log sqrt(2 pi); its neighbours, whose outside draws are zeroed and splined, are not."""
    inp = FC.flow_inputs(129, 2, 1.0)
    tile_row0 = C.tables()[0]
    k = 3 if which == "middle" else len(tile_row0) - 2
    lo, hi = int(tile_row0[k]), int(tile_row0[k + 1])
    assert hi - lo == (5 if which == "middle" else 1)
    rng = np.random.default_rng(11)
    eps = inp["eps"].copy()
    eps[lo:hi] = (rng.choice([-1.0, 1.0], size=(hi - lo, 10)) * (1.25 + rng.random((hi - lo, 10)))).astype(np.float32)
    t, e = _pitched(_dev(inp["t"]), 104), _dev(eps)
    z, zlp = _fwd_tiles(fl, t, e, tile_row0, 104)
    zr, zlpr = _fwd_per_tile(fl, t, e, tile_row0, 104)
    assert _same_bits(z, zr) and _same_bits(zlp, zlpr)
    assert _same_bits(z[lo:hi], e[lo:hi])
    want = -eps[lo:hi].astype(np.float64) ** 2 / 2 - HL
    np.testing.assert_allclose(zlp[lo:hi].cpu().numpy(), want, rtol=1e-6)
    outside = np.abs(eps) > 1
    for nb in (k - 1, k + 1):
        if nb >= len(tile_row0) - 1:
            continue
        a, b = int(tile_row0[nb]), int(tile_row0[nb + 1])
        assert (~outside[a:b]).any(), "the neighbour tile must hold an inside draw"
        # splined: an outside draw is zeroed and splined, so z leaves eps there (and everywhere else but by coincidence)
        zn = z[a:b].cpu().numpy()
        assert (zn != eps[a:b]).mean() > 0.9 and (np.abs(zn) <= 1).all()


# ------------------------------------------------------------------------------------------------ 2. vpc_flow_eval_tiles
def _loss_operands(d, ldxm, mask=None):
    inp = FC.loss_inputs(R, d)
    m = inp["m"] if mask is None else mask
    return dict(x=_dev(inp["x"]), m=_dev(m), xm=_pitched(_dev(inp["xm"][0]), ldxm), z=_dev(inp["z"][0]), zlp=_dev(inp["zlp"][0]),
                np=dict(x=inp["x"], m=m, xm=inp["xm"][0], z=inp["z"][0], zlp=inp["zlp"][0]))


def _eval_tiles(fl, o, d, ldxm, tile_row0, beta):
    tab, tab_dev = _tabs(tile_row0)
    n_tiles = len(tile_row0) - 1
    scratch = fl.flow_eval_tiles_scratch(int(np.diff(tile_row0).max()), n_tiles, "cuda")
    stats = torch.full((n_tiles, 8), -3.0, dtype=torch.float64, device="cuda")
    fl.flow_eval_tiles(o["x"], o["m"], o["xm"], o["z"], o["zlp"], R, d, tab, tab_dev, beta, scratch, stats, ldxm=ldxm)
    return stats


def _loss_per_tile(fl, o, d, ldxm, tile_row0, beta):
    out = torch.empty(len(tile_row0) - 1, 8, dtype=torch.float64, device="cuda")
    for k, (lo, hi) in enumerate(zip(tile_row0[:-1], tile_row0[1:])):
        n = int(hi - lo)
        fl.flow_loss(o["x"][lo:hi], o["m"][lo:hi], None, (o["xm"][lo:hi], None), (o["z"][lo:hi], None), (o["zlp"][lo:hi], None),
                     None, fl.flow_loss_scratch(n, "cuda"), out[k], None, None, n, d, fl.STAGE_TRAIN, 0.0, beta, 1.0, 0,
                     ldxm=ldxm)
    return out


def _stats64(o, tile_row0):
    """Columns 2, 4, 5, 6 in float64 from the fp32 operands."""
    x, m, xm, z, zlp = (o["np"][k].astype(np.float64) for k in ("x", "m", "xm", "z", "zlp"))
    out = np.zeros((len(tile_row0) - 1, 4))
    for k, (lo, hi) in enumerate(zip(tile_row0[:-1], tile_row0[1:])):
        s = slice(lo, hi)
        out[k] = [np.sum(zlp[s] + z[s] ** 2 / 2 + HL), np.sum((xm[s] - x[s]) ** 2 * (1 - m[s])), np.sum(1 - m[s]), hi - lo]
    return out


@pytest.mark.parametrize("beta", [1.0, 0.25])
@pytest.mark.parametrize("d", C.DS)
def test_eval_tiles_equals_per_tile_loss(fl, d, beta):
    ldxm = d + 3
    tile_row0 = C.tables()[0]
    o = _loss_operands(d, ldxm)
    stats = _eval_tiles(fl, o, d, ldxm, tile_row0, beta)
    out8 = _loss_per_tile(fl, o, d, ldxm, tile_row0, beta)
    for col, k8 in ((0, 0), (1, 1), (3, 7), (2, 3)):  # (column 2 = out8[3] too: the same sum)
        assert _same_bits(stats[:, col], out8[:, k8]), (col, stats[:, col], out8[:, k8])
    s, ref = stats.cpu().numpy(), _stats64(o, tile_row0)
    for col, r in ((2, 0), (4, 1)):
        err = np.abs(s[:, col] - ref[:, r]) / np.abs(ref[:, r]).clip(1e-300)
        print(f"d={d} beta={beta} column {col}: worst relative error {err.max():.3g}")
        assert (err[ref[:, r] != 0] <= 2e-5).all() and (s[ref[:, r] == 0, col] == 0).all(), (col, err)
    assert (s[:, 5] == ref[:, 2]).all() and (s[:, 6] == ref[:, 3]).all() and (s[:, 7] == 0).all()


def test_tile_with_nothing_unobserved(fl):
    """mask all ones in tile 4 (25 rows): column 5 = 0 and column 4 = 0 there, NaN for its rmse, every other tile's row
    unchanged, and the finalize returns NaN for the rmse alone."""
    d, ldxm = 12, 12
    tile_row0, pass_tile0 = C.tables()
    base = FC.loss_inputs(R, d)["m"]
    m1 = base.copy()
    lo, hi = int(tile_row0[4]), int(tile_row0[5])
    m1[lo:hi] = 1.0
    s0 = _eval_tiles(fl, _loss_operands(d, ldxm), d, ldxm, tile_row0, 1.0)
    s1 = _eval_tiles(fl, _loss_operands(d, ldxm, m1), d, ldxm, tile_row0, 1.0)
    others = [k for k in range(12) if k != 4]
    assert _same_bits(s0[others], s1[others])
    assert s1[4, 4] == 0 and s1[4, 5] == 0 and abs(float(s1[4, 3]) - 25 * 12 * HL) < 1e-3  # NLL of weight 0: the constant
    ptab, ptab_dev = _tabs(pass_tile0)
    out4 = torch.zeros(4, dtype=torch.float64, device="cuda")
    fl.flow_eval_finalize(s1, 12, ptab, ptab_dev, out4)
    got, want = out4.cpu().numpy(), C.finalize(s1.cpu().numpy(), pass_tile0)
    assert np.isnan(got[0]) and np.isnan(want[0])
    np.testing.assert_allclose(got[1:], want[1:], rtol=1e-13)
    fl.flow_eval_finalize(s0, 12, ptab, ptab_dev, out4)
    np.testing.assert_allclose(out4.cpu().numpy(), C.finalize(s0.cpu().numpy(), pass_tile0), rtol=1e-13)


def test_argument_errors_launch_nothing(fl):
    """VPC_ERR_ARG (1) from every entry, and the sentinel-filled outputs untouched."""
    lib, ptr, sp = fl.L.lib(), fl.L.ptr, fl.L.stream_ptr
    d = 12
    tile_row0, pass_tile0 = C.tables()
    o = _loss_operands(d, d)
    t = _dev(FC.flow_inputs(129, 2, 1.0)["t"])
    eps = _dev(FC.flow_inputs(129, 2, 1.0)["eps"])
    z, zlp = torch.full((R, 10), 7.0, device="cuda"), torch.full((R, 10), 7.0, device="cuda")
    scratch = fl.flow_eval_tiles_scratch(64, 12, "cuda")
    nbytes = scratch.numel() * 8
    stats = torch.full((12, 8), -3.0, dtype=torch.float64, device="cuda")
    out4 = torch.full((4,), -3.0, dtype=torch.float64, device="cuda")
    good, good_dev = _tabs(tile_row0)
    bad_tables = {"descending": tile_row0[::-1].copy(), "repeated": np.array([0, 4, 4, R]), "short of R": np.array([0, 64, R - 1]),
                  "past R": np.array([0, 64, R + 1]), "not from 0": np.array([1, 64, R])}

    def fwd(t_=t, eps_=eps, z_=z, zlp_=zlp, tab=good, dev=good_dev, n=12, ldt=100):
        return lib.vpc_flow_fwd_tiles(ptr(t_), ldt, ptr(eps_), ptr(z_), ptr(zlp_), R, ptr(tab), ptr(dev), n, sp())

    def ev(x=o["x"], m=o["m"], xm=o["xm"], z_=o["z"], zlp_=o["zlp"], tab=good, dev=good_dev, n=12, sc=scratch, nb=nbytes, st=stats,
           ldxm=d):
        return lib.vpc_flow_eval_tiles(ptr(x), ptr(m), ptr(xm), ldxm, ptr(z_), ptr(zlp_), R, d, ptr(tab), ptr(dev), n, 1.0, ptr(sc),
                                       nb, ptr(st), sp())

    pgood, pgood_dev = _tabs(pass_tile0)

    def fin(st=stats, tab=pgood, dev=pgood_dev, M=2, n=12, o4=out4):
        return lib.vpc_flow_eval_finalize(ptr(st), n, ptr(tab), ptr(dev), M, ptr(o4), sp())

    codes = {}
    for name in ("t_", "eps_", "z_", "zlp_", "tab", "dev"):
        codes["fwd null " + name] = fwd(**{name: None})
    codes["fwd n_tiles 0"], codes["fwd n_tiles -1"], codes["fwd ldt 99"] = fwd(n=0), fwd(n=-1), fwd(ldt=99)
    for name in ("x", "m", "xm", "z_", "zlp_", "tab", "dev", "sc", "st"):
        codes["eval null " + name] = ev(**{name: None})
    codes["eval n_tiles 0"], codes["eval ldxm < d"] = ev(n=0), ev(ldxm=d - 1)
    codes["eval scratch one byte short"] = ev(nb=int(lib.vpc_flow_eval_tiles_scratch(64, 12)) - 1)
    codes["eval scratch misaligned"] = lib.vpc_flow_eval_tiles(
        ptr(o["x"]), ptr(o["m"]), ptr(o["xm"]), d, ptr(o["z"]), ptr(o["zlp"]), R, d, ptr(good), ptr(good_dev), 12, 1.0,
        scratch.data_ptr() + 4, nbytes - 8, ptr(stats), sp())
    for what, tab in bad_tables.items():
        th, td = _tabs(tab)
        codes["fwd table " + what] = fwd(tab=th, dev=td, n=len(tab) - 1)
        codes["eval table " + what] = ev(tab=th, dev=td, n=len(tab) - 1)
    for name in ("st", "tab", "dev", "o4"):
        codes["finalize null " + name] = fin(**{name: None})
    codes["finalize M 0"], codes["finalize n_tiles 0"] = fin(M=0), fin(n=0)
    for what, tab in {"not ending at n_tiles": np.array([0, 8, 11]), "repeated": np.array([0, 12, 12])}.items():
        th, td = _tabs(tab)
        codes["finalize table " + what] = fin(tab=th, dev=td)
    torch.cuda.synchronize()
    assert {k: v for k, v in codes.items() if v != 1} == {}
    assert (z == 7).all() and (zlp == 7).all() and (stats == -3).all() and (out4 == -3).all()
    assert int(lib.vpc_flow_eval_tiles_scratch(0, 12)) == 0 and int(lib.vpc_flow_eval_tiles_scratch(64, 0)) == 0
    assert fwd() == 0 and ev() == 0 and fin() == 0  # and the same arguments, all valid, run
    torch.cuda.synchronize()
    assert (z != 7).any() and (stats[:, 6] == torch.from_numpy(np.diff(tile_row0)).cuda()).all() and (out4 != -3).all()


# ------------------------------------------------------------------------------------------------ 3. FlowEvaluator
def _model(fl, d, reg, model_seed=0):
    P = C.inputs(d, model_seed)["P"]
    model = (fl.REG_VAEFlow if reg else fl.VAEFlow)(d, C.HID, 10, 10, TP)
    sd = model.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in P.items()})
    model.load_state_dict(sd)
    return model.cuda()


def _case(d):
    inp = C.inputs(d)
    return _dev(inp["x"]), _dev(inp["mask"]), _dev(inp["eps"])


@pytest.mark.parametrize("reg", [True, False], ids=["reg", "van"])
@pytest.mark.parametrize("d", C.DS)
def test_evaluate_against_the_oracle(fl, d, reg):
    x, mask, eps = _case(d)
    ev = fl.FlowEvaluator(_model(fl, d, reg))
    out = ev.evaluate(x, mask, C.batches(), eps=eps)
    assert out.dtype == torch.float64 and out.shape == (4,) and out.is_cuda
    got, stats = out.cpu().numpy(), ev.tile_stats.cpu().numpy()
    ref, _ = C.oracle(d)
    _, pass_tile0 = C.tables()
    rows = ref[:, 6]
    assert (stats[:, 6] == rows).all() and (stats[:, 5] == ref[:, 5]).all()
    scale = (np.abs(ref[:, 1]) + np.abs(ref[:, 2])) / rows  # elbo: the two terms nearly cancel at d = 1
    v, vr = C.tile_values(stats), C.tile_values(ref)
    errs = dict(elbo=np.abs(v[:, 1] - vr[:, 1]) / scale, negll=np.abs(v[:, 2] - vr[:, 2]) / np.abs(vr[:, 2]),
                negll_imp=np.abs(v[:, 3] - vr[:, 3]) / np.abs(vr[:, 3]))
    seen = ~np.isnan(vr[:, 0])
    assert (np.isnan(v[:, 0]) == ~seen).all()
    errs["rmse"] = np.abs(v[seen, 0] - vr[seen, 0]) / np.abs(vr[seen, 0])
    print(f"d={d} reg={reg}: worst per-tile relative errors", {k: float(f"{e.max():.3g}") for k, e in errs.items()})
    for k, e in errs.items():
        assert (e <= C.TOL).all(), (k, e)
    # the four results: the finalize of the device's own table (the kernel's arithmetic), and of the oracle's
    own, want = C.finalize(stats, pass_tile0), C.finalize(ref, pass_tile0)
    np.testing.assert_allclose(got, own, rtol=1e-13, equal_nan=True)
    magnitude = ref.copy()
    magnitude[:, 0] = np.abs(ref[:, 1]) + np.abs(ref[:, 2])
    fscale = C.finalize(magnitude, pass_tile0)[1]
    assert np.isnan(got[0]) == np.isnan(want[0])
    if not np.isnan(want[0]):
        assert abs(got[0] - want[0]) <= C.TOL * abs(want[0])
    assert abs(got[1] - want[1]) <= C.TOL * fscale
    assert abs(got[2] - want[2]) <= C.TOL * abs(want[2]) and abs(got[3] - want[3]) <= C.TOL * abs(want[3])
    # chunks: max_rows = 128 breaks the 12 tiles into 3 runs; nothing may depend on it
    chunked = fl.FlowEvaluator(ev.model, max_rows=128)
    out3 = chunked.evaluate(x, mask, C.batches(), eps=eps)
    assert len(chunked._layouts[next(iter(chunked._layouts))]["chunks"]) == 3
    assert _same_bits(out3, out) and _same_bits(chunked.tile_stats, ev.tile_stats)
    with pytest.raises(fl.L.VpcError, match="tile 6 has 64 rows"):
        fl.FlowEvaluator(ev.model, max_rows=63).evaluate(x, mask, C.batches(), eps=eps)


def test_device_draws(fl):
    from vpc_amd import ops
    d = 12
    x, mask, _ = _case(d)
    model = _model(fl, d, True)
    a, b, c = fl.FlowEvaluator(model, seed=5), fl.FlowEvaluator(model, seed=5, max_rows=128), fl.FlowEvaluator(model, seed=6)
    for call in range(2):  # the second call draws at the offset the rule returns
        ra, rb, rc = (e.evaluate(x, mask, C.batches()) for e in (a, b, c))
        assert torch.isfinite(ra).all()
        assert _same_bits(ra, rb) and _same_bits(a.tile_stats, b.tile_stats) and not _same_bits(ra, rc)
        want = torch.empty(R * 10, device="cuda")
        ops.fill_normal(want, 5, call * 645)
        assert _same_bits(a.eps.reshape(-1), want) and _same_bits(b.eps.reshape(-1), want)
        assert a.rng_offset == (call + 1) * 645
    first = fl.FlowEvaluator(model, seed=5).evaluate(x, mask, C.batches())
    assert not _same_bits(first, ra)  # the second call did not repeat the first call's draws
    with pytest.raises(fl.L.VpcError):
        fl.FlowEvaluator(torch.nn.Linear(2, 2))


# ------------------------------------------------------------------------------------------------ harness
class _Recorder:
    """Stands in for the loaded library: records every vpc_* symbol fetched, hands out the real one (tests/test_trainer_images.py)."""

    def __init__(self, real):
        self.real, self.names = real, []

    def __getattr__(self, name):
        if name.startswith("vpc_"):
            self.names.append(name)
        return getattr(self.real, name)


def _golden_model(fl, g, cls, prefix="param."):
    model = cls(g["x"].shape[1], int(g["hid"]), 10, 10, TP)
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(prefix)})
    return model.cuda()


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_eval_vae_batched_on_the_reference_checkpoint(fl, kind, tmp_path, monkeypatch):
    """eval_vae(engine="batched") where tests/test_flow_gpu.py::test_eval_vae_flow_interop runs the chain: the same loaders, the
    four reference-named files, every value within the spread of what the reference wrote over six seeds; at most 14 library
    calls per loader stage."""
    import vpc_amd
    from vpc_amd import _lib
    g = load_golden(f"flow_eval_{kind}_d12.npz")
    vae_type = "reg_flow1" if kind == "reg" else "vanilla_flow1"
    monkeypatch.chdir(tmp_path)
    model = _golden_model(fl, g, fl.REG_VAEFlow if kind == "reg" else fl.VAEFlow)
    x, mask = torch.from_numpy(g["x"]), torch.from_numpy(g["mask"])
    loaders = [([(x[:24], mask[:24]), (x[24:], mask[24:])], "test")]
    args = (40, 12, int(g["hid"]), 10)
    rest = (10, "toy", TP, "exp", vae_type, 100, 1, 1)
    res = vpc_amd.eval_vae(loaders, *args, int(g["M"]), *rest, alpha=0.5, p_missingness=30, reg_type="kl_reg", model=model,
                           engine="batched", seed=0)["test"]
    fam = "".join(c for c in vae_type if not c.isdigit())
    files = sorted(os.path.join(sub, f) for sub in ("rest", "elbos")
                   for f in os.listdir(os.path.join("experiments", "exp", "toy", sub, fam)))
    assert [os.path.basename(f) for f in files] == [str(s) for s in g["result_files"]]
    by_name = {"vae_elbo": "elbo", "negative_llh_q_imputed": "negll_imp", "negative_llh_imputed": "negll_imp",
               "negative_llh_q": "negll", "negative_llh": "negll", "rmse": "rmse"}
    for i, name in enumerate(g["result_files"]):
        key = next(v for k, v in by_name.items() if f"_{k}_" in str(name))
        ref = g["values"][:, i]
        lo, hi = ref.min() - 3 * ref.std() - 1e-3 * abs(ref.mean()), ref.max() + 3 * ref.std() + 1e-3 * abs(ref.mean())
        got = float(res[key])
        assert lo <= got <= hi, (str(name), got, ref)
        sub, f = os.path.split(files[i])
        assert float(torch.load(os.path.join("experiments", "exp", "toy", sub, fam, f), weights_only=True)) == got
    # the launch budget at M = 2, two loader stages, counted cold (the scratch query of a new layout included)
    two = loaders + [([(x[:40], mask[:40])], "train")]
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    vpc_amd.eval_vae(two, *args, 2, *rest, alpha=0.5, p_missingness=30, reg_type="kl_reg", model=model, engine="batched",
                     save=False)
    monkeypatch.undo()
    assert len(rec.names) <= 2 * 14, rec.names
    per_stage = ["vpc_flow_prep"] + ["vpc_linear_fwd"] * 3 + ["vpc_flow_fwd_tiles"] + ["vpc_linear_fwd"] * 5 + \
        ["vpc_flow_eval_tiles", "vpc_flow_eval_finalize"]
    assert [n for n in rec.names if n != "vpc_flow_eval_tiles_scratch"] == per_stage * 2
    assert rec.names.count("vpc_flow_eval_tiles_scratch") <= 2


def test_eval_vae_batched_refusals(fl):
    import vpc_amd
    x, mask = torch.rand(8, 12), torch.rand(8, 12) < 0.7
    loaders = [([(x, mask)], "test")]
    call = lambda model, vae_type, **kw: vpc_amd.eval_vae(loaders, 40, 12, 64, 10, 2, 10, "toy", TP, "exp", vae_type, 100, 1, 1,
                                                          reg_type="kl_reg", model=model, save=False, **kw)
    with pytest.raises(vpc_amd.VpcError, match="not Reg_VAE"):
        call(vpc_amd.Reg_VAE(12, 500, 10, 10, TP, "exp", "kl_reg").cuda(), "reg_vae1", engine="batched")
    with pytest.raises(vpc_amd.VpcError, match="stage='train'"):
        call(fl.REG_VAEFlow(12, 64, 10, 10, TP).cuda(), "reg_flow1", engine="batched", stage="train")
    with pytest.raises(vpc_amd.VpcError, match="engine="):
        call(fl.VAEFlow(12, 64, 10, 10, TP).cuda(), "vanilla_flow1", engine="fused")
    # the vanilla class has no train-stage p pass: stage does not matter to it
    r = call(fl.VAEFlow(12, 64, 10, 10, TP).cuda(), "vanilla_flow1", engine="batched", stage="train")["test"]
    assert all(torch.isfinite(v) for v in r.values())


def test_eval_sweep_batched(fl, monkeypatch):
    """Two flow members and one Reg_VAE member: per member what the single calls return; the default engine keeps the flow
    members on the chain."""
    import vpc_amd
    from vpc_amd import _lib
    torch.manual_seed(3)
    ms = [fl.REG_VAEFlow(12, 64, 10, 10, TP).cuda(), vpc_amd.Reg_VAE(12, 500, 10, 10, TP, "exp", "kl_reg").cuda(),
          fl.VAEFlow(12, 64, 10, 10, TP).cuda()]
    cfgs = [dict(vae_type="reg_flow1", alpha=0.5, seed=4), dict(vae_type="reg_vae1", alpha=0.5, seed=5),
            dict(vae_type="vanilla_flow1", seed=6)]
    x, mask = torch.rand(70, 12), torch.rand(70, 12) < 0.7
    loader = [(x[:32], mask[:32]), (x[32:64], mask[32:64]), (x[64:], mask[64:])]
    sweep = lambda cf, mm, **kw: vpc_amd.eval_sweep([(loader, "test")], cf, 30, 12, 64, 10, 2, 10, "toy", TP, "exp", 5, 1, 1,
                                                    reg_type="kl_reg", models=mm, save=False, **kw)
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    out = sweep(cfgs, ms, engine="batched")
    monkeypatch.undo()
    assert rec.names.count("vpc_flow_eval_tiles") == 2 and "vpc_flow_loss" not in rec.names and "vpc_flow_fwd" not in rec.names
    for g in (0, 2):
        single = vpc_amd.eval_vae([(loader, "test")], 30, 12, 64, 10, 2, 10, "toy", TP, "exp", cfgs[g]["vae_type"], 5, 1, 1,
                                  alpha=cfgs[g]["alpha"] if "alpha" in cfgs[g] else 1.0, reg_type="kl_reg", model=ms[g],
                                  save=False, engine="batched", seed=cfgs[g]["seed"])
        for k in ("rmse", "elbo", "negll", "negll_imp"):
            assert _same_bits(out[g]["test"][k], single["test"][k]) and torch.isfinite(single["test"][k]), (g, k)
    dense = sweep([cfgs[1]], [ms[1]])
    for k in ("rmse", "elbo", "negll", "negll_imp"):
        assert _same_bits(out[1]["test"][k], dense[0]["test"][k]), k
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    torch.manual_seed(0)
    chain = sweep(cfgs, ms)
    monkeypatch.undo()
    assert "vpc_flow_eval_tiles" not in rec.names and rec.names.count("vpc_flow_loss") == 2 * 2 * 3
    for g in (0, 2):  # another draw of the same estimator
        assert all(torch.isfinite(chain[g]["test"][k]) for k in chain[g]["test"])
