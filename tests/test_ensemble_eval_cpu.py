"""The host side of the ensemble evaluation (ensemble.EnsembleEvaluator, harness.eval_sweep): the tile / batch / pass tables,
the draw-counter rule and eval_sweep's split of a mixed list of runs into ensembles and one-by-one fallbacks.  CPU only:
nothing is launched (the evaluator and eval_vae are stubbed where eval_sweep would reach them)."""
import numpy as np
import pytest
import torch

import vpc_amd as vpc
from vpc_amd import ensemble as E
from vpc_amd import harness as H
from vpc_amd.trainer import eval_draw_counters

TP = {"batch_size": 8, "patience": 1}
L = 10


# ----------------------------------------------------------------------------------------------- tables
def _check_tables(tb, N, ranges_per_pass):
    """Every structural property of the tables, against the batch ranges they were built from."""
    M = len(ranges_per_pass)
    flat = [(p, lo, hi) for p, rs in enumerate(ranges_per_pass) for lo, hi in rs]
    assert tb.batches.shape == (len(flat), 4) and tb.passes.shape == (M, 2)
    assert tb.R == sum(hi - lo for _, lo, hi in flat)
    draw_seen = np.zeros(tb.R, int)
    t_next = 0
    for b, (p, lo, hi) in enumerate(flat):
        rows, pas, t0, nt = tb.batches[b]
        assert (rows, pas) == (hi - lo, p)
        assert t0 == t_next and nt == (hi - lo + 15) // 16  # consecutive tiles, 16 rows each but the last
        t_next += nt
        covered = []
        for t in range(t0, t0 + nt):
            xrow, valid, drow, bi = tb.tiles[t]
            assert bi == b  # no tile straddles a batch: all its rows lie in [lo, hi) of ITS batch
            assert 1 <= valid <= 16 and lo <= xrow and xrow + valid <= hi
            assert valid == 16 or t == t0 + nt - 1  # only a batch's last tile is ragged
            covered += list(range(xrow, xrow + valid))
            draw_seen[drow:drow + valid] += 1
        assert covered == list(range(lo, hi))
    assert t_next == tb.tiles.shape[0]
    assert np.all(draw_seen == 1)  # draw rows are disjoint across tiles, batches and passes, and cover [0, R)
    b_next = 0
    for p, rs in enumerate(ranges_per_pass):
        assert tuple(tb.passes[p]) == (b_next, len(rs))
        b_next += len(rs)
    assert tb.tiles.dtype == tb.batches.dtype == tb.passes.dtype == np.int64


@pytest.mark.parametrize("N,bs,M", [(37, 16, 2), (37, 24, 2), (21, 16, 1), (64, 64, 3), (5, 100, 2), (1600, 64, 2)])
def test_tables_from_batch_size(N, bs, M):
    tb = E.build_eval_tables(N, bs, M)
    ranges = [[(lo, min(lo + bs, N)) for lo in range(0, N, bs)]] * M
    _check_tables(tb, N, ranges)
    # M passes over an unshuffled data set read the same data rows with different draw rows: row n of pass p draws as p N + n
    per = tb.tiles.shape[0] // M
    for p in range(M):
        blk = tb.tiles[p * per:(p + 1) * per]
        assert np.array_equal(blk[:, 0], tb.tiles[:per, 0]) and np.array_equal(blk[:, 2], p * N + blk[:, 0])
    if (N, bs) == (37, 24):  # a batch of two tiles with 8 valid rows in the second, then a 13-row batch
        assert tb.tiles[:3, :2].tolist() == [[0, 16], [16, 8], [24, 13]]


def test_tables_from_explicit_batches():
    ranges = [[(0, 16), (16, 32)], [(32, 37), (37, 64), (0, 1)]]  # any row ranges, in any order, per pass
    tb = E.build_eval_tables(64, M=2, batches=ranges)
    _check_tables(tb, 64, ranges)
    assert tb.tiles[:, 2].tolist() == [0, 16, 32, 37, 53, 64]  # draw rows count on from batch to batch


@pytest.mark.parametrize("kw", [dict(), dict(batch_size=16, batches=[[(0, 4)]]), dict(batch_size=0), dict(batches=[[(0, 4)]], M=2),
                                dict(batches=[[]]), dict(batches=[[(3, 3)]]), dict(batches=[[(0, 38)]]), dict(batches=[[(-1, 4)]]),
                                dict(batch_size=4, M=0)])
def test_tables_refuse_bad_layouts(kw):
    with pytest.raises(vpc.VpcError):
        E.build_eval_tables(37, **kw)


def test_layout_key():
    k = E.eval_layout_key
    assert k(37, 16, 2) == k(37, batch_size=16, M=2)
    assert len({k(37, 16, 2), k(38, 16, 2), k(37, 24, 2), k(37, 16, 3)}) == 4  # N, the batch layout and M all count
    a = k(37, M=1, batches=[[(0, 16), (16, 37)]])
    assert a == k(37, M=1, batches=[[[0, 16], (np.int64(16), 37)]])  # the same ranges, spelled differently
    assert a != k(37, M=1, batches=[[(0, 16), (16, 36)]])
    assert a != k(37, 16, 1)  # (an explicit layout is not compared with the batch_size that would produce it)
    hash(a)


# ----------------------------------------------------------------------------------------------- draw counters
def test_eval_draw_counter_rule():
    """One Philox group per 4 floats of the [R, 16] eps rows; the offset advances by what the call consumed."""
    off, nxt = eval_draw_counters(0, 74)
    assert (off, nxt) == (0, 74 * 4)
    off2, nxt2 = eval_draw_counters(nxt, 10)
    assert (off2, nxt2) == (296, 336)  # the next call starts where the last one ended: no counter is used twice
    assert eval_draw_counters(5, 3, pitch=8) == (5, 11)
    # the rule agrees with the tables: R draw rows -> 4 R counters
    tb = E.build_eval_tables(37, 16, 2)
    assert eval_draw_counters(0, tb.R)[1] == 4 * 2 * 37


# ----------------------------------------------------------------------------------------------- eval_sweep's grouping
def _models():
    return [vpc.Reg_VAE(14, 500, 10, L, TP, "e", "kl_reg"), vpc.vanilla_VAE(14, 500, 10, L, TP, "e"),
            vpc.Reg_VAE(14, 500, 10, L, TP, "e", "kl_reg"), vpc.Reg_VAE_mask(14, 500, 10, L, TP, "e", "kl_reg"),
            vpc.Reg_VAE(14, 500, 10, L, TP, "e", "ml_reg"), vpc.vanilla_VAE(200, 500, 10, L, TP, "e"),
            vpc.MIWAE(14, 500, 10, L, TP, 1, 1)]


def test_eval_groups():
    ms = _models()
    groups, alone = H.eval_groups(ms)
    assert groups == {(vpc.Reg_VAE, "kl_reg"): [0, 2], (vpc.vanilla_VAE, None): [1], (vpc.Reg_VAE, "ml_reg"): [4]}
    assert alone == [3, 5, 6]  # mask-augmented, wide, another family


def test_eval_sweep_routes_members(monkeypatch):
    ms = _models()[:4]
    cfgs = [dict(vae_type="reg_vae1", alpha=0.5, seed=11), dict(vae_type="vanilla_vae1", seed=12),
            dict(vae_type="reg_vae2", alpha=0.5, p_missingness=50, seed=13), dict(vae_type="reg_vae1_mask_augm", seed=14)]
    g = torch.Generator().manual_seed(0)
    x, mk = torch.rand(21, 14, generator=g), torch.rand(21, 14, generator=g) < 0.7
    loader = [(x[:16], mk[:16]), (x[16:], mk[16:])]
    calls = {"ens": [], "alone": []}

    class StubEvaluator:
        def __init__(self, models, seeds=None):
            self.models, self.seeds = list(models), list(seeds)

        def evaluate(self, x, mask, M=1, *, batches, epoch, beta, beta_annealing):
            calls["ens"].append((self.models, self.seeds, tuple(x.shape), batches, M, epoch, beta))
            return torch.arange(4.0).repeat(len(self.models), 1) + 10 * torch.tensor(self.seeds)[:, None]

    def stub_eval_vae(list_loaders, *a, model=None, save=True, **kw):
        calls["alone"].append((model, a[9], a[14], a[16], save))  # vae_type, alpha, p_missingness by position
        return {s: "alone" for _, s in list_loaders}

    monkeypatch.setattr(H, "EnsembleEvaluator", StubEvaluator)
    monkeypatch.setattr(H, "eval_vae", stub_eval_vae)
    out = H.eval_sweep([(loader, "train"), (loader[:1], "test")], cfgs, 30, 14, 500, 10, 2, L, "uci", TP, "e", 7, 1, 1,
                       device=torch.device("cpu"), beta=0.7, models=ms, save=False)
    # the mask-augmented member went through eval_vae alone, with its own config
    assert [c[0] for c in calls["alone"]] == [ms[3]] and calls["alone"][0][1:] == ("reg_vae1_mask_augm", 1.0, 30, False)
    assert out[3] == {"train": "alone", "test": "alone"}
    # the two Reg_VAE share one evaluator, the vanilla_VAE has its own; one evaluate call per (group, loader stage), over the
    # batches of both passes gathered behind each other
    by_models = {tuple(id(m) for m in c[0]): c for c in calls["ens"]}
    assert len(calls["ens"]) == 4 and set(by_models) == {(id(ms[0]), id(ms[2])), (id(ms[1]),)}
    shapes = sorted((len(c[0]), c[2], tuple(map(tuple, c[3]))) for c in calls["ens"])
    assert shapes == sorted([(2, (42, 14), (((0, 16), (16, 21)), ((21, 37), (37, 42)))), (2, (32, 14), (((0, 16),), ((16, 32),))),
                             (1, (42, 14), (((0, 16), (16, 21)), ((21, 37), (37, 42)))), (1, (32, 14), (((0, 16),), ((16, 32),)))])
    assert all(c[4] == 2 and c[5] == 7 and c[6] == 0.7 for c in calls["ens"])
    assert by_models[(id(ms[0]), id(ms[2]))][1] == [11, 13]
    for g, seed in ((0, 11), (1, 12), (2, 13)):
        for stage in ("train", "test"):
            r = out[g][stage]
            assert [float(r[k]) for k in ("rmse", "elbo", "negll", "negll_imp")] == [10.0 * seed + i for i in range(4)]


def test_eval_sweep_checks_list_lengths():
    with pytest.raises(vpc.VpcError, match="models"):
        H.eval_sweep([], [dict(vae_type="reg_vae1")], 30, 14, 500, 10, 1, L, "uci", TP, "e", 1, 1, 1, models=[])
    with pytest.raises(vpc.VpcError, match="loaders"):
        H.eval_sweep(None, [dict(vae_type="reg_vae1")], 30, 14, 500, 10, 1, L, "uci", TP, "e", 1, 1, 1, models=[None], loaders=[])
