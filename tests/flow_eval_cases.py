"""Layouts, inputs and float64 references of the batched flow evaluation (flow.FlowEvaluator, csrc/vpc_floweval.hip), shared by
tests/test_flow_eval_cpu.py and tests/test_flow_eval_gpu.py, from seeded numpy generators.

Two Monte-Carlo passes of 129 rows each with different partitions into batches ("tiles"):

    pass 0   1, 3, 4, 5, 25, 26, 64, 1      pass 1   64, 37, 27, 1

vpc_flow_fwd_tiles runs 25.6 rows per workgroup and vpc_flow_eval_tiles sums 4 rows per double partial: the tile boundaries lie
inside a workgroup's 26 rows (1, 4, 8, 13), inside a 4-row partial block (tiles of 1, 3, 5, 25, 26, 37, 27 rows) and on one (4,
64), the first and the last tile hold one row, and the passes differ in their tile count, so that a plain mean over all tiles is
not the estimator."""
import functools

import numpy as np

import flow_oracle as FO

L = FO.L
HID = 64
DS = (1, 12, 65)
PASS_TILES = ([1, 3, 4, 5, 25, 26, 64, 1], [64, 37, 27, 1])
ROWS = sum(sum(p) for p in PASS_TILES)  # 258
TOL = 2e-5  # what tests/test_flow_gpu.py holds forward_loss to against the same oracle


def batches(pass_tiles=PASS_TILES):
    """M lists of (row_lo, row_hi), as harness._gather_passes returns them."""
    out, r = [], 0
    for tiles in pass_tiles:
        pr = []
        for n in tiles:
            pr.append((r, r + n))
            r += n
        out.append(pr)
    return out


def tables(pass_tiles=PASS_TILES):
    tile_row0 = np.concatenate([[0], np.cumsum([n for p in pass_tiles for n in p])]).astype(np.int64)
    pass_tile0 = np.concatenate([[0], np.cumsum([len(p) for p in pass_tiles])]).astype(np.int64)
    return tile_row0, pass_tile0


@functools.lru_cache(maxsize=None)
def inputs(d, model_seed=0):
    """Parameters (FO.init_params, hid 64), x, mask (about 70 % observed), eps for the 258 stacked rows; fp32 / bool."""
    rng = np.random.default_rng([d, 0, 9])
    x = rng.random((ROWS, d)).astype(np.float32)
    mask = rng.random((ROWS, d)) < 0.7
    eps = rng.normal(size=(ROWS, L)).astype(np.float32)
    return dict(P=FO.init_params(d, HID, model_seed), x=x, mask=mask, eps=eps)


@functools.lru_cache(maxsize=None)
def oracle(d, model_seed=0):
    """Per tile, in float64 (FO.step, the vanilla form: the evaluate-stage loss of REG_VAEFlow is the same loss_q):
    stats [n_tiles][8] as vpc_flow_eval_tiles lays them out, and the flagged spline decisions of every tile."""
    inp = inputs(d, model_seed)
    tile_row0, _ = tables()
    stats, n_flagged = np.zeros((len(tile_row0) - 1, 8)), 0
    for t, (lo, hi) in enumerate(zip(tile_row0[:-1], tile_row0[1:])):
        x, m, e = inp["x"][lo:hi].astype(np.float64), inp["mask"][lo:hi].astype(np.float64), inp["eps"][lo:hi]
        r = FO.step(inp["P"], x, m, None, e[None])
        rows = hi - lo
        re_q, re_imp = r["llh"][0] * rows, r["llh"][1] * rows
        xm = r["fwd"]["x_mean_q"]
        stats[t] = [r["loss"] * rows, re_q, r["loss"] * rows - re_q, re_imp, np.sum((xm - x) ** 2 * (1 - m)), np.sum(1 - m),
                    rows, 0]
        # the flow cache of the q pass: recomputed here, FO.step does not return it
        ecache, _ = FO.mlp({k: np.asarray(v, np.float64) for k, v in inp["P"].items()}, FO.ENC, np.concatenate([x * m, m], 1))
        cache = FO.flow_fwd(ecache[-1], e.astype(np.float64))[2]
        if cache is not None:
            n_flagged += int(FO.flagged(FO.flow_flags(cache)).sum())
    return stats, n_flagged


def tile_values(stats):
    """[n_tiles][4] = rmse, elbo, negll, negll_imp of every tile (0 / 0 = NaN where a tile has no unobserved entry)."""
    stats = np.asarray(stats, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = np.sqrt(stats[:, 4] / stats[:, 5])
    rows = stats[:, 6]
    return np.stack([rmse, stats[:, 0] / rows, stats[:, 1] / rows, stats[:, 3] / rows], 1)


def finalize(stats, pass_tile0):
    """evaluate.py:232-245 restated: the mean over each pass's tiles of the per-tile values, then the mean over the passes, both
    summed in table order -> [4]."""
    v = tile_values(stats)
    total = np.zeros(4)
    for lo, hi in zip(pass_tile0[:-1], pass_tile0[1:]):
        s = np.zeros(4)
        for t in range(lo, hi):
            s = s + v[t]
        total = total + s / (hi - lo)
    return total / (len(pass_tile0) - 1)
