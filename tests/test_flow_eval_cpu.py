"""Host side of the batched flow evaluation (flow.FlowEvaluator) and the preconditions of its GPU cases.  No GPU:
the tile tables from harness._gather_passes' ranges, the chunk split, the counter rule, the numpy restatement of the finalize
against evaluate.py:232-245's order, and the float64 oracle's spline decisions on the committed inputs."""
import numpy as np
import pytest
import torch

import flow_eval_cases as C
import flow_oracle as FO
from vpc_amd import VpcError, flow, harness, trainer


def test_tables_from_gathered_ranges():
    """_gather_passes on a list-of-batches loader yields the ranges; tile_tables turns them into the two tables."""
    x, m = torch.rand(129, 3), torch.rand(129, 3) < 0.7
    loader = [(x[lo:hi], m[lo:hi]) for lo, hi in ((0, 64), (64, 101), (101, 128), (128, 129))]
    gx, gm, ranges = harness._gather_passes([loader], 2, 3, "cpu")
    assert gx.shape == (258, 3) and torch.equal(gx[:129], x) and torch.equal(gx[129:], x) and torch.equal(gm[129:], m)
    assert ranges == [[(0, 64), (64, 101), (101, 128), (128, 129)], [(129, 193), (193, 230), (230, 257), (257, 258)]]
    assert flow.tile_tables(ranges) == ([0, 64, 101, 128, 129, 193, 230, 257, 258], [0, 4, 8])
    tile_row0, pass_tile0 = flow.tile_tables(C.batches())
    t0, p0 = C.tables()
    assert tile_row0 == t0.tolist() and pass_tile0 == p0.tolist() == [0, 8, 12] and tile_row0[-1] == C.ROWS == 258


@pytest.mark.parametrize("bad", [[[(1, 3)]], [[(0, 3), (4, 5)]], [[(0, 3), (3, 3)]], [[(0, 3)], []], []])
def test_tables_refuse(bad):
    with pytest.raises(VpcError):
        flow.tile_tables(bad)


def test_chunks_break_at_tile_boundaries_only():
    tile_row0 = C.tables()[0].tolist()
    assert flow.eval_chunks(tile_row0, 258) == [(0, 12)] == flow.eval_chunks(tile_row0, 1 << 20)
    for max_rows in (64, 65, 100, 128, 129, 200, 257):
        ch = flow.eval_chunks(tile_row0, max_rows)
        assert ch[0][0] == 0 and ch[-1][1] == 12 and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        rows = [tile_row0[hi] - tile_row0[lo] for lo, hi in ch]
        assert all(0 < r <= max_rows for r in rows) and sum(rows) == 258
        # greedy: the next tile would not have fitted
        assert all(tile_row0[hi + 1] - tile_row0[lo] > max_rows for lo, hi in ch[:-1])
    assert flow.eval_chunks(tile_row0, 100) == [(0, 6), (6, 8), (8, 9), (9, 12)]
    assert flow.eval_chunks(tile_row0, 128) == [(0, 7), (7, 10), (10, 12)]  # the 3 chunks the GPU test forces
    with pytest.raises(VpcError, match="tile 6 has 64 rows"):
        flow.eval_chunks(tile_row0, 63)


def test_counter_rule():
    """One Philox call per 4 floats of the flat [10 rows] array; the offset advances by ceil(10 rows / 4)."""
    r = trainer.flow_eval_draw_counters
    assert r(0, 258) == (0, 645) and r(645, 258) == (645, 1290)
    assert r(7, 1) == (7, 10) and r(0, 2) == (0, 5) and r(0, 3) == (0, 8) and r(0, 4) == (0, 10)
    off = 0
    for rows in (1, 129, 8000):  # successive calls never share a counter
        lo, off = r(off, rows)
        assert off - lo == -(-10 * rows // 4)


def test_numpy_finalize_is_the_reference_order():
    """C.finalize against evaluate.py:232-245 spelled with torch on per-batch values: mean over a pass's batches, then over the
    passes - not the mean over all tiles, which the pass-dependent tile count tells apart."""
    rng = np.random.default_rng(3)
    _, pass_tile0 = C.tables()
    stats = np.zeros((12, 8))
    stats[:, :4] = rng.normal(size=(12, 4)) * 50
    stats[:, 4], stats[:, 5] = rng.random(12) * 5, rng.integers(1, 40, 12)
    stats[:, 6] = [n for p in C.PASS_TILES for n in p]
    got = C.finalize(stats, pass_tile0)
    v = torch.from_numpy(C.tile_values(stats))
    passes = [torch.stack([v[t] for t in range(lo, hi)]).mean(0) for lo, hi in zip(pass_tile0[:-1], pass_tile0[1:])]
    ref = torch.stack(passes).mean(0).numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-13)
    assert np.abs(got - C.tile_values(stats).mean(0)).max() > 1e-3
    stats[2, 5] = stats[2, 4] = 0  # a tile with no unobserved entry: NaN for the rmse alone
    got = C.finalize(stats, pass_tile0)
    assert np.isnan(got[0]) and np.isfinite(got[1:]).all()


@pytest.mark.parametrize("d", C.DS)
def test_no_tie_flagged_decision_in_the_committed_inputs(d):
    """The GPU cases compare against float64 at 2e-5: no spline decision of any tile may sit on a knot in float64."""
    stats, n_flagged = C.oracle(d)
    assert n_flagged == 0
    assert np.isfinite(stats[:, :4]).all() and (stats[:, 6] == [n for p in C.PASS_TILES for n in p]).all()


def test_the_flag_assertion_is_not_vacuous():
    """The same inputs under another model (parameter seed 22 at d = 12) do hold one flagged decision."""
    assert C.oracle(12, 22)[1] == 1


def test_eval_sweep_routes_flow_members_by_engine(monkeypatch):
    """engine="batched": the flow members reach eval_vae with engine="batched" and their config's seed; the default engine, and
    every member of another family, reach it as before."""
    import vpc_amd
    TP = {"batch_size": 8, "patience": 1}
    ms = [flow.REG_VAEFlow(12, 64, 10, 10, TP), vpc_amd.MIWAE(12, 64, 3, 10, TP, 3, 1), flow.VAEFlow(12, 64, 10, 10, TP)]
    cfgs = [dict(vae_type="reg_flow1", alpha=0.5, seed=4), dict(vae_type="vanilla_MIWAE1", seed=5), dict(vae_type="vanilla_flow1", seed=6)]
    seen = []

    def stub_eval_vae(list_loaders, *a, model=None, save=True, **kw):
        seen.append((model, kw))
        return {s: "alone" for _, s in list_loaders}

    monkeypatch.setattr(harness, "eval_vae", stub_eval_vae)
    loader = [(torch.rand(8, 12), torch.rand(8, 12) < 0.7)]
    sweep = lambda **kw: harness.eval_sweep([(loader, "test")], cfgs, 30, 12, 64, 3, 2, 10, "uci", TP, "e", 7, 1, 1,
                                            device=torch.device("cpu"), models=ms, save=False, **kw)
    assert sweep(engine="batched") == [{"test": "alone"}] * 3
    assert [(m, kw) for m, kw in seen] == [(ms[0], dict(engine="batched", seed=4)), (ms[1], {}), (ms[2], dict(engine="batched", seed=6))]
    del seen[:]
    sweep()
    assert [kw for _, kw in seen] == [{}, {}, {}]
    with pytest.raises(VpcError, match="engine="):
        sweep(engine="stream")


def test_evaluator_refuses_other_models_and_bad_limits():
    with pytest.raises(VpcError, match="VAEFlow and REG_VAEFlow"):
        flow.FlowEvaluator(torch.nn.Linear(2, 2))
    with pytest.raises(VpcError, match="max_rows"):
        flow.FlowEvaluator(flow.VAEFlow(12, 64, 10, 10, {"batch_size": 8, "patience": 1}), max_rows=0)


def test_d1_terms_nearly_cancel():
    """Why the elbo is held relative to (|RE_q| + |KL_q|) / rows: at d = 1 the oracle's loss per row spans a wide range."""
    stats, _ = C.oracle(1)
    per_row = stats[:, 0] / stats[:, 6]
    assert per_row.min() < 0 < 100 < per_row.max()
