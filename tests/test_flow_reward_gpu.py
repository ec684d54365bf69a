"""Config 5 reward of the flow models on the GPU (vpc_flow_reward_matrix, csrc/vpc_flowreward.hip) against the values
recorded from the reference (tests/golden/make_golden_flow_reward.py) and the float64 oracle
(tests/flow_reward_oracle.py).

Tolerance (flow_reward_oracle.compare): |R_gpu - R_ref| <= 8e-4 * S, S the largest |z_log_prob| the oracle met - the
2e-5-of-max the flow forward is held to (tests/test_flow_gpu.py) through 2 chains x 10 latents x a difference of 2
values.  An entry is left out only when the oracle reports a layer-2/3 bin position within the golden's `delta` of an
integer; at most 5 % of a case's unobserved entries may be.
"""
import os

import numpy as np
import pytest
import torch

import flow_reward_cases as FC
import flow_reward_oracle as FR
import vpc_amd as vpc
from conftest import load_golden

pytestmark = pytest.mark.gpu
fl = vpc.flow


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(R, ref, res, delta, tag, cap=True):
    err, bound, share = FR.compare(R, ref, res["edge"], res["S"], delta)
    print(tag, "err", err, "bound", bound, "flagged", share, "S", res["S"])
    assert np.array_equal(R == -1e4, np.asarray(ref) == -1e4), tag   # observed entries are exactly -1e4
    if cap:
        assert share <= FR.MAX_FLAGGED, tag
    assert err <= bound, tag


def _golden_case(kind, name):
    g = load_golden(name)
    m = FC.flow_model(fl, kind, g["x"].shape[1], int(g["hid"]), FC.params_of(g))
    return g, m


@pytest.mark.parametrize("kind,name", FC.GOLDEN, ids=FC.IDS)
def test_reward_matrix_matches_reference(kind, name):
    g, m = _golden_case(kind, name)
    R = vpc.flow_reward_matrix(m, _t(g["x"]), _t(g["mask"]), _t(g["im"]), eps=_t(g["eps"])).cpu().numpy()
    res = FR.reward_matrix(FC.params_of(g), g["x"], g["mask"], g["im"], g["eps"])
    _check(R, g["R"], res, float(g["delta"]), name)
    empty = [u for u in range(R.shape[1]) if (g["mask"][:, u] != 0).all()]
    assert empty and all(np.all(R[:, u] == -1e4) for u in empty)


@pytest.mark.parametrize("kind,name", FC.GOLDEN[:2], ids=FC.IDS[:2])
def test_drop_in_functions_match_reference(kind, name):
    g, m = _golden_case(kind, name)
    x, mask, im, eps = _t(g["x"]), _t(g["mask"]), _t(g["im"]), _t(g["eps"])
    M = int(g["M"])
    res = FR.reward_matrix(FC.params_of(g), g["x"], g["mask"], g["im"], g["eps"])
    bound = FR.TOL_PER_S * res["S"]
    delta = float(g["delta"])
    for u in (0, 3):
        loc = np.where(g["mask"][:, u] == 0)[0]
        keep = res["edge"][loc, u] > delta
        loc_t = torch.from_numpy(loc).cuda()
        got = vpc.R_lindley_chain_ratio_version(u, x, mask, M, m, im, loc, eps=eps[u][:, :, loc_t]).cpu().numpy()
        assert np.abs(got - g["R"][loc, u])[keep].max() <= bound
        # the API path, as evaluate.py:653-661 composes it
        tx = x.clone()
        acc = torch.zeros(len(loc), device="cuda")
        for s in range(M):
            tx[loc_t, u] = im[s, loc_t, u]
            acc += vpc.chaini_I_ratio_version(tx[loc_t], mask[loc_t], u, m, eps=eps[u, s, 0:2][:, loc_t])
            tx[loc_t, -1] = im[s, loc_t, -1]
            acc -= vpc.chaini_II_ratio_version(tx[loc_t], mask[loc_t], u, m, eps=eps[u, s, 2:4][:, loc_t])
        api = (acc / M).cpu().numpy()
        print(name, u, np.abs(got - g["R"][loc, u])[keep].max(), np.abs(api - g["R"][loc, u])[keep].max(), bound)
        assert np.abs(api - g["R"][loc, u])[keep].max() <= bound
    # the reference's signatures draw for themselves
    r = vpc.R_lindley_chain_ratio_version(0, x, mask, M, m, im, np.where(g["mask"][:, 0] == 0)[0])
    assert r.shape == (int((g["mask"][:, 0] == 0).sum()),) and torch.isfinite(r).all()
    assert vpc.chaini_I_ratio_version(x, mask, 1, m).shape == (x.shape[0],)
    assert vpc.chaini_II_ratio_version(x, mask, 1, m).shape == (x.shape[0],)


def test_wide_case_matches_oracle():
    """hid 500 (ragged tiles), d 128, n 32, M 4, a partly observed mask, injected draws, several chunks."""
    P, x, mask, im, eps = FC.big_case()
    c = FC.BIG
    m = FC.flow_model(fl, "reg", c["d"], c["hid"], P)
    R = vpc.flow_reward_matrix(m, _t(x), _t(mask), _t(im), eps=_t(eps), chunk=50).cpu().numpy()
    res = FR.reward_matrix(P, x, mask, im, eps)
    _check(R, res["R"], res, FC.big_delta(), "wide")


def test_chunk_run_and_seed_invariance():
    g, m = _golden_case("van", "flow_reward_van_d9.npz")
    x, mask, im, eps = _t(g["x"]), _t(g["mask"]), _t(g["im"]), _t(g["eps"])
    n, d = g["x"].shape
    M = int(g["M"])
    base = vpc.flow_reward_matrix(m, x, mask, im, eps=eps)
    for chunk in (1, 3, d - 1, 100):
        assert torch.equal(vpc.flow_reward_matrix(m, x, mask, im, eps=eps, chunk=chunk), base), chunk
    assert torch.equal(vpc.flow_reward_matrix(m, x, mask, im, eps=eps), base)
    drawn = vpc.flow_reward_draws(n, d, M, seed=77)
    assert drawn.shape == (d - 1, M, 4, n, 10)
    assert torch.equal(vpc.flow_reward_draws(n, d, M, seed=77), drawn)
    assert not torch.equal(vpc.flow_reward_draws(n, d, M, seed=78), drawn)
    by_eps = vpc.flow_reward_matrix(m, x, mask, im, eps=drawn)
    for chunk in (None, 1, 5):
        assert torch.equal(vpc.flow_reward_matrix(m, x, mask, im, seed=77, chunk=chunk), by_eps), chunk
    assert not torch.equal(vpc.flow_reward_matrix(m, x, mask, im, seed=78), by_eps)
    # the moment checks of the flow trainer's device draws (tests/test_flow_gpu.py)
    e = vpc.flow_reward_draws(64, 33, 5, seed=3)
    assert e.numel() > 400000
    assert abs(float(e.mean())) < 0.02 and abs(float(e.var()) - 1) < 0.03, (float(e.mean()), float(e.var()))
    assert abs(float((e.abs() <= 1).double().mean()) - 0.6827) < 0.01
    # a slab drawn with other candidates around it is the same slab
    assert torch.equal(vpc.flow_reward_draws(64, 33, 5, seed=3)[7], e[7])


def test_active_learning_flow_replays_reference(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    g = load_golden("flow_active_reg_d8.npz")
    n, d = g["x"].shape
    M, H = int(g["M"]), int(g["hid"])
    P = FC.params_of(g)
    m = FC.flow_model(fl, "reg", d, H, P)
    it = iter(g["fwd_xmean"])
    out = vpc.active_learning_flow(None, torch.from_numpy(g["x"]), torch.from_numpy(g["test_mask"]), 30, d, H, 10, M, 10,
                                   "toy", {"batch_size": 64, "patience": 100}, "exp", "reg_flow1", 100, 1, 1, alpha=1.0,
                                   p_missingness=30, reg_type="kl_reg", Repeat=1, model=m,
                                   _forward=lambda mask: torch.from_numpy(next(it).copy()),
                                   _reward_eps=lambda t: torch.from_numpy(g["reward_eps"][t]))
    assert next(it, None) is None
    R, act = out["R_hist_CHAI"][0].numpy(), out["action_CHAI"][0].numpy()
    delta = FC.golden_delta()
    mask = np.zeros((n, d))
    for t in range(d - 1):
        same = np.all(act[:, :t] == g["action"][:, :t], axis=1)  # rows whose mask history equals the reference's so far
        assert same.all() or same.mean() > 0.9
        res = FR.reward_matrix(P, g["x"], mask, g["im"][t], g["reward_eps"][t])
        res["edge"] = np.where(same[:, None], res["edge"], 0.0)   # rows off the reference's history are not compared
        _check(np.where(same[:, None], R[t], g["R_hist"][t]), g["R_hist"][t], res, delta, f"step {t}", cap=False)
        mask[np.arange(n), g["action"][:, t].astype(int)] += 1
    assert (act == g["action"]).mean() > 0.98
    assert np.array_equal(out["im_CHAI"][0].numpy(), g["im"])
    assert np.allclose(out["information_curve_CHAI"][0, 0].numpy(), g["info_curve"], rtol=1e-5, atol=1e-7)
    assert sorted(os.listdir(os.path.join("experiments", "exp", "toy", "rest", "reg_flow"))) == sorted(str(f) for f in g["files"])
    # reward_matrix dispatches flow models; the other entry still refuses them
    assert vpc.reward_matrix(m, _t(g["x"]), _t(mask * 0), _t(g["im"][0])).shape == (n, d - 1)
    with pytest.raises(NotImplementedError):
        vpc.active_learning_func(None, torch.from_numpy(g["x"]), torch.from_numpy(g["test_mask"]), 30, d, H, 10, M, 10, "toy",
                                 {}, "exp", "reg_flow1", 100, 1, 1, model=m, save=False)


def test_active_learning_flow_device_draws(tmp_path, monkeypatch):
    """The product path: forwards and reward draws on the device.  RNG-dependent, so properties only."""
    monkeypatch.chdir(tmp_path)
    g = load_golden("flow_active_reg_d8.npz")
    n, d = g["x"].shape
    m = FC.flow_model(fl, "reg", d, int(g["hid"]), FC.params_of(g))
    out = vpc.active_learning_flow(None, torch.from_numpy(g["x"]), torch.from_numpy(g["test_mask"]), 30, d, int(g["hid"]), 10,
                                   4, 10, "toy", {}, "exp", "reg_flow1", 100, 1, 1, Repeat=1, model=m, save=False, seed=5)
    for row in out["action_CHAI"][0].numpy():
        assert sorted(row.astype(int)) == list(range(d - 1))
    assert torch.isfinite(out["information_curve_CHAI"]).all()


def test_guards():
    g, m = _golden_case("van", "flow_reward_van_d9.npz")
    x, mask, im, eps = (torch.from_numpy(g[k]) for k in ("x", "mask", "im", "eps"))
    with pytest.raises(vpc.VpcError):
        vpc.flow_reward_matrix(m, x, mask, im)                                   # CPU tensors
    with pytest.raises(vpc.VpcError):
        vpc.flow_reward_matrix(m, x.cuda(), mask.cuda(), im.cuda(), eps=eps.cuda()[:, :, :2])   # wrong eps shape
    with pytest.raises(vpc.VpcError):
        vpc.flow_reward_matrix(m, x.cuda(), mask.cuda(), im.cuda(), chunk=0)
    big = fl.VAEFlow(x.shape[1], 520, 10, 10, {"batch_size": 64, "patience": 100}).cuda()
    with pytest.raises(vpc.VpcError):
        vpc.flow_reward_matrix(big, x.cuda(), mask.cuda(), im.cuda())           # hid > 512
