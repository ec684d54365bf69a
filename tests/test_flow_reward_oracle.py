"""CPU checks of the flow models' config 5 reward: the float64 restatement (tests/flow_reward_oracle.py) against the
values recorded from the reference's R_lindley_chain_ratio_version and active_learning_func
(tests/golden/make_golden_flow_reward.py), and the argument checks of the C entry points, which return before any launch.
"""
import ctypes as C

import numpy as np
import pytest

import flow_reward_cases as FC
import flow_reward_oracle as FR
import vpc_amd as vpc
from conftest import load_golden


@pytest.mark.parametrize("kind,name", FC.GOLDEN, ids=FC.IDS)
def test_oracle_matches_reference(kind, name):
    g = load_golden(name)
    res = FR.reward_matrix(FC.params_of(g), g["x"], g["mask"], g["im"], g["eps"])
    err, bound, share = FR.compare(res["R"], g["R"], res["edge"], res["S"], float(g["delta"]))
    print(name, "err", err, "bound", bound, "flagged", share, "S", res["S"])
    assert np.array_equal(res["R"] == -1e4, g["R"] == -1e4)
    assert share <= FR.MAX_FLAGGED
    assert err <= bound


def test_golden_masks_cover_the_quirks():
    g = load_golden("flow_reward_reg_d12.npz")
    mask = g["mask"]
    assert (mask[:, -1] != 0).sum() == 2                      # rows that see the carried-over target
    assert any((mask[:, u] != 0).all() for u in range(mask.shape[1] - 1))   # a candidate with empty loc
    assert 0 < (mask[:, :-1] != 0).mean() < 1
    q = load_golden("flow_reward_quirk_reg.npz")
    u, m, c = (int(v) for v in q["quirk_group"])
    loc = q["mask"][:, u] == 0
    grp = q["eps"][u, m, c]
    assert loc.any() and np.all(np.abs(grp[loc]) > 1) and np.all(np.abs(grp[~loc]) <= 1)
    assert sum(int(np.all(np.abs(q["eps"][uu, mm, cc][q["mask"][:, uu] == 0]) > 1))
               for uu in range(q["eps"].shape[0]) for mm in range(q["eps"].shape[1]) for cc in range(4)
               if (q["mask"][:, uu] == 0).any()) == 1


def test_carry_over_changes_the_target_rows():
    """Dropping the carry-over (calls Ia / Ib always seeing x[:, T]) moves exactly the rows with the target observed."""
    g = load_golden("flow_reward_reg_d12.npz")
    P = FC.params_of(g)
    res = FR.reward_matrix(P, g["x"], g["mask"], g["im"], g["eps"])
    im2 = g["im"].copy()
    im2[:-1, :, -1] = g["x"][None, :, -1]   # sample m >= 1 would carry im[m - 1, :, T]: make that equal to x[:, T]
    mk = g["mask"].copy()
    res2 = FR.reward_matrix(P, g["x"], mk, im2, g["eps"])
    rows = np.where(g["mask"][:, -1] != 0)[0]
    moved = np.where(np.any(np.abs(res["R"] - res2["R"]) > 1e-9, axis=1))[0]
    assert set(rows) <= set(moved)


def test_active_golden_rewards_replay():
    """Every step of the reference's active_learning_func on reg_flow1: the oracle with the recorded imputations and
    reward draws reproduces R_hist; the recorded actions are its argmax."""
    g = load_golden("flow_active_reg_d8.npz")
    P = FC.params_of(g)
    n, d = g["x"].shape
    mask = np.zeros((n, d))
    delta = FC.golden_delta()
    for t in range(d - 1):
        res = FR.reward_matrix(P, g["x"], mask, g["im"][t], g["reward_eps"][t])
        err, bound, share = FR.compare(res["R"], g["R_hist"][t], res["edge"], res["S"], delta)
        print("step", t, "err", err, "bound", bound, "flagged", share)
        assert np.array_equal(res["R"] == -1e4, g["R_hist"][t] == -1e4)
        assert err <= bound
        assert np.array_equal(g["R_hist"][t].argmax(1), g["action"][:, t].astype(int))
        mask[np.arange(n), g["action"][:, t].astype(int)] += 1


def test_big_case_flagged_share_within_cap():
    """The inputs of the hid 500 / d 128 GPU test: the oracle alone flags at most 5 % of the unobserved entries."""
    P, x, mask, im, eps = FC.big_case()
    res = FR.reward_matrix(P, x, mask, im, eps)
    unobs = res["R"] != -1e4
    share = float((unobs & (res["edge"] <= FC.big_delta())).sum()) / unobs.sum()
    print("flagged", share, "S", res["S"])
    assert share <= FR.MAX_FLAGGED


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = vpc._lib.lib()
    size = C.c_long(0)
    assert lib.vpc_flow_reward_scratch(8, 6, 64, 2, 3, C.byref(size)) == 0 and size.value > 0
    small = size.value
    assert lib.vpc_flow_reward_scratch(8, 6, 64, 2, 5, C.byref(size)) == 0 and size.value > small
    for bad in [(8, 1, 64, 2, 1), (8, 6, 513, 2, 1), (8, 6, 64, 0, 1), (8, 6, 64, 2, 0), (0, 6, 64, 2, 1)]:
        assert lib.vpc_flow_reward_scratch(*bad, C.byref(size)) != 0, bad
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    mis = C.c_void_p(p.value + 4)
    args = lambda scratch, n_s, d, hid, M: (p, p, p, p, p, p, p, p, p, None, 0, scratch, n_s, p, 8, d, hid, M, 1, None)
    assert lib.vpc_flow_reward_matrix(*args(p, 1 << 40, 1, 64, 2)) != 0      # d < 2
    assert lib.vpc_flow_reward_matrix(*args(p, 1 << 40, 6, 513, 2)) != 0    # hid > 512
    assert lib.vpc_flow_reward_matrix(*args(p, 1 << 40, 6, 64, 0)) != 0     # M < 1
    assert lib.vpc_flow_reward_matrix(*args(mis, 1 << 40, 6, 64, 2)) != 0   # misaligned scratch
    assert lib.vpc_flow_reward_matrix(*args(p, 16, 6, 64, 2)) != 0          # scratch too small
    assert lib.vpc_flow_reward_draws(None, 8, 6, 2, 0, None) != 0
