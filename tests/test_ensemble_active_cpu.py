"""The host side of the ensemble acquisition loop (ensemble.EnsembleAcquirer, active.active_sweep): active_sweep's split of a
mixed list of runs, the draw offsets of a run, validation before any device call, the C entries' argument checks, and the input
guard of the GPU loop test.  CPU only: nothing is launched (the acquirer and active_learning_func are stubbed where
active_sweep would reach them; the C entries return before their first launch)."""
import ctypes

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from ensemble_active_cases import L, LOOP, Port64, history_match, loop_data, loop_eps, oracle_loop, train_on_cpu
from oracle import vae_oracle as O
from vpc_amd import active as A
from vpc_amd import ensemble as E
from vpc_amd.fused import LP
from vpc_amd.trainer import eval_draw_counters

TP = {"batch_size": 8, "patience": 1}


def _cpu(cls, d=14, reg_type="kl_reg"):
    return cls(d, 500, 10, L, TP, "e", reg_type) if issubclass(cls, vpc.Reg_VAE) else cls(d, 500, 10, L, TP, "e")


# ----------------------------------------------------------------------------------------------- active_sweep's grouping
def test_active_sweep_routes_members(monkeypatch):
    ms = [_cpu(vpc.Reg_VAE), _cpu(vpc.vanilla_VAE), _cpu(vpc.Reg_VAE), _cpu(vpc.Reg_VAE_mask), _cpu(vpc.Reg_EDDI)]
    cfgs = [dict(vae_type="reg_vae1", alpha=0.5, seed=11), dict(vae_type="vanilla_vae1", seed=12),
            dict(vae_type="reg_vae2", alpha=0.5, p_missingness=50, seed=13), dict(vae_type="reg_vae1_mask_augm", seed=14),
            dict(vae_type="reg_EDDI1", seed=15)]
    n, d, M, rep = 21, 14, 3, 2
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(0))
    calls = {"ens": [], "alone": []}

    class StubAcquirer:
        def __init__(self, models, seeds=None):
            self.models, self.seeds = list(models), list(seeds)

        def run(self, x, M, *, repeats=1, max_steps=None):
            calls["ens"].append((self.models, self.seeds, tuple(x.shape), M, repeats, max_steps))
            G = len(self.models)
            tag = torch.tensor(self.seeds, dtype=torch.float32)
            return (tag[:, None, None] + torch.arange(d, dtype=torch.float32).expand(G, repeats, d),
                    torch.arange(d - 1, dtype=torch.int32).expand(G, repeats, n, d - 1).contiguous(),
                    tag[:, None, None, None, None] * torch.ones(G, repeats, d - 1, n, d - 1),
                    tag[:, None, None, None, None, None] * torch.ones(G, repeats, d - 1, M, n, d))

    def stub_alone(*a, model=None, save=True, max_steps=None, **kw):
        calls["alone"].append((model, a[12], a[17], a[19], a[24], save, max_steps))  # vae_type, alpha, p_missingness, Repeat
        return "alone"

    monkeypatch.setattr(A, "EnsembleAcquirer", StubAcquirer)
    monkeypatch.setattr(A, "active_learning_func", stub_alone)
    out = A.active_sweep(None, cfgs, x, torch.ones(n, d, dtype=torch.bool), 30, d, 500, 10, M, L, "uci", TP, "e", 7, 1, 1,
                         device="cpu", Repeat=rep, models=ms, save=False, max_steps=5)
    # the mask-augmented and the EDDI member went through active_learning_func alone, each with its own config
    assert [c[0] for c in calls["alone"]] == [ms[3], ms[4]]
    assert calls["alone"][0][1:] == ("reg_vae1_mask_augm", 1.0, 30, rep, False, 5)
    assert calls["alone"][1][1:] == ("reg_EDDI1", 1.0, 30, rep, False, 5)
    assert out[3] == "alone" and out[4] == "alone"
    # the two Reg_VAE share one acquirer, the vanilla_VAE has its own: one run per group
    by_models = {tuple(id(m) for m in c[0]): c for c in calls["ens"]}
    assert len(calls["ens"]) == 2 and set(by_models) == {(id(ms[0]), id(ms[2])), (id(ms[1]),)}
    assert by_models[(id(ms[0]), id(ms[2]))][1:] == ([11, 13], (n, d), M, rep, 5)
    assert by_models[(id(ms[1]),)][1:] == ([12], (n, d), M, rep, 5)
    # outputs in config order, with the reference's shapes; the scalar curve broadcast over the rows; the action as float
    for g, seed in ((0, 11), (1, 12), (2, 13)):
        r = out[g]
        assert set(r) == {"information_curve_CHAI", "action_CHAI", "R_hist_CHAI", "im_CHAI"}
        assert tuple(r["information_curve_CHAI"].shape) == (rep, n, d)
        assert tuple(r["action_CHAI"].shape) == (rep, n, d - 1) and r["action_CHAI"].dtype == torch.float32
        assert tuple(r["R_hist_CHAI"].shape) == (rep, d - 1, n, d - 1)
        assert tuple(r["im_CHAI"].shape) == (rep, d - 1, M, n, d)
        assert torch.equal(r["information_curve_CHAI"], (seed + torch.arange(d, dtype=torch.float32)).expand(rep, n, d))
        assert torch.equal(r["action_CHAI"][1, 5], torch.arange(d - 1, dtype=torch.float32))
        assert torch.all(r["R_hist_CHAI"] == seed) and torch.all(r["im_CHAI"] == seed)


def test_active_sweep_checks_list_lengths():
    with pytest.raises(vpc.VpcError, match="models"):
        A.active_sweep(None, [dict(vae_type="reg_vae1")], torch.zeros(2, 14), torch.ones(2, 14), 30, 14, 500, 10, 1, L, "uci",
                       TP, "e", 1, 1, 1, models=[])


def test_exports():
    assert vpc.EnsembleAcquirer is E.EnsembleAcquirer and vpc.active_sweep is A.active_sweep
    assert "EnsembleAcquirer" in vpc.__all__ and "active_sweep" in vpc.__all__


# ----------------------------------------------------------------------------------------------- draw offsets
@pytest.mark.parametrize("d,max_steps,repeats", [(14, None, 1), (14, 3, 2), (14, 0, 1), (14, 99, 1)])
def test_draw_offsets_of_a_run(d, max_steps, repeats):
    n, M, G = 21, 3, 2
    n_, steps, calls, R = E.acquire_plan(G, d, L, (n, d), M, repeats, max_steps)
    assert (n_, R) == (n, M * n)
    assert steps == (d - 1 if max_steps is None else min(max_steps, d - 1))  # max_steps shortens the sequence
    assert calls == repeats * (1 + 2 * steps)
    offs, after = E.acquire_draw_offsets(40, R, steps, repeats)
    assert len(offs) == calls
    cur = 40
    for o in offs:  # successive eval_draw_counters(., M n): no counter rule of its own
        want, cur = eval_draw_counters(cur, R, LP)
        assert o == want
    assert after == cur == 40 + calls * 4 * R


# ----------------------------------------------------------------------------------------------- validation
def test_members_are_validated_before_any_device_call():
    for models, exc in (([_cpu(vpc.Reg_VAE), _cpu(vpc.vanilla_VAE)], TypeError),       # mixed classes
                        ([_cpu(vpc.vanilla_VAE, 200)] * 2, vpc.VpcError),              # a wide member
                        ([_cpu(vpc.Reg_VAE), _cpu(vpc.Reg_VAE_mask)], (TypeError, vpc.VpcError)),
                        ([], vpc.VpcError)):
        with pytest.raises(exc) as ei:  # (CPU models: a device call would raise "... got a CPU tensor" instead)
            E.EnsembleAcquirer(models)
        assert "CPU tensor" not in str(ei.value)


def test_run_shapes_are_validated_on_the_host():
    G, d, n, M = 3, 14, 21, 3
    ok = E.acquire_plan(G, d, L, (G, n, d), M, 2, 4, (G, 18, M * n, L))
    assert ok == (n, 4, 18, M * n)
    assert E.acquire_plan(G, d, L, (n, d), M, 1, None, (27, M * n, L))[2] == 27
    for x_shape in ((n, 13), (n, 16), (G + 1, n, d), (d,), (1, G, n, d)):  # an x of the wrong width / member count / rank
        with pytest.raises(vpc.VpcError, match="x:"):
            E.acquire_plan(G, d, L, x_shape, M)
    for eps_shape in ((26, M * n, L), (28, M * n, L), (27, M * n, L + 1), (27, n, L), (G + 1, 27, M * n, L)):
        with pytest.raises(vpc.VpcError, match="eps"):  # an eps of the wrong call count (or rows, or width)
            E.acquire_plan(G, d, L, (n, d), M, 1, None, eps_shape)
    with pytest.raises(vpc.VpcError, match="eps"):
        E.acquire_plan(G, d, L, (n, d), M, 1, 3, (27, M * n, L))  # max_steps = 3: 7 calls
    for kw in (dict(M=0), dict(repeats=0), dict(max_steps=-1)):
        with pytest.raises(vpc.VpcError):
            E.acquire_plan(G, d, L, (n, d), **{"M": M, **kw})


def test_member_chunk_under_a_workspace_budget():
    sizes = (9 * 2 ** 18, 2 ** 18, 2 ** 12)
    per = sum(sizes)
    assert E.reward_member_chunk(64, 160, 12, 50, 64 << 20, sizes) == min(64, (64 << 20) // per)
    assert E.reward_member_chunk(3, 21, 14, 3, 2 * per, sizes) == 2   # two members fit: chunks of 2 + 1
    assert E.reward_member_chunk(3, 21, 14, 3, 1, sizes) == 1         # never less than one member
    assert E.reward_member_chunk(3, 21, 14, 3, 100 * per, sizes) == 3


# ----------------------------------------------------------------------------------------------- the C entries
def test_c_entries_refuse_bad_arguments_before_launching():
    l = vpc._lib.lib()
    host = (ctypes.c_float * 64)()
    base = ctypes.addressof(host)
    p = ctypes.c_void_p((base + 15) // 16 * 16)            # 16-byte aligned
    odd = ctypes.c_void_p((base + 15) // 16 * 16 + 4)       # 4-byte aligned only
    S9 = lambda *v: (ctypes.c_long * 9)(*v)
    ms = S9(0, 0, 0, 0, 64, 0, 0, 0, 0)
    ARG, SHAPE = 1, 2

    def impute(x=p, mask=p, eps=p, enc=p, dec=p, mem=p, G=1, tiles=p, nt=1, N=16, R=16, draw=0, mode=0, out=p, so=16 * 16,
               strides=ms, d=16, dr=14, Ld=10, mb=0):
        return l.vpc_impute_small_multi_f32(x, mask, eps, enc, dec, mem, G, tiles, nt, N, R, draw, 0, -3.9, mode, out, so,
                                            strides, d, dr, Ld, mb, None)

    for kw in (dict(x=None), dict(mask=None), dict(enc=None), dict(dec=None), dict(mem=None), dict(tiles=None), dict(out=None),
               dict(strides=None), dict(eps=None), dict(mode=2), dict(mode=-1), dict(G=0), dict(nt=0), dict(R=0), dict(mb=-1),
               dict(dr=20), dict(dr=0), dict(x=odd), dict(enc=odd), dict(dec=odd), dict(eps=odd), dict(so=16 * 14 - 1),
               dict(mode=1, so=15), dict(strides=S9(0, 0, 0, 0, 0, 0, 0, 0, 0)), dict(strides=S9(8, 0, 0, 0, 64, 0, 0, 0, 0))):
        assert impute(**kw) == ARG, kw
    for kw in (dict(d=132, dr=130), dict(d=14), dict(Ld=16), dict(Ld=0)):
        assert impute(**kw) == SHAPE, kw
    # (the evaluation entry kept its checks)
    assert l.vpc_eval_small_multi_f32(p, p, p, p, p, p, 1, p, 1, 16, 16, 0, 0, -3.9, None, ms, 16, 14, 10, 0, None) == ARG
    assert l.vpc_eval_small_multi_f32(p, p, p, p, p, p, 1, p, 1, 16, 16, 0, 0, -3.9, p, ms, 132, 130, 10, 0, None) == SHAPE

    assert l.vpc_target_mse_multi(None, 63, 63, 3, p, 1, None) == ARG
    assert l.vpc_target_mse_multi(p, 63, 63, 3, None, 1, None) == ARG
    assert l.vpc_target_mse_multi(p, 62, 63, 3, p, 1, None) == ARG   # a member's slice outside its stride
    assert l.vpc_target_mse_multi(p, 63, 0, 3, p, 1, None) == ARG
    assert l.vpc_target_mse_multi(p, 63, 63, 0, p, 1, None) == ARG

    n, d, M = 5, 14, 3
    sz = [ctypes.c_long() for _ in range(3)]
    assert l.vpc_reward_scratch_multi(n, d, M, *[ctypes.byref(s) for s in sz]) == 0
    pre, stat, w1t = [s.value for s in sz]
    assert pre == n * 16 * 224 and stat == n * 16 * 64 and w1t % 4 == 0 and w1t >= d * 112 + n * d + 4
    assert l.vpc_reward_scratch_multi(n, 129, M, None, None, None) == ARG and l.vpc_reward_scratch_multi(0, d, M, None, None, None) == ARG
    good = [0, n * d, M * n * d, 2048, 4096, pre, stat, w1t, n * (d - 1)]

    def reward(x=p, mask=p, im=p, W1=p, b1=p, img=p, pre_=p, stat_=p, w1t_=p, R=p, G=3, chunk=2, strides=S9(*good), n_=n, d_=d,
               Ld=10, M_=M):
        return l.vpc_reward_matrix_multi(x, mask, im, W1, b1, img, pre_, stat_, w1t_, R, G, chunk, strides, n_, d_, Ld, M_, None)

    bad = lambda i, v: S9(*[v if k == i else s for k, s in enumerate(good)])
    for kw in (dict(x=None), dict(mask=None), dict(im=None), dict(W1=None), dict(b1=None), dict(img=None), dict(pre_=None),
               dict(stat_=None), dict(w1t_=None), dict(R=None), dict(strides=None), dict(G=0), dict(chunk=0), dict(n_=0), dict(M_=0),
               dict(pre_=odd), dict(stat_=odd), dict(w1t_=odd), dict(img=odd),            # misaligned workspaces / image
               dict(strides=bad(0, n * d - 1)), dict(strides=bad(1, 0)), dict(strides=bad(2, M * n * d - 1)),
               dict(strides=bad(3, 100 * d)), dict(strides=bad(4, 0)), dict(strides=bad(4, 4098)), dict(strides=bad(5, pre - 4)),
               dict(strides=bad(5, pre + 2)), dict(strides=bad(6, stat - 4)), dict(strides=bad(7, w1t - 4)),
               dict(strides=bad(8, n * (d - 1) - 1))):
        assert reward(**kw) == ARG, kw
    for kw in (dict(d_=129), dict(d_=1), dict(Ld=16), dict(Ld=0)):
        assert reward(**kw) == SHAPE, kw

    def acquire(R=p, Rs=n * (d - 1), mask=p, msk_s=n * d, pitch=d, mask2=None, m2s=0, p2=0, act=p, acs=n * (d - 1), ap=d - 1, G=3,
                n_=n, d_=d):
        return l.vpc_acquire_multi(R, Rs, mask, msk_s, pitch, mask2, m2s, p2, act, acs, ap, G, n_, d_, None)

    for kw in (dict(R=None), dict(mask=None), dict(act=None), dict(G=0), dict(n_=0), dict(Rs=n * (d - 1) - 1), dict(pitch=d - 1),
               dict(msk_s=n * d - 1), dict(ap=0), dict(acs=(n - 1) * (d - 1)), dict(mask2=p, m2s=n * 16, p2=d - 1),
               dict(mask2=p, m2s=n * 16 - 1, p2=16)):
        assert acquire(**kw) == ARG, kw
    for kw in (dict(d_=129), dict(d_=1)):
        assert acquire(**kw) == SHAPE, kw


# ----------------------------------------------------------------------------------------------- the GPU loop test's input guard
def test_loop_case_is_decided_by_its_inputs_not_by_rounding():
    """The cap of tests/test_ensemble_active_gpu.py::test_loop_vs_oracle, on the reference side alone: the oracle's loop in
    float32 and in float64 arithmetic, on that test's data and eps stream and a model trained by its recipe, agree on the action
    history of at least 90 % of the rows at every compared step.  (A case whose argmax is decided by round-off would make the
    GPU comparison a coin toss.)"""
    d, n, M, steps = LOOP["d"], LOOP["n"], LOOP["M"], LOOP["steps"]
    x, xt, mt = loop_data()
    params = train_on_cpu(O.init_params(d, L, seed=3), xt, mt)
    eps = loop_eps(1)[0]
    a32 = oracle_loop(O.TorchPort(params, L), x, eps, M, steps)
    a64 = oracle_loop(Port64(params, L), x, eps, M, steps)
    live = a32["R_hist"] != -1e4
    scale = float(a32["R_hist"][live].abs().max())
    same = history_match(a32["action"].numpy(), a64["action"].numpy())
    print("rows with the same history per step:", same.mean(1).tolist(), "reward scale", scale)
    assert scale > 1e-3  # the trained encoder does discriminate between candidates
    assert np.all(same.mean(1) >= 0.9)
