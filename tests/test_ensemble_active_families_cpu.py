"""The host side of the acquisition loop of the mask-augmented and point-net sweeps (ensemble.MaskEnsembleAcquirer,
ensemble.EDDIEnsembleAcquirer, active.active_sweep): active_sweep's split of a mixed list of runs, validation before any device
call, the new C entries' argument checks, and the input guard of the GPU loop test.  CPU only: nothing is launched (the acquirers
and active_learning_func are stubbed where active_sweep would reach them; the C entries return before their first launch)."""
import ctypes

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from ensemble_active_cases import history_match, oracle_loop
from ensemble_active_family_cases import LOOP, LOOP_CASES, init_params, loop_data, loop_eps, port, port64, train_on_cpu
from family_eval_cases import L, TP, build
from vpc_amd import active as A
from vpc_amd import ensemble as E

ACQ = {"mask": "MaskEnsembleAcquirer", "eddi": "EDDIEnsembleAcquirer"}  # (by name: without them the routing test says what is missing)


# ----------------------------------------------------------------------------------------------- 1. active_sweep's grouping
def test_active_sweep_routes_family_groups(monkeypatch):
    d, n, M, rep = 14, 21, 3, 2
    ms = [build("mask", "reg", d), build("eddi", "reg", d), vpc.Reg_VAE(d, 500, 10, L, TP, "e", "kl_reg"), build("eddi", "van", d),
          build("mask", "reg", d), build("eddi", "reg", d), vpc.Reg_VAE(d, 500, 10, L, TP, "e", "kl_reg")]
    cfgs = [dict(vae_type="reg_vae1_mask_augm", alpha=0.5, seed=11), dict(vae_type="reg_EDDI1", alpha=0.5, seed=12),
            dict(vae_type="reg_vae1", seed=13), dict(vae_type="vanilla_EDDI1", seed=14),
            dict(vae_type="reg_vae2_mask_augm", alpha=0.8, p_missingness=50, seed=15), dict(vae_type="reg_EDDI2", seed=16),
            dict(vae_type="reg_vae2", alpha=0.8, seed=17)]
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(0))
    calls = {"plain": [], "mask": [], "eddi": [], "alone": []}

    def stub(name):
        class StubAcquirer:
            def __init__(self, models, seeds=None):
                self.models, self.seeds = list(models), list(seeds)

            def run(self, x, M, *, repeats=1, max_steps=None):
                calls[name].append((self.models, self.seeds, tuple(x.shape), M, repeats, max_steps))
                G = len(self.models)
                tag = torch.tensor(self.seeds, dtype=torch.float32)
                return (tag[:, None, None] + torch.arange(d, dtype=torch.float32).expand(G, repeats, d),
                        torch.arange(d - 1, dtype=torch.int32).expand(G, repeats, n, d - 1).contiguous(),
                        tag[:, None, None, None, None] * torch.ones(G, repeats, d - 1, n, d - 1),
                        tag[:, None, None, None, None, None] * torch.ones(G, repeats, d - 1, M, n, d))
        return StubAcquirer

    def stub_alone(*a, model=None, save=True, max_steps=None, **kw):
        calls["alone"].append((model, a[12], a[17], a[19], a[24], save, max_steps))  # vae_type, alpha, p_missingness, Repeat
        return "alone"

    monkeypatch.setattr(A, "EnsembleAcquirer", stub("plain"))
    monkeypatch.setattr(A, "MaskEnsembleAcquirer", stub("mask"), raising=False)
    monkeypatch.setattr(A, "EDDIEnsembleAcquirer", stub("eddi"), raising=False)
    monkeypatch.setattr(A, "active_learning_func", stub_alone)
    out = A.active_sweep(None, cfgs, x, torch.ones(n, d, dtype=torch.bool), 30, d, 500, 10, M, L, "uci", TP, "e", 7, 1, 1,
                         device="cpu", Repeat=rep, models=ms, save=False, max_steps=5)
    # one run per family group of two, with the configs' seeds; the lone vanilla_EDDI through active_learning_func
    for name, idx in (("mask", (0, 4)), ("eddi", (1, 5)), ("plain", (2, 6))):
        assert len(calls[name]) == 1, name
        models, seeds, *rest = calls[name][0]
        assert [id(m) for m in models] == [id(ms[g]) for g in idx] and seeds == [cfgs[g]["seed"] for g in idx], name
        assert rest == [(n, d), M, rep, 5], name
    assert calls["alone"] == [(ms[3], "vanilla_EDDI1", 1.0, 30, rep, False, 5)] and out[3] == "alone"
    # outputs in config order, with the reference's shapes; the scalar curve broadcast over the rows; the action as float
    for g, c in enumerate(cfgs):
        if g == 3:
            continue
        r, seed = out[g], c["seed"]
        assert set(r) == {"information_curve_CHAI", "action_CHAI", "R_hist_CHAI", "im_CHAI"}
        assert tuple(r["action_CHAI"].shape) == (rep, n, d - 1) and r["action_CHAI"].dtype == torch.float32
        assert tuple(r["R_hist_CHAI"].shape) == (rep, d - 1, n, d - 1) and tuple(r["im_CHAI"].shape) == (rep, d - 1, M, n, d)
        assert torch.equal(r["information_curve_CHAI"], (seed + torch.arange(d, dtype=torch.float32)).expand(rep, n, d))
        assert torch.all(r["R_hist_CHAI"] == seed) and torch.all(r["im_CHAI"] == seed)


# ----------------------------------------------------------------------------------------------- 2. validation
def test_members_are_validated_before_any_device_call():
    plain = vpc.Reg_VAE(14, 500, 10, L, TP, "e", "kl_reg")
    wide_emb = build("eddi", "reg", 14)
    wide_emb.emb_dim = 33  # (the model class itself refuses K > 32; the acquirer's own check is what is under test)
    cases = [("mask", [build("mask", "reg", 14), build("mask", "van", 14)], TypeError),          # mixed classes
             ("eddi", [build("eddi", "reg", 14), build("eddi", "van", 14)], TypeError),
             ("mask", [build("mask", "reg", 14), plain], TypeError),                                # a plain member
             ("eddi", [build("eddi", "reg", 14), plain], TypeError),
             ("mask", [build("eddi", "reg", 14)] * 2, TypeError),                                   # the other family's member
             ("eddi", [build("mask", "reg", 14)] * 2, TypeError),
             ("mask", [build("mask", "reg", 65)] * 2, vpc.VpcError),                                # 2 d > 128
             ("eddi", [build("eddi", "reg", 65)] * 2, vpc.VpcError),                                # d > 64
             ("eddi", [wide_emb] * 2, vpc.VpcError),                                                # K > 32
             ("mask", [build("mask", "reg", 14), build("mask", "reg", 20)], vpc.VpcError),          # two shapes
             ("eddi", [build("eddi", "reg", 14, K=10), build("eddi", "reg", 14, K=20)], vpc.VpcError),
             ("mask", [], vpc.VpcError)]
    for family, models, exc in cases:
        with pytest.raises(exc) as ei:  # (CPU models: a device call would raise "... got a CPU tensor" instead)
            getattr(E, ACQ[family])(models)
        assert "CPU tensor" not in str(ei.value), (family, ei.value)
    for family in ACQ:
        with pytest.raises(vpc.VpcError, match="single-process") as ei:
            getattr(E, ACQ[family])([build(family, "reg", 14)] * 2, world_size=2)
        assert "CPU tensor" not in str(ei.value)


def test_for_trainer_takes_its_own_family():
    class FakeTrainer:
        family = E.EDDI
    with pytest.raises(TypeError, match="own family"):
        E.MaskEnsembleAcquirer.for_trainer(FakeTrainer())
    FakeTrainer.family = E.MASK
    with pytest.raises(TypeError, match="own family"):
        E.EDDIEnsembleAcquirer.for_trainer(FakeTrainer())
    with pytest.raises(TypeError, match="own family"):
        E.EDDIEnsembleAcquirer.for_trainer(object())


def test_exports_and_the_trainers_pointer():
    assert vpc.MaskEnsembleAcquirer is E.MaskEnsembleAcquirer and vpc.EDDIEnsembleAcquirer is E.EDDIEnsembleAcquirer
    assert {"MaskEnsembleAcquirer", "EDDIEnsembleAcquirer"} <= set(vpc.__all__)
    for cls, ev in ((E.MaskEnsembleAcquirer, E.MaskEnsembleEvaluator), (E.EDDIEnsembleAcquirer, E.EDDIEnsembleEvaluator)):
        assert issubclass(cls, E.EnsembleAcquirer) and issubclass(cls, ev) and cls.family is ev.family
        # the loop, the draw rule and the launch accounting are stated once
        for name in ("run", "impute", "reward", "_setup", "_reward_workspaces"):
            assert getattr(cls, name) is getattr(E.EnsembleAcquirer, name), name
    with pytest.raises(vpc.VpcError, match="cover the plain") as ei:
        E._FamilyTrainer.evaluator(None)
    assert "MaskEnsembleAcquirer" in str(ei.value) and "EDDIEnsembleAcquirer" in str(ei.value)


# ----------------------------------------------------------------------------------------------- 3. the C entries
def test_new_c_entries_refuse_bad_arguments_before_launching():
    l = vpc._lib.lib()
    host = (ctypes.c_float * 64)()
    base = ctypes.addressof(host)
    p = ctypes.c_void_p((base + 15) // 16 * 16)            # 16-byte aligned
    odd = ctypes.c_void_p((base + 15) // 16 * 16 + 4)       # 4-byte aligned only
    odd1 = ctypes.c_void_p((base + 15) // 16 * 16 + 1)
    S = lambda *v: (ctypes.c_long * len(v))(*v)
    ARG, SHAPE = 1, 2
    ms = S(0, 0, 0, 0, 64, 0, 0, 0, 4096)  # VPC_MS_*: x, mask shared; MS_IMG 64; MS_PARAM (the front-ends) 4096

    def impute_aug(x=p, mask=p, eps=p, enc=p, dec=p, mem=p, G=1, tiles=p, nt=1, N=16, R=16, draw=0, mode=0, out=p, so=16 * 14,
                   strides=ms, d=16, dr=14, Ld=10, mb=0):
        return l.vpc_impute_small_multi_aug_f32(x, mask, eps, enc, dec, mem, G, tiles, nt, N, R, draw, 0, -3.9, mode, out, so,
                                                strides, d, dr, Ld, mb, None)

    def impute_eddi(x=p, mask=p, eps=p, enc=p, dec=p, mem=p, G=1, tiles=p, nt=1, N=16, R=16, draw=0, mode=0, out=p, so=16 * 14,
                    strides=ms, d=16, dr=14, Ld=10, K=10, front=p, mb=0):
        return l.vpc_impute_small_multi_eddi_f32(x, mask, eps, enc, dec, mem, G, tiles, nt, N, R, draw, 0, -3.9, mode, out, so,
                                                 strides, d, dr, Ld, K, front, mb, None)

    common_arg = (dict(x=None), dict(mask=None), dict(enc=None), dict(dec=None), dict(mem=None), dict(tiles=None), dict(out=None),
                  dict(strides=None), dict(eps=None), dict(mode=2), dict(mode=-1), dict(G=0), dict(nt=0), dict(R=0), dict(mb=-1),
                  dict(x=odd), dict(enc=odd), dict(dec=odd), dict(eps=odd), dict(out=odd1), dict(so=16 * 14 - 1),
                  dict(mode=1, so=15), dict(strides=S(0, 0, 0, 0, 0, 0, 0, 0, 4096)),
                  dict(strides=S(8, 0, 0, 0, 64, 0, 0, 0, 4096)))     # a member's x outside its stride
    for fn in (impute_aug, impute_eddi):
        for kw in common_arg:
            assert fn(**kw) == ARG, (fn.__name__, kw)
        for kw in (dict(dr=20), dict(dr=0), dict(d=20, dr=14), dict(d=14), dict(Ld=16), dict(Ld=0)):
            assert fn(**kw) == SHAPE, (fn.__name__, kw)
    assert impute_aug(d=68, dr=65) == SHAPE                       # 2 d > 128
    assert impute_eddi(d=68, dr=65) == SHAPE                      # d > 64
    for kw in (dict(K=33), dict(K=0)):
        assert impute_eddi(**kw) == SHAPE, kw
    nfront = 14 * 10 + 14 + 10 * 12 + 10
    for kw in (dict(front=None), dict(front=odd1), dict(strides=S(0, 0, 0, 0, 64, 0, 0, 0, nfront - 1))):
        assert impute_eddi(**kw) == ARG, kw

    # ---- the fold
    def fold(front=p, fs=nfront, AC=p, acs=2 * 10 * 14, G=3, d=14, K=10):
        return l.vpc_eddi_fold_multi(front, fs, AC, acs, G, d, K, None)

    for kw in (dict(front=None), dict(AC=None), dict(front=odd1), dict(AC=odd1), dict(G=0), dict(fs=nfront - 1),
               dict(acs=2 * 10 * 14 - 1)):
        assert fold(**kw) == ARG, kw
    for kw in (dict(K=33, fs=1 << 20, acs=1 << 20), dict(K=0), dict(d=0), dict(d=129, fs=1 << 20, acs=1 << 20)):
        assert fold(**kw) == SHAPE, kw

    # ---- the reward with a member dimension and a kind
    MASK_KIND, PN_KIND = 1, 2
    n, d, M, K = 5, 14, 3, 10
    sz = [ctypes.c_long() for _ in range(3)]
    refs = [ctypes.byref(s) for s in sz]
    sizes = {}
    for kind, table in ((MASK_KIND, 2 * d * 112), (PN_KIND, 2 * 7 * 64 * 4)):
        assert l.vpc_reward_scratch_multi_ex(kind, n, d, M, K, *refs) == 0
        pre, stat, w1t = sizes[kind] = [s.value for s in sz]
        assert pre == n * 16 * 224 and stat == n * 16 * 64 and w1t % 4 == 0 and table + n * d + 4 <= w1t < table + n * d + 8
    assert l.vpc_reward_scratch_multi_ex(0, n, d, M, K, *refs) == ARG                   # the plain kind has its own entry
    assert l.vpc_reward_scratch_multi_ex(3, n, d, M, K, *refs) == ARG
    assert l.vpc_reward_scratch_multi_ex(MASK_KIND, 0, d, M, K, *refs) == ARG
    assert l.vpc_reward_scratch_multi_ex(MASK_KIND, n, 65, M, K, *refs) == SHAPE
    assert l.vpc_reward_scratch_multi_ex(PN_KIND, n, 65, M, K, *refs) == SHAPE
    assert l.vpc_reward_scratch_multi_ex(PN_KIND, n, d, M, 33, *refs) == SHAPE
    for kind, cols in ((MASK_KIND, 2 * d), (PN_KIND, K)):
        pre, stat, w1t = sizes[kind]
        good = [0, n * d, M * n * d, 100 * cols + 100, 10240, pre, stat, w1t, n * (d - 1), 2 * K * d]
        bad = lambda i, v: S(*[v if k == i else s for k, s in enumerate(good)])

        def reward(kind_=kind, x=p, mask=p, im=p, W1=p, b1=p, AC=p, K_=K, w23=p, pre_=p, stat_=p, w1t_=p, R=p, G=3, chunk=2,
                   strides=S(*good), n_=n, d_=d, Ld=10, M_=M):
            return l.vpc_reward_matrix_multi_ex(kind_, x, mask, im, W1, b1, AC, K_, w23, pre_, stat_, w1t_, R, G, chunk, strides,
                                                n_, d_, Ld, M_, None)

        for kw in (dict(x=None), dict(mask=None), dict(im=None), dict(W1=None), dict(b1=None), dict(w23=None), dict(pre_=None),
                   dict(stat_=None), dict(w1t_=None), dict(R=None), dict(strides=None), dict(G=0), dict(chunk=0), dict(n_=0),
                   dict(M_=0), dict(kind_=0), dict(kind_=3),
                   dict(pre_=odd), dict(stat_=odd), dict(w1t_=odd), dict(w23=odd),            # misaligned workspaces / image
                   dict(strides=bad(0, n * d - 1)), dict(strides=bad(1, 0)), dict(strides=bad(2, M * n * d - 1)),
                   dict(strides=bad(3, 100 * cols + 99)), dict(strides=bad(4, 0)), dict(strides=bad(4, 10242)),
                   dict(strides=bad(4, 10236)), dict(strides=bad(5, pre - 4)), dict(strides=bad(5, pre + 2)),
                   dict(strides=bad(6, stat - 4)), dict(strides=bad(7, w1t - 4)), dict(strides=bad(8, n * (d - 1) - 1))):
            assert reward(**kw) == ARG, (kind, kw)
        for kw in (dict(d_=65), dict(d_=1), dict(Ld=16), dict(Ld=0)):
            assert reward(**kw) == SHAPE, (kind, kw)
        if kind == PN_KIND:
            for kw in (dict(AC=None), dict(AC=odd1), dict(strides=bad(9, 2 * K * d - 1))):
                assert reward(**kw) == ARG, kw
            for kw in (dict(K_=33), dict(K_=0)):
                assert reward(**kw) == SHAPE, kw

    # ---- vpc_reward_matrix_multi is untouched: it reads exactly nine strides (a 9-slot array, the plain members' limits)
    assert l.vpc_reward_scratch_multi(n, d, M, *refs) == 0
    pre, stat, w1t = [s.value for s in sz]
    nine = [0, n * d, M * n * d, 2048, 4096, pre, stat, w1t, n * (d - 1)]

    def plain(strides, d_=d, w1t_=p):
        return l.vpc_reward_matrix_multi(p, p, p, p, p, p, p, p, w1t_, p, 3, 2, strides, n, d_, 10, M, None)

    # its limits are the plain members' (d <= 128, not the families'), and its ninth slot is the last one it has to be given: each
    # of the nine is checked, the new tenth is not asked for
    assert plain(S(*nine), d_=129) == SHAPE and plain(S(*nine), w1t_=odd) == ARG
    for k in range(1, 9):
        assert plain(S(*[0 if i == k else s for i, s in enumerate(nine)])) == ARG, k


# ----------------------------------------------------------------------------------------------- 4. the GPU loop test's input guard
@pytest.mark.parametrize("family,d,K", LOOP_CASES)
def test_loop_case_is_decided_by_its_inputs_not_by_rounding(family, d, K):
    """The cap of tests/test_ensemble_active_families_gpu.py::test_loop_vs_oracle, on the reference side alone: the oracle's loop
    in float32 and in float64 arithmetic, on that test's data and eps stream and a model trained by its recipe, agree on the
    action history of at least 90 % of the rows at every compared step."""
    n, M, steps = LOOP["n"], LOOP["M"], LOOP["steps"]
    x, xt, mt = loop_data(d)
    params = train_on_cpu(family, init_params(family, d, K), xt, mt)
    eps = loop_eps(1)[0]
    a32 = oracle_loop(port(family, params), x, eps, M, steps)
    a64 = oracle_loop(port64(family, params), x, eps, M, steps)
    live = a32["R_hist"] != -1e4
    scale = float(a32["R_hist"][live].abs().max())
    same = history_match(a32["action"].numpy(), a64["action"].numpy())
    print(family, d, K, "rows with the same history per step:", same.mean(1).tolist(), "reward scale", scale)
    assert scale > 1e-3  # the trained encoder does discriminate between candidates
    assert np.all(same.mean(1) >= 0.9)
