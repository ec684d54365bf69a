"""The host side of the mask-augmented and point-net ensemble evaluation, without a GPU: the float64 closed form the GPU tests
hold the kernels to (against the reference's own numbers), the split of a sweep into family groups, eval_sweep's routing and the
refusals the evaluators make before anything touches the device."""
import pytest
import torch

import vpc_amd as vpc
from family_eval_cases import GOLDEN_TAGS, L, TP, batch_ranges, build, golden_case, oracle_eval, rel
from vpc_amd import ensemble as E
from vpc_amd import harness as H


def _k40():
    """A point-net model that says emb_dim = 40 (the class itself builds none past 32: the evaluator's own check is what is met)."""
    m = build("eddi", "van", 14, K=32)
    m.emb_dim = 40
    return m


# ----------------------------------------------------------------------------------------------- 1. closed form == reference
@pytest.mark.parametrize("tag", sorted(GOLDEN_TAGS))
def test_closed_form_agrees_with_the_reference(tag):
    family, kind, params, x, mask, eps_q, llh = golden_case(tag)
    B = x.shape[0]
    want, every = oracle_eval(family, params, x, mask, eps_q, batch_ranges(B, B, 1))
    assert every
    print(tag, "closed form", want.tolist(), "reference", llh.tolist(), "rel", rel(want[1:], llh))
    assert rel(want[1:], llh) < 3e-6  # (test_oracle_golden.py's bound)
    assert 0.25 <= want[0] <= 0.33  # (a fresh model on x ~ U(0, 1): the GPU tests' rmse bound needs rmse >= 0.25)


# ----------------------------------------------------------------------------------------------- 2. the split
def test_family_eval_groups_splits_a_mixed_list():
    ms = [build("mask", "reg", 14), build("eddi", "reg", 14, K=10), build("mask", "van", 14), build("mask", "reg", 14),
          build("eddi", "reg", 14, K=20), vpc.Reg_VAE(14, 500, 10, L, TP, "e", "kl_reg"), build("eddi", "reg", 14, K=10),
          vpc.MIWAE(14, 500, 10, L, TP, 5, 1)]
    groups, rest = H.family_eval_groups(ms, [dict(vae_type="x")] * len(ms))
    assert sorted(groups.values()) == [[0, 3], [1, 6], [2], [4]] and rest == [7]  # (the plain Reg_VAE, 5, is eval_groups' own)
    assert H.eval_groups(ms)[0] == {(vpc.Reg_VAE, "kl_reg"): [5]}
    by = {tuple(v): k for k, v in groups.items()}
    assert by[(0, 3)] == ("mask", vpc.Reg_VAE_mask, 14, L, "kl_reg") and by[(2,)] == ("mask", vpc.vanilla_VAE_mask, 14, L, None)
    assert by[(1, 6)] == ("eddi", vpc.Reg_EDDI, 14, 10, L, "kl_reg") and by[(4,)] == ("eddi", vpc.Reg_EDDI, 14, 20, L, "kl_reg")
    # the grouping is on class, shape and reg_type: another obs_dim, latent_dim or reg_type is another group
    ms2 = [build("mask", "reg", 14), build("mask", "reg", 12), build("mask", "reg", 14, latent=6),
           build("mask", "reg", 14, reg_type="ml_reg"), build("eddi", "van", 14), build("eddi", "van", 13)]
    assert sorted(H.family_eval_groups(ms2)[0].values()) == [[g] for g in range(6)]
    # past the families' kernels: no family, the member goes alone
    wide = [build("mask", "van", 70), build("mask", "van", 70), build("eddi", "van", 70), build("eddi", "van", 70), _k40(), _k40()]
    assert H.family_eval_groups(wide) == ({}, [0, 1, 2, 3, 4, 5])


# ----------------------------------------------------------------------------------------------- 3. eval_sweep's routing
def test_eval_sweep_routes_family_members(monkeypatch):
    ms = [build("mask", "reg", 14), build("eddi", "reg", 14), build("mask", "reg", 14)]
    cfgs = [dict(vae_type="reg_vae1_mask_augm", alpha=0.5, seed=11), dict(vae_type="reg_EDDI1", alpha=0.5, seed=12),
            dict(vae_type="reg_vae2_mask_augm_with_drop", alpha=0.8, p_missingness=50, seed=13)]
    g = torch.Generator().manual_seed(0)
    x, mk = torch.rand(21, 14, generator=g), torch.rand(21, 14, generator=g) < 0.7
    loader = [(x[:16], mk[:16]), (x[16:], mk[16:])]
    calls = {"mask": [], "eddi": [], "plain": [], "alone": []}

    def stub(name):
        class StubEvaluator:
            def __init__(self, models, seeds=None):
                self.models, self.seeds = list(models), list(seeds)

            def evaluate(self, x, mask, M=1, *, batches, epoch, beta, beta_annealing):
                calls[name].append((self.models, self.seeds, tuple(x.shape), batches, M, epoch, beta))
                return torch.arange(4.0).repeat(len(self.models), 1) + 10 * torch.tensor(self.seeds)[:, None]
        return StubEvaluator

    def stub_eval_vae(list_loaders, *a, model=None, save=True, **kw):
        calls["alone"].append((model, a[9], a[14], a[16], save))  # vae_type, alpha, p_missingness by position
        return {s: "alone" for _, s in list_loaders}

    monkeypatch.setattr(H, "EnsembleEvaluator", stub("plain"))
    monkeypatch.setattr(H, "MaskEnsembleEvaluator", stub("mask"))
    monkeypatch.setattr(H, "EDDIEnsembleEvaluator", stub("eddi"))
    monkeypatch.setattr(H, "eval_vae", stub_eval_vae)
    out = H.eval_sweep([(loader, "train"), (loader[:1], "test")], cfgs, 30, 14, 500, 10, 2, L, "uci", TP, "e", 7, 1, 1,
                       device=torch.device("cpu"), beta=0.7, models=ms, save=False)
    # the lone point-net member went through eval_vae, with its own config
    assert [c[0] for c in calls["alone"]] == [ms[1]] and calls["alone"][0][1:] == ("reg_EDDI1", 0.5, 30, False)
    assert out[1] == {"train": "alone", "test": "alone"}
    # the two mask members (one of them a 'with_drop' run) share ONE MaskEnsembleEvaluator: one evaluate call per loader stage
    # over the batches of both passes gathered behind each other
    assert calls["plain"] == [] and calls["eddi"] == [] and len(calls["mask"]) == 2
    assert all(c[0] == [ms[0], ms[2]] and c[1] == [11, 13] for c in calls["mask"])
    shapes = [(c[2], tuple(map(tuple, c[3]))) for c in calls["mask"]]
    assert shapes == [((42, 14), (((0, 16), (16, 21)), ((21, 37), (37, 42)))), ((32, 14), (((0, 16),), ((16, 32),)))]
    assert all(c[4] == 2 and c[5] == 7 and c[6] == 0.7 for c in calls["mask"])
    for g, seed in ((0, 11), (2, 13)):
        for stage in ("train", "test"):
            r = out[g][stage]
            assert [float(r[k]) for k in ("rmse", "elbo", "negll", "negll_imp")] == [10.0 * seed + i for i in range(4)]


# ----------------------------------------------------------------------------------------------- 4. refusals on the host
def test_evaluators_validate_before_any_device_call():
    M_, E_ = E.MaskEnsembleEvaluator, E.EDDIEnsembleEvaluator
    plain = vpc.Reg_VAE(14, 500, 10, L, TP, "e", "kl_reg")
    cases = [(M_, [build("mask", "reg", 14), build("mask", "van", 14)], TypeError, {}),  # mixed classes
             (E_, [build("eddi", "reg", 14), build("eddi", "van", 14)], TypeError, {}),
             (M_, [build("mask", "van", 70)] * 2, vpc.VpcError, {}),  # 2 * obs_dim > 128
             (E_, [_k40()] * 2, vpc.VpcError, {}),  # emb_dim > 32
             (E_, [build("eddi", "van", 70)] * 2, vpc.VpcError, {}),  # obs_dim > 64
             (M_, [build("mask", "reg", 14)] * 2, vpc.VpcError, dict(world_size=2)),
             (E_, [build("eddi", "reg", 14)] * 2, vpc.VpcError, dict(world_size=2)),
             (M_, [plain], TypeError, {}), (E_, [plain], TypeError, {}),  # a plain model
             (M_, [build("eddi", "reg", 14)], TypeError, {}), (E_, [build("mask", "reg", 14)], TypeError, {})]
    for cls, models, exc, kw in cases:
        with pytest.raises(exc) as ei:  # (CPU models: a device call would raise "... got a CPU tensor" instead)
            cls(models, **kw)
        assert "CPU tensor" not in str(ei.value), (cls.__name__, str(ei.value))
    # the plain evaluator and the acquirer still take plain members only
    for cls in (E.EnsembleEvaluator, E.EnsembleAcquirer):
        with pytest.raises(vpc.VpcError, match="plain"):
            cls([build("mask", "reg", 14)])
        with pytest.raises(TypeError):
            cls([build("eddi", "reg", 14)])
    assert {"MaskEnsembleEvaluator", "EDDIEnsembleEvaluator"} <= set(vpc.__all__)


def test_for_trainer_takes_its_own_family():
    class FakeTrainer:
        family = E.EDDI
    with pytest.raises(TypeError, match="own family"):
        E.MaskEnsembleEvaluator.for_trainer(FakeTrainer())
    with pytest.raises(TypeError, match="own family"):
        E.EDDIEnsembleEvaluator.for_trainer(object())
