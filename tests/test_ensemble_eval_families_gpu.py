"""The ensemble evaluation of the mask-augmented and point-net members on the MI355X (ensemble.MaskEnsembleEvaluator:
vpc_eval_small_multi_aug_f32, ensemble.EDDIEnsembleEvaluator: vpc_eval_small_multi_eddi_f32, both + vpc_eval_reduce_multi;
harness.eval_sweep).

The bounds are those of tests/test_ensemble_eval_gpu.py: (elbo, negll, negll_imp) to 2e-5 relative against the reference's own
numbers and the float64 closed form (family_eval_cases.oracle_eval), rmse to 1e-4 relative where the float64 rmse is >= 0.25
(asserted wherever the bound is used).  Structure (members, tiles, chunks, draws, freshness) is compared with torch.equal: the
same kernel on the same buffers, so a difference is an indexing defect, not rounding."""
import os

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from family_eval_cases import (GOLDEN_TAGS, L, TP, batch_ranges, build, copy_of, data, golden_case, oracle_eval, params_of, rel)
from vpc_amd import ensemble as E
from vpc_amd import harness as H
from vpc_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
EV = {"mask": E.MaskEnsembleEvaluator, "eddi": E.EDDIEnsembleEvaluator}
TRAINER = {"mask": E.MaskEnsembleTrainer, "eddi": E.EDDIEnsembleTrainer}
FRONT = ("type_pars1", "type_bias1", "pnp_encoder1.0.weight", "pnp_encoder1.0.bias")


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def check_numbers(got, want, what):
    got = np.asarray(got, np.float64)
    print(what, "got", got.tolist(), "want", np.asarray(want).tolist(), "rel(llh)", rel(got[1:], want[1:]),
          "rel(rmse)", abs(got[0] - want[0]) / want[0])
    assert want[0] >= 0.25, "the rmse bound was derived for rmse >= 0.25"
    assert rel(got[1:], want[1:]) < 2e-5, what
    assert abs(got[0] - want[0]) <= 1e-4 * want[0], what


# ----------------------------------------------------------------------------------------------- 1. reference numbers
@pytest.mark.parametrize("tag", sorted(GOLDEN_TAGS))
def test_reference_numbers(tag):
    family, kind, params, x, mask, eps_q, llh = golden_case(tag)
    B, d = x.shape
    m = build(family, kind, d, params=params).to(DEV)
    ev = EV[family]([m])
    out = ev.evaluate(_t(x), _t(mask), B, 1, epoch=7, beta=1.0, eps=_t(eps_q))
    assert out.shape == (1, 4) and out.dtype == torch.float32 and out.is_cuda and ev.launches == 2
    want, every = oracle_eval(family, params, x, mask, eps_q, batch_ranges(B, B, 1))
    assert every
    # (elbo, negll, negll_imp) against the reference's own numbers; rmse against the float64 closed form (d = 14: rows of 16
    # columns - padding that leaked into the ~mask sums would show in negll_imp and rmse)
    check_numbers(out[0].cpu().numpy(), np.concatenate([want[:1], llh]), tag)


# ----------------------------------------------------------------------------------------------- 2. shapes against float64
SHAPES = [("mask", 8, 0, 37),    # 2 d fills the input tile exactly
          ("mask", 14, 0, 37),   # pitch 16, column d not 4-aligned
          ("mask", 20, 0, 37),   # (DTI, DT) = (4, 2)
          ("mask", 40, 0, 37),   # (8, 4)
          ("eddi", 13, 10, 37),  # odd pitch
          ("eddi", 14, 20, 37),  # (2, 1)
          ("eddi", 20, 10, 37),  # (1, 2)
          ("eddi", 40, 20, 37)]  # (2, 4)


@pytest.mark.parametrize("family,d,K,N,bs", [s + (bs,) for s in SHAPES for bs in (16, 24)] + [("eddi", 64, 32, 21, 16)])
def test_shapes_vs_float64(family, d, K, N, bs):
    M = 2
    torch.manual_seed(N + d + bs + K)
    kind = "reg" if (d + bs) % 16 else "van"
    m = build(family, kind, d, K)
    params = params_of(m)
    x, mask = data((N, d), seed=bs + d)
    eps = torch.randn(M * N, L, generator=torch.Generator().manual_seed(7))
    ranges = batch_ranges(N, bs, M)
    want, every = oracle_eval(family, params, x, mask, eps, ranges, bw=0.7)
    assert every, "every batch needs an unobserved entry: no case may be silently NaN"
    ev = EV[family]([m.to(DEV)])
    out = ev.evaluate(x.to(DEV), mask.to(DEV), bs, M, epoch=5, beta=0.7, eps=eps.to(DEV))
    check_numbers(out[0].cpu().numpy(), want, (family, kind, d, K, N, bs))
    assert ev.tables(N, bs, M) is ev.tables(N, bs, M) and len(ev._tables) == 1  # built and uploaded once per layout
    # the same layout spelled as explicit ranges gives the same bits
    assert torch.equal(ev.evaluate(x.to(DEV), mask.to(DEV), M=M, batches=ranges, epoch=5, beta=0.7, eps=eps.to(DEV)), out)


# ----------------------------------------------------------------------------------------------- 3. members == stand-alone
@pytest.mark.parametrize("family,kind,d,K,N,G,shared,max_blocks", [("mask", "reg", 14, 0, 37, 3, False, 0),
                                                                   ("eddi", "reg", 14, 10, 37, 3, False, 0),
                                                                   ("eddi", "van", 20, 20, 16, 9, True, 9)])
def test_member_equals_its_stand_alone_evaluation_bitwise(family, kind, d, K, N, G, shared, max_blocks):
    torch.manual_seed(d + K)
    ms = [build(family, kind, d, K).to(DEV) for _ in range(G)]
    twins = [copy_of(family, m, DEV) for m in ms]
    seeds = [3 + 5 * g for g in range(G)]
    betas = [1.0 - 0.1 * g for g in range(G)]
    x, mask = data((N, d) if shared else (G, N, d), seed=G)
    x, mask = x.to(DEV), mask.to(DEV)
    kw = dict(epoch=1400, beta_annealing=True)
    ev = EV[family](ms, seeds=seeds)
    out = ev.evaluate(x, mask, 16, 2, beta=betas, max_blocks=max_blocks, **kw)  # device draws; max_blocks 9: one tile per launch
    if max_blocks:
        assert ev.launches == 2 + 1 and ev.tables(N, 16, 2)[0].tiles.shape[0] == 2
    assert torch.isfinite(out).all() and len({tuple(r) for r in out.tolist()}) == G
    for g in range(G):
        alone = EV[family]([twins[g]], seeds=[seeds[g]])
        r = alone.evaluate(x if shared else x[g], mask if shared else mask[g], 16, 2, beta=betas[g], **kw)
        assert torch.equal(r[0], out[g]), (g, r[0].tolist(), out[g].tolist())


# ----------------------------------------------------------------------------------------------- 4. the draw rule
def test_point_net_draws_on_the_device_at_any_obs_dim():
    d, K, N, M, G = 13, 10, 37, 2, 2  # (obs_dim % 4 != 0: EDDIEnsembleTrainer.step refuses to draw here, evaluation does not)
    torch.manual_seed(1)
    ms = [build("eddi", "reg", d, K).to(DEV) for _ in range(G)]
    seeds = [5, 2 ** 40 + 6]
    x, mask = data((N, d), seed=4)
    x, mask = x.to(DEV), mask.to(DEV)
    kw = dict(epoch=1, beta=1.0)
    ev = E.EDDIEnsembleEvaluator(ms, seeds=seeds)
    first = ev.evaluate(x, mask, 16, M, **kw)
    R = M * N
    assert ev.rng_offset == 4 * R
    second = ev.evaluate(x, mask, 16, M, **kw)
    assert ev.rng_offset == 8 * R and not torch.equal(first, second) and torch.isfinite(first).all()
    # the eps of draw row r under member g is what fill_normal writes into a flat [R x 16] array with the member's seed and the
    # call's offset: injecting those planes reproduces both calls bit for bit
    inj = E.EDDIEnsembleEvaluator(ms, seeds=seeds)
    for offset, want in ((0, first), (4 * R, second)):
        planes = torch.empty(G, R * 16, device=DEV)
        for g in range(G):
            ops.fill_normal(planes[g], seeds[g], offset)
        got = inj.evaluate(x, mask, 16, M, eps=planes.view(G, R, 16)[:, :, :L], **kw)
        assert torch.equal(got, want), offset
    assert inj.rng_offset == 0  # injected eps consume no counters


# ----------------------------------------------------------------------------------------------- 5. freshness
@pytest.mark.parametrize("family,d", [("mask", 14), ("eddi", 12)])
def test_evaluation_reads_the_current_weights(family, d):
    N, G = 37, 2
    torch.manual_seed(2)
    ms = [build(family, "reg", d).to(DEV) for _ in range(G)]
    x, mask = data((N, d), seed=9)
    x, mask = x.to(DEV), mask.to(DEV)
    eps = torch.randn(2 * N, L, generator=torch.Generator().manual_seed(3)).to(DEV)
    run = lambda e: e.evaluate(x, mask, 16, 2, epoch=1, beta=1.0, eps=eps)
    fresh = lambda: run(EV[family]([copy_of(family, m, DEV) for m in ms]))
    ev = EV[family](ms)  # (built before the trainer)
    r0 = run(ev)
    tr = TRAINER[family](ms)
    ev2 = EV[family].for_trainer(tr)
    assert ev2.models == tr.models and ev2.table.rows["seed"].tolist() == tr.table.rows["seed"].tolist()
    for _ in range(2):
        tr.step(x, mask, epoch=1)
    r1 = run(ev)
    assert not torch.equal(r0, r1) and not torch.equal(r1[0], r1[1])
    assert torch.equal(run(ev2), r1)
    assert torch.equal(fresh(), r1)
    state = lambda m: {k: v.detach().clone() for k, v in m.state_dict().items()}
    if family == "eddi":
        # the front-end is part of what is evaluated: a copy of member 1 without it gives neither member's numbers
        ms[0].load_state_dict({**state(ms[1]), **{k: v for k, v in state(ms[0]).items() if k in FRONT}})
        ra = run(ev)
        assert not torch.equal(ra[0], r1[1]) and not torch.equal(ra[0], r1[0]) and torch.equal(ra[1], r1[1])
        assert torch.equal(run(ev2), ra) and torch.equal(fresh(), ra)
    # an in-place load_state_dict (the point-net front-end included)
    ms[0].load_state_dict(state(ms[1]))
    r2 = run(ev)
    assert torch.equal(r2[0], r1[1]) and torch.equal(r2[1], r1[1]) and not torch.equal(r2[0], r1[0])
    assert torch.equal(run(ev2), r2) and torch.equal(fresh(), r2)


def test_point_net_member_that_left_the_stack_is_named():
    torch.manual_seed(3)
    ms = [build("eddi", "van", 12).to(DEV) for _ in range(2)]
    x, mask = data((16, 12), seed=1)
    ev = E.EDDIEnsembleEvaluator(ms)
    ev.evaluate(x.to(DEV), mask.to(DEV), 16, 1, epoch=1)
    ms[1].to("cpu")
    ms[1].to(DEV)
    ms[1].flatten_parameters()  # (a buffer of its own: the front-end of row 1 of the stack is no longer this model's)
    with pytest.raises(vpc.VpcError, match="member 1 no longer sits"):
        ev.evaluate(x.to(DEV), mask.to(DEV), 16, 1, epoch=1)


# ----------------------------------------------------------------------------------------------- 6. eval_sweep
def test_eval_sweep(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    d, M, epochs, beta = 14, 2, 7, 0.7
    torch.manual_seed(6)
    ms = [build("mask", "reg", d).to(DEV), build("eddi", "van", d).to(DEV), build("eddi", "reg", d).to(DEV),
          build("mask", "reg", d).to(DEV), build("eddi", "van", d).to(DEV)]
    cfgs = [dict(vae_type="reg_vae1_mask_augm", alpha=0.5, seed=11), dict(vae_type="vanilla_EDDI1", seed=12),
            dict(vae_type="reg_EDDI1", alpha=0.5, seed=13), dict(vae_type="reg_vae2_mask_augm", alpha=0.8, p_missingness=50, seed=14),
            dict(vae_type="vanilla_EDDI2", seed=15)]
    x, mask = data((32, d), seed=8)
    loaders = [([(x[:16], mask[:16]), (x[16:], mask[16:])], "test")]
    args = (30, d, 500, 10, M, L, "uci", TP, "exp")
    torch.manual_seed(21)
    out = H.eval_sweep(loaders, cfgs, *args, epochs, 1, 1, reg_type="kl_reg", beta=beta, models=ms, save=True)
    assert len(out) == 5
    for g, c in enumerate(cfgs):  # the four files of every member, under its own alpha / p_missingness, hold what is returned
        paths = H.result_paths("exp", "uci", c["vae_type"], "test", 30, c.get("alpha", 1.0), c.get("p_missingness", 30), "kl_reg")
        assert set(out[g]["test"]) == set(paths) == {"rmse", "elbo", "negll", "negll_imp"}
        for k, pth in paths.items():
            assert os.path.exists(pth), pth
            assert torch.equal(torch.load(pth, weights_only=True), out[g]["test"][k]), (g, k)
            assert torch.isfinite(out[g]["test"][k])
    assert len({os.path.abspath(p) for g, c in enumerate(cfgs) for p in H.result_paths(
        "exp", "uci", c["vae_type"], "test", 30, c.get("alpha", 1.0), c.get("p_missingness", 30), "kl_reg").values()}) == 20
    # the lone Reg_EDDI is the fallback: eval_vae alone, under the same torch seed, exactly
    torch.manual_seed(21)
    ref = H.eval_vae(loaders, *args, "reg_EDDI1", epochs, 1, 1, alpha=0.5, reg_type="kl_reg", beta=beta, model=ms[2], save=False)
    for k, v in ref["test"].items():
        assert torch.equal(v, out[2]["test"][k]), k
    # the grouped members: one evaluate call per group over the batches of both passes, gathered behind each other
    xg, mg = torch.cat([x, x]).to(DEV), torch.cat([mask, mask]).to(DEV)
    ranges = [[(0, 16), (16, 32)], [(32, 48), (48, 64)]]
    for family, idx in (("mask", [0, 3]), ("eddi", [1, 4])):
        ev = EV[family]([ms[g] for g in idx], seeds=[cfgs[g]["seed"] for g in idx])
        r = ev.evaluate(xg, mg, M=M, batches=ranges, epoch=epochs, beta=beta).cpu()
        for k, g in enumerate(idx):
            got = torch.stack([out[g]["test"][n] for n in ("rmse", "elbo", "negll", "negll_imp")])
            assert torch.equal(got, r[k]), g


# ----------------------------------------------------------------------------------------------- 7. the C entries refuse
def test_c_entries_refuse_bad_arguments():
    N, Ld = 16, L
    tb = E.build_eval_tables(N, 16, 1)
    tiles = torch.from_numpy(tb.tiles).to(DEV)
    members = torch.zeros(64, dtype=torch.uint8, device=DEV)
    img = torch.zeros(1 << 16, device=DEV)
    part = torch.full((5,), 7.0, dtype=torch.float64, device=DEV)
    eps = torch.zeros(N, 16, device=DEV)
    front = torch.zeros(4096, device=DEV)

    def strides(dk, param):
        return ops.stride_vector(ops.MS_COUNT, {ops.MS_X: N * dk, ops.MS_MASK: N * dk, ops.MS_EPS: N * 16, ops.MS_IMG: 1 << 15,
                                                ops.MS_PART: 5, ops.MS_PARAM: param})

    def aug(d, d_real):
        x, mk = torch.zeros(N, d, device=DEV), torch.zeros(N, d, dtype=torch.uint8, device=DEV)
        ops.eval_small_multi_aug_f32(x, mk, eps, img, img[1 << 14:], members, 1, tiles, 1, N, N, False, 0, -3.9, part,
                                     strides(d, 0), d, d_real, Ld)

    def eddi(d, d_real, K, front, param):
        x, mk = torch.zeros(N, d, device=DEV), torch.zeros(N, d, dtype=torch.uint8, device=DEV)
        ops.eval_small_multi_eddi_f32(x, mk, eps, img, img[1 << 14:], members, 1, tiles, 1, N, N, False, 0, -3.9, part,
                                      strides(d, param), d, d_real, Ld, K, front)

    n_front = 14 * 10 + 14 + 10 * 12 + 10
    with pytest.raises(vpc.VpcError, match="shape"):
        aug(72, 70)  # 2 * d_real > 128
    with pytest.raises(vpc.VpcError, match="shape"):
        eddi(16, 14, 33, front, 4096)  # K > 32
    with pytest.raises(vpc.VpcError, match="shape"):
        eddi(16, 14, 0, front, 4096)
    with pytest.raises(vpc.VpcError, match="shape"):
        eddi(68, 68, 10, front, 4096)  # d_real > 64
    with pytest.raises(vpc.VpcError, match="bad argument"):
        eddi(16, 14, 10, front.view(torch.uint8)[2:2 + 4 * 2048].view(torch.uint8), 4096)  # front not 4-byte aligned
    with pytest.raises(vpc.VpcError, match="bad argument"):
        eddi(16, 14, 10, None, 4096)
    with pytest.raises(vpc.VpcError, match="bad argument"):
        eddi(16, 14, 10, front, n_front - 1)  # a member stride smaller than the front-end
    torch.cuda.synchronize()
    assert bool((part == 7.0).all())  # nothing was launched
