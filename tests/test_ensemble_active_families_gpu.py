"""The acquisition loop of the mask-augmented and point-net sweeps (ensemble.MaskEnsembleAcquirer: vpc_impute_small_multi_aug_f32,
ensemble.EDDIEnsembleAcquirer: vpc_impute_small_multi_eddi_f32 + vpc_eddi_fold_multi, both + vpc_reward_matrix_multi_ex,
vpc_acquire_multi, vpc_target_mse_multi; active.active_sweep) on the MI355X.

Numbers are held to the oracle (oracle.vae_oracle.TorchPort(mask_augm=True), oracle.eddi_oracle.EDDIPort, reward_matrix,
active_learning_loop) and to the reference's own rewards (tests/golden/reward_vaemask_d14.npz, reward_eddi_d14.npz); structure
(members, chunks, draws, freshness) is compared with torch.equal: the same kernel on the same buffers, so a difference is an
indexing defect, not rounding."""
import os

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from conftest import golden_params, load_golden
from ensemble_active_cases import history_match, oracle_loop
from ensemble_active_family_cases import LOOP, loop_data, loop_eps, port
from family_eval_cases import L, TP, build, copy_of, params_of
from oracle import vae_oracle as O
from vpc_amd import active as A
from vpc_amd import ensemble as E
from vpc_amd import ops
from vpc_amd.eddi import eddi_fold

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACQ = {"mask": E.MaskEnsembleAcquirer, "eddi": E.EDDIEnsembleAcquirer}
TRAINER = {"mask": E.MaskEnsembleTrainer, "eddi": E.EDDIEnsembleTrainer}
FOLD = {"mask": 0, "eddi": 1}  # launches of the once-per-call fold
# one width per instantiation of the two forward kernels
WIDTHS = [("mask", 6, 0), ("mask", 14, 0), ("mask", 20, 0), ("mask", 40, 0),
          ("eddi", 14, 10), ("eddi", 20, 10), ("eddi", 40, 10), ("eddi", 14, 20), ("eddi", 20, 20), ("eddi", 40, 32)]


def rand_masks(G, n, d, seed, keep=0.4):
    """[G, n, d] bool, the target (last column) unobserved."""
    mk = torch.rand(G, n, d, generator=torch.Generator().manual_seed(seed)) < keep
    mk[:, :, -1] = False
    return mk


def models(family, kind, d, K, G, seed):
    torch.manual_seed(seed)
    return [build(family, kind, d, K or 10).to(DEV) for _ in range(G)]


# ----------------------------------------------------------------------------------------------- 1. impute vs oracle
@pytest.mark.parametrize("family,d,K", WIDTHS)
def test_impute_vs_oracle(family, d, K):
    n, M, G = 21, 3, 3
    g = torch.Generator().manual_seed(d + K)
    ms = models(family, "reg", d, K, G, seed=d + K)
    x = torch.rand(G, n, d, generator=g)
    mask = rand_masks(G, n, d, seed=d + 1, keep=0.6)
    eps = torch.randn(G, M * n, L, generator=g)
    acq = ACQ[family](ms)
    im = acq.impute(x.to(DEV), mask.to(DEV), M, 0, eps=eps.to(DEV))
    sq = acq.impute(x.to(DEV), mask.to(DEV), M, 1, eps=eps.to(DEV))
    assert tuple(im.shape) == (G, M, n, d) and tuple(sq.shape) == (G, M * n) and acq.launches == 1
    for k in range(G):
        pt = port(family, params_of(ms[k]))
        with torch.no_grad():
            z, _, _ = pt.encoder(x[k].repeat(M, 1), mask[k].repeat(M, 1), eps=eps[k])
            want = pt.decoder(z)[0].reshape(M, n, d)
        err = float((im[k].cpu() - want).abs().max())
        print(family, "d", d, "K", K, "member", k, "max |x_hat - oracle|", err)
        assert err <= 2e-5  # tests/test_gpu_parity.py's bound on x_mean_q
    # mode 1 is the squared target error of mode 0's output, exactly
    assert torch.equal(sq.view(G, M, n), (im[..., -1] - x.to(DEV)[:, None, :, -1]) ** 2)


# ----------------------------------------------------------------------------------------------- 2. impute indexing
@pytest.mark.parametrize("family,kind,d,K", [("mask", "reg", 40, 0), ("mask", "van", 14, 0), ("eddi", "reg", 14, 20),
                                             ("eddi", "van", 40, 10)])
def test_impute_member_equals_its_stand_alone_call_bitwise(family, kind, d, K):
    n, M, G = 21, 3, 9
    ms = models(family, kind, d, K, G, seed=7)
    twins = [copy_of(family, m, DEV) for m in ms]
    seeds = [3 + 5 * k for k in range(G)]
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(1)).to(DEV)
    mask = rand_masks(G, n, d, seed=2, keep=0.5).to(DEV)
    acq = ACQ[family](ms, seeds=seeds)
    im = acq.impute(x, mask, M, 0, max_blocks=9)  # device draws; one tile per launch: the chunk loop runs
    assert acq.launches == acq.tables(n, n, M)[0].tiles.shape[0] == 2 * M
    sq = acq.impute(x, mask, M, 1, max_blocks=9)
    assert torch.isfinite(im).all() and len({float(v) for v in im[:, 0, 0, 0]}) == G
    for k in range(G):
        alone = ACQ[family]([twins[k]], seeds=[seeds[k]])
        assert torch.equal(alone.impute(x, mask[k:k + 1], M, 0)[0], im[k]), k
        assert torch.equal(alone.impute(x, mask[k:k + 1], M, 1)[0], sq[k]), k


@pytest.mark.parametrize("family,K", [("mask", 0), ("eddi", 10)])
def test_impute_draw_rule(family, K):
    d, n, M, G = 14, 21, 3, 2
    ms = models(family, "reg", d, K, G, seed=1)
    seeds = [5, 2 ** 40 + 6]
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(4)).to(DEV)
    mask = rand_masks(G, n, d, seed=3).to(DEV)
    R = M * n
    acq = ACQ[family](ms, seeds=seeds)
    first = acq.impute(x, mask, M, 0)
    assert acq.rng_offset == 4 * R
    second = acq.impute(x, mask, M, 0)  # two consecutive calls: the offset advance
    assert acq.rng_offset == 8 * R and not torch.equal(first, second)
    inj = ACQ[family](ms, seeds=seeds)
    for offset, want in ((0, first), (4 * R, second)):
        planes = torch.empty(G, R * 16, device=DEV)
        for k in range(G):
            ops.fill_normal(planes[k], seeds[k], offset)
        assert torch.equal(inj.impute(x, mask, M, 0, eps=planes.view(G, R, 16)[:, :, :L]), want), offset
    assert inj.rng_offset == 0  # injected eps consume no counters


# ----------------------------------------------------------------------------------------------- 3. reward
@pytest.mark.parametrize("family", ["mask", "eddi"])
@pytest.mark.parametrize("d,n,M", [(14, 5, 3), (14, 21, 17), (40, 21, 3), (40, 5, 17)])
def test_reward_multi_equals_reward_matrix_bitwise(family, d, n, M):
    G, K = 3, (0 if family == "mask" else 20 if d == 14 else 32)
    seed = d + n + M
    g = torch.Generator().manual_seed(seed)
    ms = models(family, "reg", d, K, G, seed=seed)
    x = torch.rand(G, n, d, generator=g).to(DEV)
    mask = rand_masks(G, n, d, seed=seed + 1)
    mask[1, 0, :d - 1] = True
    mask[1, 0, (d - 1) // 2] = False  # a row with a single unobserved candidate
    mask = mask.to(DEV)
    im = torch.rand(G, M, n, d, generator=g).to(DEV)
    acq = ACQ[family](ms)
    R = acq.reward(x, mask, im)
    assert acq.launches == 3 + FOLD[family]
    sizes = ops.reward_scratch_multi_ex(acq.kind, n, d, M, K)
    R2 = acq.reward(x, mask, im, ws_floats=2 * sum(sizes))  # two members fit: two member chunks
    assert acq.launches == 6 + FOLD[family]
    assert int((R[1, 0] != -1e4).sum()) == 1
    for k in range(G):
        want = A.reward_matrix(ms[k], x[k], mask[k], im[k])
        assert torch.equal(R[k], want), k
        assert torch.equal(R2[k], want), k
        if family == "eddi":
            # the folded front-end is vpc_eddi_fold's, and [W2 | W3] of the trunk image is the image active.reward_matrix packs
            AC = torch.empty(2, K, d, device=DEV)
            eddi_fold(*[p.data for p in ms[k].trainable()[12:16]], AC, d, K)
            assert torch.equal(acq._AC[k, :2 * K * d].view(2, K, d), AC), k
            lay = acq.lay
            assert torch.equal(acq.img[k, lay.enc_img - E.W23_FLOATS:lay.enc_img], A._w23_image(ms[k])), k
    assert not torch.equal(R[0], R[1])


def _check(R, want, atol=2e-6, min_scale=1e-4):  # tests/test_reward_families.py::_check
    assert np.array_equal(R == -1e4, want == -1e4)
    live = want != -1e4
    scale = np.max(np.abs(want[live]))
    assert scale > min_scale  # a trained encoder: rewards well above round-off
    err = np.max(np.abs(R[live] - want[live]))
    print("max |R - reference|", err, "scale", scale)
    assert err <= atol + 1e-3 * scale, (err, scale)


@pytest.mark.parametrize("family,fixture", [("mask", "reward_vaemask_d14.npz"), ("eddi", "reward_eddi_d14.npz")])
def test_reward_multi_vs_the_reference(family, fixture):
    g = load_golden(fixture)
    d = g["x"].shape[1]
    pr = golden_params(g)
    noise = torch.Generator().manual_seed(0)
    pm = {k: v + 0.01 * torch.randn(v.shape, generator=noise) for k, v in pr.items()}  # member 1: a perturbed copy
    ms = [build(family, "reg", d, params=p).to(DEV) for p in (pr, pm, pr)]
    acq = ACQ[family](ms)
    x, im = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["im"]).to(DEV)
    for tag in ("t0", "t1"):
        mask = torch.from_numpy(g[f"mask_{tag}"]).to(DEV)
        R = acq.reward(x, mask[None].expand(3, -1, -1).contiguous(), im[None].expand(3, -1, -1, -1).contiguous()).cpu().numpy()
        for k in (0, 2):
            _check(R[k], g[f"R_{tag}"])
        assert np.array_equal(R[0], R[2]) and not np.array_equal(R[0], R[1])


# ----------------------------------------------------------------------------------------------- 5. the loop vs the oracle
@pytest.mark.parametrize("family,K", [("mask", 0), ("eddi", 10)])
def test_loop_vs_oracle(family, K):
    """Measured on an MI355X (max over members and steps): see profiles/ensemble_active_families_notes.md."""
    d, n, M, steps = 40, LOOP["n"], LOOP["M"], LOOP["steps"]
    x, xt, mt = loop_data(d)
    torch.manual_seed(3)
    m0 = build(family, "reg", d, K or 10).to(DEV)
    tr = vpc.FusedTrainer(m0) if family == "mask" else vpc.EDDITrainer(m0)
    xt, mt = xt.to(DEV), mt.to(DEV)
    for i in range(200):  # a briefly trained model: rewards of a random-init encoder are all round-off
        tr.step(xt, mt, alpha=1.0, epoch=i + 1)
    p0 = params_of(m0)
    for i in range(100):  # member 1: a further-trained copy
        tr.step(xt, mt, alpha=1.0, epoch=201 + i)
    p1 = params_of(m0)
    ms = [build(family, "reg", d, K or 10, params=p).to(DEV) for p in (p0, p1)]
    eps = loop_eps(2)
    acq = ACQ[family](ms)
    info, action, R_hist, im_hist = [t.cpu().numpy() for t in acq.run(x.to(DEV), M, max_steps=steps, eps=eps.to(DEV))]
    assert info.shape == (2, 1, d) and action.shape == (2, 1, n, d - 1) and R_hist.shape == (2, 1, d - 1, n, d - 1)
    assert im_hist.shape == (2, 1, d - 1, M, n, d)
    assert not info[:, :, steps + 1:].any() and not action[:, :, :, steps:].any() and not R_hist[:, :, steps:].any()
    assert acq.launches == FOLD[family] + 2 + steps * 7 and acq.launches_per_step == 7
    for k, p in enumerate((p0, p1)):
        ref = oracle_loop(port(family, p), x, eps[k], M, steps)
        want, act_ref = ref["R_hist"].numpy(), ref["action"].numpy().astype(np.int64)
        act = action[k, 0, :, :steps].astype(np.int64)
        live = want != -1e4
        scale = np.max(np.abs(want[live]))
        tol = 2e-6 + 1e-3 * scale  # the bound these first-layer kinds are held to against the oracle (test_reward_families._check)
        same = history_match(act, act_ref)
        print(family, "member", k, "scale", scale, "rows with the oracle's history per step", same.mean(1).tolist())
        assert scale > 1e-3  # the trained encoder does discriminate between candidates
        assert np.all(same.mean(1) >= 0.9)
        for t in range(steps):
            rows = same[t]
            R = R_hist[k, 0, t]
            assert np.array_equal(R[rows] == -1e4, want[t][rows] == -1e4), (k, t)
            err = np.max(np.abs(R[rows] - want[t][rows]))
            print(family, "member", k, "step", t, "max |R - oracle|", err, "tol", tol, "plain bound", 1e-4 * scale + 5e-7)
            assert err <= tol, (k, t, err, tol)
            # the picked feature is the oracle's, or one within that tolerance of its best
            gap = want[t][rows].max(1) - want[t][rows][np.arange(rows.sum()), act[rows, t]]
            assert np.all(gap <= tol), (k, t, gap.max())
            im_err = np.max(np.abs(im_hist[k, 0, t][:, rows] - ref["im"].numpy()[t][:, rows]))
            print(family, "member", k, "step", t, "max |im - oracle|", im_err)
            assert im_err <= 2e-5
        # the curve, while all rows match (the bound of tests/test_ensemble_active_gpu.py::test_loop_vs_oracle)
        want_c = ref["info_curve"].numpy()
        for t in range(steps + 1):
            if same[t].all():
                assert abs(info[k, 0, t] - want_c[t]) <= 1e-5 * abs(want_c[t]) + 1e-7 + 4e-5, (k, t, info[k, 0, t], want_c[t])


# ----------------------------------------------------------------------------------------------- 6. device draws, freshness
def _golden_members(family, G, scale=0.005):
    g = load_golden({"mask": "reward_vaemask_d14.npz", "eddi": "reward_eddi_d14.npz"}[family])
    pr = golden_params(g)
    noise = torch.Generator().manual_seed(1)
    plist = [pr] + [{k: v + scale * torch.randn(v.shape, generator=noise) for k, v in pr.items()} for _ in range(G - 1)]
    return [build(family, "reg", g["x"].shape[1], params=p).to(DEV) for p in plist]


@pytest.mark.parametrize("family", ["mask", "eddi"])
def test_loop_properties_with_device_draws(family):
    d, n, M, G, rep = 14, 24, 25, 4, 2
    ms = _golden_members(family, G)
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(5)).to(DEV)
    seeds = [11, 12, 13, 14]
    acq = ACQ[family](ms, seeds=seeds)
    info, action, R_hist, im_hist = acq.run(x, M, repeats=rep)
    calls = rep * (1 + 2 * (d - 1))
    assert acq.rng_offset == calls * 4 * M * n
    assert acq.launches_per_step == 7 and acq.launches == FOLD[family] + rep * (2 + (d - 1) * 7)
    act = action.cpu().numpy()
    for k in range(G):
        for r in range(rep):
            for row in act[k, r]:
                assert sorted(row) == list(range(d - 1))  # every row acquires d - 1 distinct features
    assert not torch.equal(info[:, 0], info[:, 1]) and not torch.equal(im_hist[:, 0], im_hist[:, 1])  # two repeats differ
    # the same seeds reproduce the run bit for bit in a fresh acquirer; keep_im=False gives the same info / action / R_hist
    again = ACQ[family]([copy_of(family, m, DEV) for m in ms], seeds=seeds)
    i2, a2, R2, im2 = again.run(x, M, repeats=rep, keep_im=False)
    assert im2 is None
    assert torch.equal(i2, info) and torch.equal(a2, action) and torch.equal(R2, R_hist)
    i3, a3, R3, im3 = ACQ[family](ms, seeds=seeds).run(x, M, repeats=rep)
    assert torch.equal(i3, info) and torch.equal(a3, action) and torch.equal(R3, R_hist) and torch.equal(im3, im_hist)


@pytest.mark.parametrize("family", ["mask", "eddi"])
def test_run_reads_the_current_weights(family):
    d, n, M, G = 14, 21, 3, 2
    ms = models(family, "reg", d, 10, G, seed=2)
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(9)).to(DEV)
    eps = torch.randn(1 + 2 * 4, M * n, L, generator=torch.Generator().manual_seed(3)).to(DEV)
    run = lambda a: a.run(x, M, max_steps=4, eps=eps, keep_im=False)[:3]
    acq = ACQ[family](ms)
    r0 = run(acq)
    ms[0].load_state_dict({k: v.detach().clone() for k, v in ms[1].state_dict().items()})  # in place
    r1 = run(acq)
    assert not torch.equal(r0[0][0], r1[0][0]) and torch.equal(r0[0][1], r1[0][1])
    for a in r1:
        assert torch.equal(a[0], a[1])  # member 0 now computes what member 1 computes
    fresh = run(ACQ[family]([copy_of(family, m, DEV) for m in ms]))
    for a, b in zip(r1, fresh):
        assert torch.equal(a, b)


@pytest.mark.parametrize("family,d", [("mask", 14), ("eddi", 12)])  # (the point-net trainer draws in its launch where d % 4 == 0)
def test_for_trainer_reads_the_trainers_image_rows(family, d):
    n, M, G, B = 21, 3, 2, 32
    ms = models(family, "reg", d, 10, G, seed=4)
    tr = TRAINER[family](ms, seeds=[21, 22])
    acq = ACQ[family].for_trainer(tr)
    assert acq.table.rows["seed"].tolist() == [21, 22]
    g = torch.Generator().manual_seed(6)
    xb, mb = torch.rand(B, d, generator=g).to(DEV), (torch.rand(B, d, generator=g) < 0.7).to(DEV)
    x = torch.rand(n, d, generator=g).to(DEV)
    eps = torch.randn(1 + 2 * 3, M * n, L, generator=g).to(DEV)
    run = lambda a: a.run(x, M, max_steps=3, eps=eps)
    tr.step(xb, mb, epoch=1)
    r0 = run(acq)
    tr.step(xb, mb, epoch=2)  # one more trainer step: the tail re-packed the image rows the acquirer reads
    r1 = run(acq)
    assert not torch.equal(r0[2], r1[2])
    fresh = run(ACQ[family]([copy_of(family, m, DEV) for m in ms]))
    for a, b in zip(r1, fresh):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------- 7. active_sweep
def test_active_sweep(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    d, n, M, rep = 14, 21, 3, 2
    torch.manual_seed(6)
    ms = [build("mask", "reg", d).to(DEV), build("eddi", "reg", d).to(DEV), vpc.Reg_VAE(d, 500, 10, L, TP, "exp", "kl_reg").to(DEV),
          build("mask", "reg", d).to(DEV), build("eddi", "reg", d).to(DEV), vpc.Reg_VAE(d, 500, 10, L, TP, "exp", "kl_reg").to(DEV)]
    cfgs = [dict(vae_type="reg_vae1_mask_augm", alpha=0.5, seed=11), dict(vae_type="reg_EDDI1", alpha=0.5, seed=12),
            dict(vae_type="reg_vae1", alpha=0.5, seed=13),
            dict(vae_type="reg_vae2_mask_augm", alpha=0.8, p_missingness=50, seed=14),
            dict(vae_type="reg_EDDI2", alpha=0.8, p_missingness=50, seed=15), dict(vae_type="reg_vae2", alpha=0.8, seed=16)]
    g = torch.Generator().manual_seed(8)
    x, tmask = torch.rand(n, d, generator=g), torch.rand(n, d, generator=g) < 0.7
    out = vpc.active_sweep(None, cfgs, x, tmask, 30, d, 500, 10, M, L, "uci", TP, "exp", 7, 1, 1, reg_type="kl_reg", Repeat=rep,
                           models=ms, save=True, max_steps=4)
    assert len(out) == 6
    shapes = dict(information_curve_CHAI=(rep, n, d), action_CHAI=(rep, n, d - 1), R_hist_CHAI=(rep, d - 1, n, d - 1),
                  im_CHAI=(rep, d - 1, M, n, d))
    seen = set()
    for k, c in enumerate(cfgs):  # the four files of every member, under its own alpha / p_missingness, hold what is returned
        paths = A.active_result_paths("exp", "uci", c["vae_type"], 30, c["alpha"], c.get("p_missingness", 30), "kl_reg")
        assert set(out[k]) == set(paths) == set(shapes)
        for name, pth in paths.items():
            assert os.path.exists(pth) and pth not in seen, pth
            seen.add(pth)
            assert tuple(out[k][name].shape) == shapes[name] and out[k][name].dtype == torch.float32
            assert torch.equal(torch.load(pth, weights_only=True), out[k][name]), (k, name)
    # every pair ran together: what a two-member acquirer of its class with the configs' seeds gives
    for cls, idx in ((E.MaskEnsembleAcquirer, (0, 3)), (E.EDDIEnsembleAcquirer, (1, 4)), (E.EnsembleAcquirer, (2, 5))):
        acq = cls([ms[g] for g in idx], seeds=[cfgs[g]["seed"] for g in idx])
        info, action, R_hist, im_hist = [t.cpu() for t in acq.run(x.to(DEV), M, repeats=rep, max_steps=4)]
        for k, g in enumerate(idx):
            assert torch.equal(out[g]["information_curve_CHAI"], info[k][:, None, :].expand(rep, n, d)), g
            assert torch.equal(out[g]["action_CHAI"], action[k].float()) and torch.equal(out[g]["R_hist_CHAI"], R_hist[k]), g
            assert torch.equal(out[g]["im_CHAI"], im_hist[k]), g
            assert out[g]["information_curve_CHAI"][:, :, :5].min() > 0 and not out[g]["information_curve_CHAI"][:, :, 5:].any()
