"""The ensemble acquisition loop (ensemble.EnsembleAcquirer: vpc_impute_small_multi_f32, vpc_reward_matrix_multi, vpc_acquire_multi,
vpc_target_mse_multi; active.active_sweep) on the MI355X.

Numbers are held to the oracle (oracle.vae_oracle: TorchPort, reward_matrix, active_learning_loop) and to the vectors recorded from
the reference's own active_learning_func (tests/golden/active_*_d14.npz); structure (members, chunks, draws, freshness) is compared
with torch.equal: the same kernel on the same buffers, so a difference is an indexing defect, not rounding."""
import os

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from conftest import golden_params, load_golden
from ensemble_active_cases import L, LOOP, history_match, loop_data, loop_eps, oracle_loop
from oracle import vae_oracle as O
from vpc_amd import active as A
from vpc_amd import ensemble as E
from vpc_amd import ops

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 100}
DEV = "cuda"


def build(cls, d, reg_type="kl_reg", params=None):
    m = cls(d, 500, 10, L, TP, "exp", reg_type) if issubclass(cls, vpc.Reg_VAE) else cls(d, 500, 10, L, TP, "exp")
    if params is not None:
        sd = m.state_dict()
        for k, v in params.items():
            sd[k] = v.clone()
        m.load_state_dict(sd)
    return m.to(DEV)


def params_of(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if "prior" not in k}


def copy_of(m):
    """A fresh, unstacked model with m's current parameters."""
    return build(type(m), m.obs_dim, getattr(m, "reg_type", None), {k: v.detach().cpu() for k, v in m.state_dict().items()})


def rand_masks(G, n, d, seed, keep=0.4):
    """[G, n, d] bool, the target (last column) unobserved."""
    mk = torch.rand(G, n, d, generator=torch.Generator().manual_seed(seed)) < keep
    mk[:, :, -1] = False
    return mk


# ----------------------------------------------------------------------------------------------- 1. impute vs oracle
@pytest.mark.parametrize("d", [14, 20, 128])
def test_impute_vs_oracle(d):
    n, M, G = 21, 3, 3
    g = torch.Generator().manual_seed(d)
    plist = [O.init_params(d, L, seed=d + k) for k in range(G)]
    ms = [build(vpc.Reg_VAE, d, params=p) for p in plist]
    x = torch.rand(G, n, d, generator=g)
    mask = rand_masks(G, n, d, seed=d + 1, keep=0.6)
    eps = torch.randn(G, M * n, L, generator=g)
    acq = E.EnsembleAcquirer(ms)
    im = acq.impute(x.to(DEV), mask.to(DEV), M, 0, eps=eps.to(DEV))
    sq = acq.impute(x.to(DEV), mask.to(DEV), M, 1, eps=eps.to(DEV))
    assert tuple(im.shape) == (G, M, n, d) and tuple(sq.shape) == (G, M * n) and acq.launches == 1
    for k in range(G):
        port = O.TorchPort(plist[k], L)
        with torch.no_grad():
            z, _, _ = port.encoder(x[k].repeat(M, 1), mask[k].repeat(M, 1), eps=eps[k])
            want = port.decoder(z)[0].reshape(M, n, d)
        err = float((im[k].cpu() - want).abs().max())
        print("d", d, "member", k, "max |x_hat - oracle|", err)
        assert err <= 2e-5  # tests/test_gpu_parity.py's bound on x_mean_q
    # mode 1 is the squared target error of mode 0's output, exactly
    assert torch.equal(sq.view(G, M, n), (im[..., -1] - x.to(DEV)[:, None, :, -1]) ** 2)


# ----------------------------------------------------------------------------------------------- 2. impute indexing
@pytest.mark.parametrize("cls", [vpc.Reg_VAE, vpc.vanilla_VAE])
def test_impute_member_equals_its_stand_alone_call_bitwise(cls):
    d, n, M, G = 128, 21, 3, 9
    torch.manual_seed(7)
    ms = [build(cls, d) for _ in range(G)]
    twins = [copy_of(m) for m in ms]
    seeds = [3 + 5 * k for k in range(G)]
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(1)).to(DEV)
    mask = rand_masks(G, n, d, seed=2, keep=0.5).to(DEV)
    acq = E.EnsembleAcquirer(ms, seeds=seeds)
    im = acq.impute(x, mask, M, 0, max_blocks=9)  # device draws; one tile per launch: the chunk loop runs
    assert acq.launches == acq.tables(n, n, M)[0].tiles.shape[0] == 2 * M
    sq = acq.impute(x, mask, M, 1, max_blocks=9)
    assert torch.isfinite(im).all() and len({float(v) for v in im[:, 0, 0, 0]}) == G
    for k in range(G):
        alone = E.EnsembleAcquirer([twins[k]], seeds=[seeds[k]])
        assert torch.equal(alone.impute(x, mask[k:k + 1], M, 0)[0], im[k]), k
        assert torch.equal(alone.impute(x, mask[k:k + 1], M, 1)[0], sq[k]), k


def test_impute_draw_rule():
    d, n, M, G = 14, 21, 3, 2
    torch.manual_seed(1)
    ms = [build(vpc.Reg_VAE, d) for _ in range(G)]
    seeds = [5, 2 ** 40 + 6]
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(4)).to(DEV)
    mask = rand_masks(G, n, d, seed=3).to(DEV)
    R = M * n
    acq = E.EnsembleAcquirer(ms, seeds=seeds)
    first = acq.impute(x, mask, M, 0)
    assert acq.rng_offset == 4 * R
    second = acq.impute(x, mask, M, 0)  # two consecutive calls: the offset advance
    assert acq.rng_offset == 8 * R and not torch.equal(first, second)
    inj = E.EnsembleAcquirer(ms, seeds=seeds)
    for offset, want in ((0, first), (4 * R, second)):
        planes = torch.empty(G, R * 16, device=DEV)
        for k in range(G):
            ops.fill_normal(planes[k], seeds[k], offset)
        assert torch.equal(inj.impute(x, mask, M, 0, eps=planes.view(G, R, 16)[:, :, :L]), want), offset
    assert inj.rng_offset == 0  # injected eps consume no counters


# ----------------------------------------------------------------------------------------------- 3. reward
def _reward_case(d, n, M, seed):
    G = 3
    g = torch.Generator().manual_seed(seed)
    ms = [build(vpc.Reg_VAE, d, params=O.init_params(d, L, seed=seed + k)) for k in range(G)]
    x = torch.rand(G, n, d, generator=g)
    mask = rand_masks(G, n, d, seed=seed + 1)
    mask[1, 0, :d - 1] = True
    mask[1, 0, (d - 1) // 2] = False  # a row with a single unobserved candidate
    im = torch.rand(G, M, n, d, generator=g)
    return ms, x.to(DEV), mask.to(DEV), im.to(DEV)


@pytest.mark.parametrize("d,n,M", [(14, 5, 3), (14, 21, 17), (40, 21, 3), (40, 5, 17), (128, 21, 17), (128, 5, 3)])
def test_reward_multi_equals_reward_matrix_bitwise(d, n, M):
    ms, x, mask, im = _reward_case(d, n, M, seed=d + n + M)
    G = len(ms)
    acq = E.EnsembleAcquirer(ms)
    R = acq.reward(x, mask, im)
    assert acq.launches == 3
    sizes = ops.reward_scratch_multi(n, d, M)
    R2 = acq.reward(x, mask, im, ws_floats=2 * sum(sizes))  # two members fit: two member chunks
    assert acq.launches == 6
    assert int((R[1, 0] != -1e4).sum()) == 1
    for k in range(G):
        want = A.reward_matrix(ms[k], x[k], mask[k], im[k])
        assert torch.equal(R[k], want), k
        assert torch.equal(R2[k], want), k
    assert not torch.equal(R[0], R[1])


def test_reward_multi_vs_the_reference():
    gr, gv = load_golden("active_reg_d14.npz"), load_golden("active_van_d14.npz")
    d, M, n = 14, int(gr["M"]), gr["x"].shape[0]
    pr, pv = golden_params(gr), golden_params(gv)
    noise = torch.Generator().manual_seed(0)
    pm = {k: v + 0.01 * torch.randn(v.shape, generator=noise) for k, v in pr.items()}  # member 1: a perturbed copy
    ms = [build(vpc.Reg_VAE, d, params=p) for p in (pr, pm, pv)]
    acq = E.EnsembleAcquirer(ms)
    x = torch.from_numpy(gr["x"]).to(DEV)
    for t in (0, 3, d - 2):
        masks, ims = [], []
        for g in (gr, gr, gv):
            mk = torch.zeros(n, d, dtype=torch.bool)
            for s in range(t):  # the mask rebuilt from the golden's action history
                mk[torch.arange(n), torch.from_numpy(g["action"][:, s].astype(np.int64))] = True
            masks.append(mk)
            ims.append(torch.from_numpy(g["im"][t]))
        R = acq.reward(x, torch.stack(masks).to(DEV), torch.stack(ims).to(DEV)).cpu().numpy()
        for k, g in ((0, gr), (2, gv)):
            want = g["R_hist"][t]
            tol = 5e-7 + 1e-3 * np.max(np.abs(g["R_hist"][g["R_hist"] != -1e4]))  # test_gpu_loop_matches_reference's
            assert np.array_equal(R[k] == -1e4, want == -1e4), (t, k)
            err = np.max(np.abs(R[k] - want))
            print("step", t, "member", k, "max |R - reference|", err, "tol", tol)
            assert err <= tol, (t, k)


# ----------------------------------------------------------------------------------------------- 4. acquire, target MSE
def test_acquire():
    G, n, d = 3, 21, 14
    g = torch.Generator().manual_seed(0)
    R = torch.rand(G, n, d - 1, generator=g)
    best = torch.randint(0, d - 1, (G, n), generator=g)
    R.scatter_(2, best[..., None], 2.0)  # a unique maximum per row
    R[0, 0] = -1e4
    R[0, 0, [4, 9]] = 0.25     # a tie: the lowest index
    R[1, 1] = 0.5              # all equal: index 0
    best[0, 0], best[1, 1] = 4, 0
    assert torch.equal(R.argmax(2), best)
    seen = torch.rand(G, n, d, generator=g) < 0.3
    mask = seen.to(torch.uint8).to(DEV)
    maskk = torch.zeros(G, n, 16, dtype=torch.uint8, device=DEV)
    maskk[:, :, :d] = mask
    action = torch.full((G, 2, n, d - 1), -1, dtype=torch.int32, device=DEV)
    Rd = R.to(DEV)
    ops.acquire_multi(Rd, Rd.stride(0), mask, mask.stride(0), d, maskk, maskk.stride(0), 16, action[0, 1, :, 5:], action.stride(0),
                      d - 1, G, n, d)
    want_mask = (seen | (torch.eye(d)[best] > 0)).to(torch.uint8)
    assert torch.equal(mask.cpu(), want_mask)
    assert torch.equal(maskk[:, :, :d].cpu(), want_mask) and not maskk[:, :, d:].any()
    assert torch.equal(action[:, 1, :, 5].cpu(), best.to(torch.int32))
    action[:, 1, :, 5] = -1
    assert (action == -1).all()  # nothing but the step's slot was written


def test_target_mse():
    G, R = 3, 63
    sq = torch.rand(G, 80, generator=torch.Generator().manual_seed(0)) * torch.tensor([1.0, 1e-3, 50.0])[:, None]
    out = torch.full((G, 2, 5), -1.0, device=DEV)
    sqd = sq.to(DEV)
    ops.target_mse_multi(sqd, sqd.stride(0), R, G, out[0, 1, 3:], out.stride(0))
    want = sq[:, :R].double().mean(1)
    got = out[:, 1, 3].cpu().double()
    print("target mse rel", ((got - want).abs() / want).tolist())
    assert torch.all((got - want).abs() <= 1e-6 * want)
    out[:, 1, 3] = -1.0
    assert (out == -1.0).all()


# ----------------------------------------------------------------------------------------------- 5. the loop vs the oracle
def test_loop_vs_oracle():
    d, n, M, steps = LOOP["d"], LOOP["n"], LOOP["M"], LOOP["steps"]
    x, xt, mt = loop_data()
    torch.manual_seed(3)
    m0 = build(vpc.Reg_VAE, d)
    tr = vpc.FusedTrainer(m0)
    xt, mt = xt.to(DEV), mt.to(DEV)
    for i in range(200):  # a briefly trained model: rewards of a random-init encoder are all round-off
        tr.step(xt, mt, alpha=1.0, epoch=i + 1)
    p0 = params_of(m0)
    for i in range(100):  # member 1: a further-trained copy
        tr.step(xt, mt, alpha=1.0, epoch=201 + i)
    p1 = params_of(m0)
    ms = [build(vpc.Reg_VAE, d, params=p0), build(vpc.Reg_VAE, d, params=p1)]
    eps = loop_eps(2)
    acq = E.EnsembleAcquirer(ms)
    info, action, R_hist, im_hist = [t.cpu().numpy() for t in acq.run(x.to(DEV), M, max_steps=steps, eps=eps.to(DEV))]
    assert info.shape == (2, 1, d) and action.shape == (2, 1, n, d - 1) and R_hist.shape == (2, 1, d - 1, n, d - 1)
    assert im_hist.shape == (2, 1, d - 1, M, n, d)
    assert not info[:, :, steps + 1:].any() and not action[:, :, :, steps:].any() and not R_hist[:, :, steps:].any()
    assert acq.launches == 2 + steps * 7 and acq.launches_per_step == 7
    for k, p in enumerate((p0, p1)):
        ref = oracle_loop(O.TorchPort(p, L), x, eps[k], M, steps)
        want, act_ref = ref["R_hist"].numpy(), ref["action"].numpy().astype(np.int64)
        act = action[k, 0, :, :steps].astype(np.int64)
        live = want != -1e4
        scale = np.max(np.abs(want[live]))
        tol = 1e-4 * scale + 5e-7
        same = history_match(act, act_ref)
        print("member", k, "scale", scale, "rows with the oracle's history per step", same.mean(1).tolist())
        assert scale > 1e-3  # the trained encoder does discriminate between candidates
        assert np.all(same.mean(1) >= 0.9)
        for t in range(steps):
            rows = same[t]
            R = R_hist[k, 0, t]
            assert np.array_equal(R[rows] == -1e4, want[t][rows] == -1e4), (k, t)
            err = np.max(np.abs(R[rows] - want[t][rows]))
            print("member", k, "step", t, "max |R - oracle|", err, "tol", tol)
            assert err <= tol, (k, t, err, tol)
            # the picked feature is the oracle's, or one within that tolerance of its best
            gap = want[t][rows].max(1) - want[t][rows][np.arange(rows.sum()), act[rows, t]]
            assert np.all(gap <= tol), (k, t, gap.max())
            assert np.max(np.abs(im_hist[k, 0, t][:, rows] - ref["im"].numpy()[t][:, rows])) <= 2e-5
        # the curve: a mean of (x_hat - x)^2 with |d x_hat| <= 2e-5 (the forward bound) moves by at most 2 * 2e-5 * |x_hat - x| + 4e-10,
        # |x_hat - x| <= 1; rows that left the oracle's history are bounded by their share, so the curve is compared while all rows match
        want_c = ref["info_curve"].numpy()
        for t in range(steps + 1):
            if same[t].all():
                assert abs(info[k, 0, t] - want_c[t]) <= 1e-5 * abs(want_c[t]) + 1e-7 + 4e-5, (k, t, info[k, 0, t], want_c[t])


# ----------------------------------------------------------------------------------------------- 6. device draws
def test_loop_properties_with_device_draws():
    d, n, M, G, rep = 14, 24, 25, 4, 2
    gold = load_golden("active_reg_d14.npz")
    pr = golden_params(gold)
    noise = torch.Generator().manual_seed(1)
    plist = [pr] + [{k: v + 0.005 * torch.randn(v.shape, generator=noise) for k, v in pr.items()} for _ in range(G - 1)]
    ms = [build(vpc.Reg_VAE, d, params=p) for p in plist]
    x = torch.from_numpy(gold["x"]).to(DEV)
    seeds = [11, 12, 13, 14]
    acq = E.EnsembleAcquirer(ms, seeds=seeds)
    info, action, R_hist, im_hist = acq.run(x, M, repeats=rep)
    calls = rep * (1 + 2 * (d - 1))
    assert acq.rng_offset == calls * 4 * M * n
    act = action.cpu().numpy()
    for k in range(G):
        for r in range(rep):
            for row in act[k, r]:
                assert sorted(row) == list(range(d - 1))  # every row acquires d - 1 distinct features
    curve = info.cpu().numpy()
    assert np.all(curve[:, :, -1] < 0.5 * curve[:, :, 0])  # the curve ends below half its start
    assert not torch.equal(info[:, 0], info[:, 1]) and not torch.equal(im_hist[:, 0], im_hist[:, 1])  # two repeats differ
    # the same seeds reproduce the run bit for bit in a fresh acquirer; keep_im=False gives the same info / action / R_hist
    again = E.EnsembleAcquirer([copy_of(m) for m in ms], seeds=seeds)
    i2, a2, R2, im2 = again.run(x, M, repeats=rep, keep_im=False)
    assert im2 is None
    assert torch.equal(i2, info) and torch.equal(a2, action) and torch.equal(R2, R_hist)
    i3, a3, R3, im3 = E.EnsembleAcquirer(ms, seeds=seeds).run(x, M, repeats=rep)
    assert torch.equal(i3, info) and torch.equal(a3, action) and torch.equal(R3, R_hist) and torch.equal(im3, im_hist)


# ----------------------------------------------------------------------------------------------- 7. freshness
def test_run_reads_the_current_weights():
    d, n, M, G = 14, 21, 3, 2
    torch.manual_seed(2)
    ms = [build(vpc.Reg_VAE, d) for _ in range(G)]
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(9)).to(DEV)
    eps = torch.randn(1 + 2 * 4, M * n, L, generator=torch.Generator().manual_seed(3)).to(DEV)
    run = lambda a: a.run(x, M, max_steps=4, eps=eps, keep_im=False)[:3]
    acq = E.EnsembleAcquirer(ms)
    r0 = run(acq)
    ms[0].load_state_dict({k: v.detach().clone() for k, v in ms[1].state_dict().items()})  # in place
    r1 = run(acq)
    assert not torch.equal(r0[0][0], r1[0][0]) and torch.equal(r0[0][1], r1[0][1])
    for a, b in zip(r1, r1):
        assert torch.equal(a[0], b[1])  # member 0 now computes what member 1 computes
    fresh = run(E.EnsembleAcquirer([copy_of(m) for m in ms]))
    for a, b in zip(r1, fresh):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------- 8. active_sweep
def test_active_sweep(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    d, n, M, rep = 14, 21, 3, 2
    torch.manual_seed(6)
    ms = [build(vpc.Reg_VAE, d), build(vpc.Reg_VAE, d), build(vpc.Reg_VAE_mask, d)]
    cfgs = [dict(vae_type="reg_vae1", alpha=0.5, seed=11), dict(vae_type="reg_vae2", alpha=0.8, p_missingness=50, seed=13),
            dict(vae_type="reg_vae1_mask_augm", alpha=0.5, seed=14)]
    g = torch.Generator().manual_seed(8)
    x, tmask = torch.rand(n, d, generator=g), torch.rand(n, d, generator=g) < 0.7
    # (active_learning_func reloads the checkpoint from the second repeat on, as the reference does)
    ck = vpc.checkpoint_path("exp", "uci", "reg_vae1_mask_augm", 30, alpha=0.5, p_missingness=30, reg_type="kl_reg")
    os.makedirs(os.path.dirname(ck), exist_ok=True)
    torch.save({k: v.detach().cpu() for k, v in ms[2].state_dict().items()}, ck)
    out = vpc.active_sweep(None, cfgs, x, tmask, 30, d, 500, 10, M, L, "uci", TP, "exp", 7, 1, 1, reg_type="kl_reg", Repeat=rep,
                           models=ms, save=True, max_steps=4)
    assert len(out) == 3
    shapes = dict(information_curve_CHAI=(rep, n, d), action_CHAI=(rep, n, d - 1), R_hist_CHAI=(rep, d - 1, n, d - 1),
                  im_CHAI=(rep, d - 1, M, n, d))
    for k, c in enumerate(cfgs):  # the four files of every member, under its own alpha / p_missingness, hold what is returned
        paths = A.active_result_paths("exp", "uci", c["vae_type"], 30, c["alpha"], c.get("p_missingness", 30), "kl_reg")
        assert set(out[k]) == set(paths) == set(shapes)
        for name, pth in paths.items():
            assert os.path.exists(pth), pth
            assert tuple(out[k][name].shape) == shapes[name] and out[k][name].dtype == torch.float32
            assert torch.equal(torch.load(pth, weights_only=True), out[k][name]), (k, name)
    # the stackable members ran together: what a two-member acquirer with their seeds gives
    acq = E.EnsembleAcquirer(ms[:2], seeds=[11, 13])
    info, action, R_hist, im_hist = [t.cpu() for t in acq.run(x.to(DEV), M, repeats=rep, max_steps=4)]
    for k in range(2):
        assert torch.equal(out[k]["information_curve_CHAI"], info[k][:, None, :].expand(rep, n, d))
        assert torch.equal(out[k]["action_CHAI"], action[k].float()) and torch.equal(out[k]["R_hist_CHAI"], R_hist[k])
        assert torch.equal(out[k]["im_CHAI"], im_hist[k])
        assert out[k]["information_curve_CHAI"][:, :, :5].min() > 0 and not out[k]["information_curve_CHAI"][:, :, 5:].any()
    # the mask-augmented member went alone through active_learning_func: its rewards mark the observed features its own way
    assert (out[2]["R_hist_CHAI"][:, 1] == -1e4).sum() == rep * n
