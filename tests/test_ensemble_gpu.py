"""The ensemble step (ensemble.EnsembleTrainer: vpc_step_small_multi_f32 + vpc_reduce_step_adam_multi) on the MI355X.

A "twin" of member g is a stand-alone FusedTrainer with the member's initial parameters, seed, lr and hyperparameters, fed the
member's data.  The ensemble kernels run the single-model kernels' bodies on member g's buffers, so a member and its twin are
compared with torch.equal: any difference is an indexing defect, not rounding."""
import copy
import os

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from conftest import golden_params, load_golden
from oracle import vae_oracle as O
from vpc_amd import ensemble as E
from vpc_amd import ops

pytestmark = pytest.mark.gpu
L = 10
TP = {"batch_size": 64, "patience": 100}
DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def build(cls, d, reg_type="kl_reg", params=None):
    m = cls(d, 500, 10, L, TP, "exp", reg_type) if cls is vpc.Reg_VAE else cls(d, 500, 10, L, TP, "exp")
    if params is not None:
        sd = m.state_dict()
        for k, v in params.items():
            sd[k] = v.clone()
        m.load_state_dict(sd)
    return m


def members_and_twins(cls, d, G, reg_type="kl_reg", seed=0, params=None):
    """G freshly initialised models (or G copies of `params`) and a deep copy of each, all on the GPU."""
    torch.manual_seed(seed)
    ms = [build(cls, d, reg_type, params) for _ in range(G)]
    twins = [copy.deepcopy(m) for m in ms]
    return [m.to(DEV) for m in ms], [m.to(DEV) for m in twins]


def data(G, B, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(G, B, d, generator=g)
    mask = torch.rand(G, B, d, generator=g) < 0.7
    return x.to(DEV), mask.to(DEV)


def need_rows(B):
    if ops.step_small_max_rows() < B:
        pytest.skip("the twin would run other kernels at this batch size")


def assert_member_equals_twin(ens, g, tw, what=""):
    v = ens.trainers[g]
    assert torch.equal(ens.params[g], tw.model.flatten_parameters()), (what, g, "params")
    assert torch.equal(v.exp_avg, tw.exp_avg), (what, g, "exp_avg")
    assert torch.equal(v.exp_avg_sq, tw.exp_avg_sq), (what, g, "exp_avg_sq")
    assert torch.equal(v.grad, tw.grad), (what, g, "grad")
    assert torch.equal(v.out9, tw.out9), (what, g, "out9")


# ----------------------------------------------------------------------------------------------- 1. members == twins
CASES = {
    # three tiles, the last one 5 rows; d padded 14 -> 16; everything per member
    "kl_d14": dict(cls="reg", rt="kl_reg", d=14, B=37, G=3, seeds=(1, 2, 3), alpha=(1.0, 0.5, 0.8), pm=(30, 50, 10),
                   lr=(1e-3, 1e-3, 3e-4), epoch=1, shared=False),
    # wml != 0: the third eps plane; one batch shared by the members
    "ml_d40": dict(cls="reg", rt="ml_reg", d=40, B=16, G=2, seeds=(5, 6), alpha=(0.5, 0.9), pm=(30, 30), lr=(1e-3, 1e-3),
                   epoch=1400, shared=True),
    "van_d128": dict(cls="van", rt=None, d=128, B=64, G=2, seeds=(7, 8), alpha=(1.0, 1.0), pm=(30, 30), lr=(1e-3, 2e-3),
                     epoch=1, shared=False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_members_equal_their_twins_bitwise(name):
    c = CASES[name]
    need_rows(c["B"])
    cls = vpc.Reg_VAE if c["cls"] == "reg" else vpc.vanilla_VAE
    G, B, d = c["G"], c["B"], c["d"]
    ms, tms = members_and_twins(cls, d, G, c["rt"], seed=11)
    ens = E.EnsembleTrainer(ms, lr=c["lr"], seeds=c["seeds"])
    twins = [vpc.FusedTrainer(tms[g], lr=c["lr"][g], seed=c["seeds"][g]) for g in range(G)]
    for step in range(4):
        x, mask = data(1 if c["shared"] else G, B, d, seed=100 + step)
        if c["shared"]:
            ens.step(x[0], mask[0], epoch=c["epoch"], alpha=c["alpha"], p_missingness=c["pm"])
        else:
            ens.step(x, mask, epoch=c["epoch"], alpha=c["alpha"], p_missingness=c["pm"])
        for g, tw in enumerate(twins):
            xg, mg = (x[0], mask[0]) if c["shared"] else (x[g], mask[g])
            tw.step(xg, mg, epoch=c["epoch"], alpha=c["alpha"][g], p_missingness=c["pm"][g])
            assert tw.dominant_launch() == "step_small"
            assert_member_equals_twin(ens, g, tw, f"step {step}")
        assert ens.rng_offset == twins[0].rng_offset and ens.step_count == twins[0].step_count
    assert np.isfinite(ens.loss_values()).all()
    if G > 1 and not c["shared"]:  # the members really are different runs
        assert not torch.equal(ens.params[0], ens.params[1])


# ----------------------------------------------------------------------------------------------- 2. reference trajectory
@pytest.mark.parametrize("kind", ["reg", "vanilla"])
def test_members_follow_the_golden_trajectory(kind):
    """Members 0 and 1 start from the golden's param0 and are fed its injected mask_p / eps: each reproduces the golden losses
    and paramT at the bounds of test_fused_adam_trajectory_matches_golden (3e-5 relative on every loss and on the epoch total,
    1e-4 of the tensor's maximum on every final parameter).  The last member has other hyperparameters: it differs from them
    and equals its own twin.  vanilla_VAE's loss has no alpha (VAE.py:1183-1195): there member 2 (alpha 0.5) must STILL follow
    the golden, and it is member 3, with beta 0.5, that differs."""
    g = load_golden(f"traj_{kind}_d14.npz")
    cls = vpc.Reg_VAE if kind == "reg" else vpc.vanilla_VAE
    G = 3 if kind == "reg" else 4
    alphas = (1.0, 1.0, 0.5) if kind == "reg" else (1.0, 1.0, 0.5, 1.0)
    betas = (1.0, 1.0, 1.0) if kind == "reg" else (1.0, 1.0, 1.0, 0.5)
    ms, tms = members_and_twins(cls, 14, G, params=golden_params(g, "param0."))
    ens = E.EnsembleTrainer(ms, lr=1e-3)
    tw = vpc.FusedTrainer(tms[-1], lr=1e-3)
    x, mk = _t(g["x"]), _t(g["mask"])
    follow = range(G - 1)
    for i in range(len(g["loss"])):
        if kind == "reg":
            inj = (_t(g["mask_p"][i]), _t(g["eps_q"][i]), _t(g["eps_p"][i]))
            ens.step(x, mk, *inj, epoch=i + 1, alpha=alphas, beta=betas)
            tw.step(x, mk, *inj, epoch=i + 1, alpha=alphas[-1], beta=betas[-1])
        else:
            ens.step(x, mk, eps_q=_t(g["eps_q"][i]), epoch=i + 1, alpha=alphas, beta=betas)
            tw.step(x, mk, eps_q=_t(g["eps_q"][i]), epoch=i + 1, alpha=alphas[-1], beta=betas[-1])
        losses = ens.loss_values()
        for m in follow:
            assert abs(losses[m] - g["loss"][i]) <= 3e-5 * abs(g["loss"][i]), (i, m)
        assert_member_equals_twin(ens, G - 1, tw, f"step {i}")
    totals = ens.epoch_total()
    pT = golden_params(g, "paramT.")
    for m in follow:
        assert abs(totals[m] - g["loss"].sum()) <= 3e-5 * g["loss"].sum()
        for k, p in zip(O.PARAM_KEYS, ms[m].trainable()):
            assert rel(p.detach().cpu().numpy(), pT[k].numpy()) < 1e-4, (m, k)
        assert torch.equal(ens.params[m], ens.params[0])  # same start, same inputs: the same run
    assert not torch.equal(ens.params[G - 1], ens.params[0])
    assert ens.rng_offset == 0  # injected draws consume no counters, as in FusedTrainer.step


# ----------------------------------------------------------------------------------------------- 3. more workgroups than CUs
def test_more_workgroups_than_cus_and_members_do_not_leak():
    """G = 80 at B = 64 is 320 workgroups.  Members 0, 41 and 79 equal their twins; a second ensemble from the same start, in
    the OTHER workgroup order and with member 17's inputs altered, differs from the first in row 17 of every stack and nowhere
    else (which also shows the two workgroup orders to give the same bits)."""
    G, B, d, alt = 80, 64, 128, 17
    need_rows(B)
    torch.manual_seed(3)
    base = [build(vpc.Reg_VAE, d) for _ in range(G)]
    ms_a = [copy.deepcopy(m).to(DEV) for m in base]
    ms_b = [copy.deepcopy(m).to(DEV) for m in base]
    picks = (0, 41, 79)
    seeds = list(range(100, 100 + G))
    alphas = [0.3 + 0.005 * g for g in range(G)]
    x, mask = data(G, B, d, seed=9)
    a = E.EnsembleTrainer(ms_a, seeds=seeds)
    b = E.EnsembleTrainer(ms_b, seeds=seeds)
    b.order = 1 - a.order
    a.step(x, mask, alpha=alphas)
    for g in picks:
        tw = vpc.FusedTrainer(base[g].to(DEV), seed=seeds[g])
        tw.step(x[g], mask[g], alpha=alphas[g])
        assert_member_equals_twin(a, g, tw)
    x2 = x.clone()
    x2[alt] = 1.0 - x2[alt]
    b.step(x2, mask, alpha=alphas)
    others = [g for g in range(G) if g != alt]
    for name in ("params", "grad", "exp_avg", "exp_avg_sq", "out9", "accum", "img"):
        sa, sb = getattr(a, name), getattr(b, name)
        assert torch.equal(sa[others], sb[others]), name
        assert not torch.equal(sa[alt], sb[alt]), name


# ----------------------------------------------------------------------------------------------- 4. images are fresh
def test_api_path_reads_fresh_images_after_ensemble_steps():
    G, B, d = 3, 24, 14
    need_rows(B)
    ms, tms = members_and_twins(vpc.Reg_VAE, d, G, seed=5)
    ens = E.EnsembleTrainer(ms, seeds=(4, 5, 6))
    tw = vpc.FusedTrainer(tms[1], seed=5)
    x, mask = data(G, B, d, seed=2)
    for _ in range(2):
        ens.step(x, mask, alpha=0.8)
        tw.step(x[1], mask[1], alpha=0.8)
    with torch.no_grad():
        _, mean, logvar = ms[1].encoder(x[1], mask[1], sample=False)
        _, mean_t, logvar_t = tms[1].encoder(x[1], mask[1], sample=False)
        xhat, _ = ms[1].decoder(mean)
        xhat_t, _ = tms[1].decoder(mean_t)
    assert torch.equal(mean, mean_t) and torch.equal(logvar, logvar_t) and torch.equal(xhat, xhat_t)
    # and the image the API path read is the ensemble's row, stamped fresh by the step (no re-pack happened)
    assert ms[1]._img.buf.data_ptr() == ens.img[1].data_ptr()
    assert ms[1]._img.key == ms[1]._param_key()
    # a write torch counts makes member 2's image stale: the next step re-packs that member alone, and everybody goes on
    with torch.no_grad():
        ms[2].seq_encoder[0].bias.mul_(0.5)
    assert ms[2]._img.key != ms[2]._param_key()
    ens.step(x, mask, alpha=0.8)
    tw.step(x[1], mask[1], alpha=0.8)
    assert torch.equal(ens.params[1], tms[1].flatten_parameters())
    fresh = build(vpc.Reg_VAE, d, params={k: v.detach().cpu() for k, v in ms[2].state_dict().items()}).to(DEV)
    with torch.no_grad():
        _, mean, _ = ms[2].encoder(x[2], mask[2], sample=False)
        _, mean_f, _ = fresh.encoder(x[2], mask[2], sample=False)
    assert torch.equal(mean, mean_f)


# ----------------------------------------------------------------------------------------------- 5. epoch total
def test_epoch_total_per_member():
    G, B, d = 2, 16, 14
    need_rows(B)
    ms, tms = members_and_twins(vpc.vanilla_VAE, d, G, seed=8)
    ens = E.EnsembleTrainer(ms, seeds=(1, 2))
    twins = [vpc.FusedTrainer(tms[g], seed=g + 1) for g in range(G)]
    for s in range(3):
        x, mask = data(G, B, d, seed=s)
        ens.step(x, mask)
        for g in range(G):
            twins[g].step(x[g], mask[g])
    assert ens.epoch_total(reset=False) == [tw.epoch_total(reset=False) for tw in twins]
    tot = ens.epoch_total()
    assert tot == [tw.epoch_total() for tw in twins] and len(tot) == G and all(t > 0 for t in tot)
    assert ens.epoch_total() == [0.0] * G


# ----------------------------------------------------------------------------------------------- 6. harness.train_sweep
def test_train_sweep_equals_train_member_by_member(tmp_path, monkeypatch):
    d, epochs = 14, 2
    need_rows(16)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(39, d, generator=g)
    mask = torch.rand(39, d, generator=g) < 0.7
    loader = [(x[0:16], mask[0:16]), (x[16:32], mask[16:32]), (x[32:39], mask[32:39])]
    cfgs = [dict(vae_type="reg_vae1", alpha=1.0, p_missingness=30, seed=3),
            dict(vae_type="reg_vae1", alpha=0.5, p_missingness=30, seed=4)]
    torch.manual_seed(1)
    base = [build(vpc.Reg_VAE, d) for _ in cfgs]
    args = (30, d, 500, 10, 1, L, "synth", TP, "exp")
    (tmp_path / "sweep").mkdir()
    (tmp_path / "solo").mkdir()
    monkeypatch.chdir(tmp_path / "sweep")
    out = vpc.train_sweep((loader, None), cfgs, *args, 20, 10, max_epochs=epochs, device=torch.device(DEV), reg_type="kl_reg",
                          verbose=False, models=[copy.deepcopy(m) for m in base])
    assert len(out) == 2
    for c, m0 in zip(cfgs, base):
        path = vpc.checkpoint_path("exp", "synth", c["vae_type"], 30, c["alpha"], c["p_missingness"], "kl_reg")
        monkeypatch.chdir(tmp_path / "sweep")
        assert os.path.exists(path)
        loaded = vpc.model_loader("test", d, 500, 10, L, 30, "synth", TP, epochs, 20, 10, "exp", "kl_reg", c["vae_type"],
                                  alpha=c["alpha"], p_missingness=c["p_missingness"])
        monkeypatch.chdir(tmp_path / "solo")
        vpc.train((loader, None), *args, c["vae_type"], 20, 10, max_epochs=epochs, device=torch.device(DEV), alpha=c["alpha"],
                  p_missingness=c["p_missingness"], reg_type="kl_reg", seed=c["seed"], verbose=False, model=copy.deepcopy(m0))
        solo = torch.load(path, map_location="cpu", weights_only=True)
        sd = loaded.state_dict()
        assert list(sd) == list(solo)
        for k in solo:
            assert torch.equal(sd[k], solo[k]), (c["alpha"], k)
        assert not torch.equal(sd["seq_encoder.0.weight"], m0.state_dict()["seq_encoder.0.weight"])  # it trained
    # per-member loaders (different splits): same result as the shared loader when they hold the same batches ...
    monkeypatch.chdir(tmp_path / "sweep")
    out2 = vpc.train_sweep(None, cfgs, *args, 20, 10, max_epochs=epochs, device=torch.device(DEV), reg_type="kl_reg",
                           verbose=False, save=False, models=[copy.deepcopy(m) for m in base],
                           loaders=[(loader, None), (list(loader), None)])
    for a, b in zip(out, out2):
        assert torch.equal(a.flatten_parameters(), b.flatten_parameters())
    # ... and loaders of unequal length, or unequal batch shapes, are refused
    with pytest.raises(vpc.VpcError, match="same number of batches"):
        vpc.train_sweep(None, cfgs, *args, 20, 10, max_epochs=1, device=torch.device(DEV), reg_type="kl_reg", verbose=False,
                        save=False, models=[copy.deepcopy(m) for m in base], loaders=[(loader, None), (loader[:2], None)])
    with pytest.raises(vpc.VpcError, match="equal batch shapes"):
        vpc.train_sweep(None, cfgs, *args, 20, 10, max_epochs=1, device=torch.device(DEV), reg_type="kl_reg", verbose=False,
                        save=False, models=[copy.deepcopy(m) for m in base],
                        loaders=[(loader, None), ([loader[0], loader[2], loader[1]], None)])


def test_train_sweep_splits_a_mixed_list(tmp_path, monkeypatch):
    """Two classes and a family outside the ensemble's scope in one list: every member is trained and saved."""
    monkeypatch.chdir(tmp_path)
    d = 14
    need_rows(16)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(32, d, generator=g)
    mask = torch.rand(32, d, generator=g) < 0.7
    loader = [(x[0:16], mask[0:16]), (x[16:32], mask[16:32])]
    cfgs = [dict(vae_type="reg_vae1", alpha=0.5), dict(vae_type="vanilla_vae1"), dict(vae_type="reg_vae2", alpha=0.8),
            dict(vae_type="reg_vae_mask_augm1", alpha=0.5)]
    torch.manual_seed(2)
    out = vpc.train_sweep((loader, None), cfgs, 30, d, 500, 10, 1, L, "synth", TP, "exp", 20, 10, max_epochs=1,
                          device=torch.device(DEV), reg_type="kl_reg", verbose=False)
    assert [type(m) for m in out] == [vpc.Reg_VAE, vpc.vanilla_VAE, vpc.Reg_VAE, vpc.Reg_VAE_mask]
    for c in cfgs:
        assert os.path.exists(vpc.checkpoint_path("exp", "synth", c["vae_type"], 30, c.get("alpha", 1.0), 30, "kl_reg"))
    assert out[0].__dict__["_stack"][0] is out[2].__dict__["_stack"][0]  # the two Reg_VAE members shared one ensemble


# ----------------------------------------------------------------------------------------------- 7. limits
def test_limits_raise_instead_of_launching():
    rows = ops.step_small_max_rows()
    if rows < 16:
        pytest.skip("the small-batch step is switched off")
    torch.manual_seed(0)
    ms = [build(vpc.vanilla_VAE, 4).to(DEV) for _ in range(2)]
    ens = E.EnsembleTrainer(ms)
    B = rows + 1
    with pytest.raises(vpc.VpcError, match="rows"):
        ens.step(torch.rand(B, 4, device=DEV), torch.ones(B, 4, dtype=torch.bool, device=DEV))
    # G x tiles beyond VPC_MULTI_MAX_BLOCKS (include/vpc.h)
    tiles = (rows + 15) // 16
    G = E.MAX_BLOCKS // tiles + 1
    if G <= 64:
        big = E.EnsembleTrainer([build(vpc.vanilla_VAE, 4).to(DEV) for _ in range(G)])
        with pytest.raises(vpc.VpcError, match="workgroups"):
            big.step(torch.rand(rows, 4, device=DEV), torch.ones(rows, 4, dtype=torch.bool, device=DEV))
    # the C entry point refuses what the kernel does not cover (nothing is launched): d % 4 != 0, d > 128, L > 15, a member
    # stride that does not hold the member's blocks, and more workgroups than the bound
    x, mask = torch.rand(2, 16, 8, device=DEV), torch.ones(2, 16, 8, dtype=torch.uint8, device=DEV)
    ens.step(x[:, :, :4].contiguous(), mask[:, :, :4].contiguous())  # (allocates the workspaces used below)
    lay = ens.lay
    good = [16 * 4, 16 * 4, 0, ens.eps_buf.stride(0), ens.img.stride(0), ens.partE.stride(0), ens.partD.stride(0),
            ens.loss_part.stride(0), ens.row_pitch]

    def call(strides=good, G=2, B=16, d=4, Ld=L):
        ops.step_small_multi_f32(x, mask, None, ens.eps_buf, ens.img[0, :lay.enc_img], ens.img[0, lay.enc_img:], ens.table_dev,
                                 G, 1, 1, 0, 0, 0, 1.0 / B, 0.0, ens.partE, ens.partD, ens.loss_part, strides, B, d, Ld)

    for kw in (dict(d=6), dict(d=132), dict(Ld=16), dict(G=E.MAX_BLOCKS + 1)):
        with pytest.raises(vpc.VpcError, match="unsupported shape"):
            call(**kw)
    short = list(good)
    short[5] = lay.enc_part - 4
    with pytest.raises(vpc.VpcError, match="bad argument"):
        call(strides=short)
    torch.cuda.synchronize()
