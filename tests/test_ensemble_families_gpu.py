"""The ensemble step of the mask-augmented and point-net members on the MI355X (ensemble.MaskEnsembleTrainer: vpc_step_small_multi_aug_f32
+ vpc_reduce_step_adam_multi; ensemble.EDDIEnsembleTrainer: vpc_step_small_multi_eddi_f32 + vpc_reduce_step_adam_eddi_multi).

A member's TWIN is the stand-alone FusedTrainer / EDDITrainer with the member's initial parameters, seed, learning rate and
hyperparameters on the member's data, on its small-batch path.  The comparison with the twin is torch.equal on the flat
parameters, both Adam moments, the gradient and the nine loss terms after every step - the kernels run one tile body and one set
of reduction bodies - and equality of rng_offset and step_count.  The anchors that do not go through the twin (vectors and
trajectories captured from the reference) use the bounds of the stand-alone tests: tests/test_eddi_small_gpu.py (losses 1e-4,
final parameters 5e-5) and tests/test_small_augm_gpu.py (loss 2e-5, every gradient tensor 2e-4 of its maximum)."""
import copy
import os

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from conftest import load_golden
from oracle import vae_oracle as O
from vpc_amd import ensemble as E
from vpc_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
L = 10
TP = {"batch_size": 64, "patience": 1}
STEPS = 4


def need_rows(B):
    if ops.step_small_max_rows() < B:
        pytest.skip(f"the small-batch step is off for {B} rows (VPC_STEP_SMALL / VPC_TILE)")


def build(family, kind, d, K=10, reg_type="kl_reg"):
    if family == "mask":
        m = vpc.Reg_VAE_mask(d, 500, 10, L, TP, "e", reg_type) if kind == "reg" else vpc.vanilla_VAE_mask(d, 500, 10, L, TP, "e")
    else:
        m = vpc.Reg_EDDI(d, 500, K, L, TP, "e", reg_type) if kind == "reg" else vpc.vanilla_EDDI(d, 500, K, L, TP, "e")
    return m


def data(G, B, d, seed, shared=False):
    g = torch.Generator().manual_seed(seed)
    shape = (B, d) if shared else (G, B, d)
    return torch.rand(*shape, generator=g).to(DEV), (torch.rand(*shape, generator=g) < 0.7).to(DEV)


def injected(G, B, d, mask, seed, planes):
    g = torch.Generator().manual_seed(seed)
    mask_p = mask & (torch.rand(G, B, d, generator=g) < 0.7).to(DEV)
    return mask_p, [torch.randn(G, B, L, generator=g).to(DEV) for _ in range(planes)]


def twin_of(family, model, lr, seed):
    cls = vpc.FusedTrainer if family == "mask" else vpc.EDDITrainer
    return cls(model, lr=lr, seed=seed)


def on_small_path(family, tw):
    return tw.dominant_launch() == "step_small" if family == "mask" else tw.last_path == "small"


def state_of(ens, g):
    return [t.clone() for t in (ens.params[g], ens.exp_avg[g], ens.exp_avg_sq[g], ens.grad[g], ens.out9[g])]


def assert_member_equals_twin(ens, g, tw, what):
    names = ("params", "exp_avg", "exp_avg_sq", "grad", "out9")
    theirs = (tw.model._flat, tw.exp_avg, tw.exp_avg_sq, tw.grad, tw.out9)
    for n, a, b in zip(names, state_of(ens, g), theirs):
        assert a.shape == b.shape, (what, n, a.shape, b.shape)
        assert bool(torch.isfinite(a).all()), (what, n)
        assert torch.equal(a, b), (what, n, float((a - b).abs().max()))
    assert ens.rng_offset == tw.rng_offset and ens.step_count == tw.step_count, (what, ens.rng_offset, tw.rng_offset)
    if hasattr(ens, "snap"):  # point-net: member g's tile 0 left the member's own front-end parameters of this step
        assert torch.equal(ens.snap[g, :ens.lay.n_front], tw._small.snap), (what, "snapshot")


def run_case(family, kind, d, B, G, K=10, reg_type="kl_reg", shared=False, per_member=False, epoch=1, steps=STEPS, inject=False,
             perturb=None, seed=0):
    """Build G members and their twins, run `steps` steps of both, compare after each -> (ens, final states).  perturb = g:
    member g gets other data and another seed (the independence test)."""
    need_rows(B)
    torch.manual_seed(100 + seed)
    models = [build(family, kind, d, K, reg_type).to(DEV) for _ in range(G)]
    twins_m = [copy.deepcopy(m) for m in models]
    x, mask = data(G, B, d, 7 + seed, shared)
    seeds = [11 + 3 * g for g in range(G)]
    lrs = [1e-3 * (1 + g) for g in range(G)] if per_member else [1e-3] * G
    alphas = [0.3 + 0.6 * g / max(1, G - 1) for g in range(G)] if per_member else [0.7] * G
    pms = [20 + 10 * g for g in range(G)] if per_member else [30] * G
    if perturb is not None:
        x, mask = x.clone(), mask.clone()
        x[perturb] = 1.0 - x[perturb]
        mask[perturb] = ~mask[perturb]
        seeds[perturb] += 1000
    cls = vpc.MaskEnsembleTrainer if family == "mask" else vpc.EDDIEnsembleTrainer
    ens = cls(models, lr=lrs, seeds=seeds)
    twins = [twin_of(family, m, lrs[g], seeds[g]) for g, m in enumerate(twins_m)]
    two = kind == "reg"
    planes = 3 if (two and reg_type == "ml_reg") else 2 if two else 1
    for s in range(steps):
        kw = dict(epoch=epoch + s, beta=0.9)
        draws = {}
        if inject:
            mp, eps = injected(G, B, d, mask if not shared else mask.expand(G, B, d), 50 + s, planes)
            draws = dict(zip(("eps_q", "eps_p", "eps_ml"), eps))
            if two:
                draws["mask_p"] = mp
        ens.step(x, mask, alpha=alphas, p_missingness=pms, **draws, **kw)
        for g, tw in enumerate(twins):
            xg, mg = (x, mask) if shared else (x[g], mask[g])
            tw.step(xg, mg, alpha=alphas[g], p_missingness=pms[g], **{k: v[g] for k, v in draws.items()}, **kw)
            assert on_small_path(family, tw)
            assert_member_equals_twin(ens, g, tw, f"{family} {kind} d={d} B={B} G={G} step {s} member {g}")
    # the members differ from each other wherever their inputs do (a launch that served every member from member 0 would not)
    if per_member or not shared:
        assert not torch.equal(ens.params[0], ens.params[1])
    return ens, [state_of(ens, g) for g in range(G)]


# ------------------------------------------------------------------ 1. the twin table
MASK_CASES = [
    # (kind, reg_type, d, B, G, shared, per_member, epoch): what it reaches
    ("reg", "kl_reg", 14, 37, 3, False, True, 1),    # pitch 16 != d; (DTI, DT) = (2, 1); 3 tiles, the last one 5 rows; all per member
    ("van", None, 5, 16, 2, True, False, 1),         # (1, 1); one pass; one shared batch
    ("reg", "ml_reg", 20, 16, 9, False, False, 1400),  # (4, 2); third eps plane; order 1 with 7 surplus workgroups
    ("reg", "kl_reg", 40, 16, 2, False, False, 1),   # (8, 4)
]


@pytest.mark.parametrize("kind,reg_type,d,B,G,shared,per_member,epoch", MASK_CASES)
def test_mask_members_equal_their_twins(kind, reg_type, d, B, G, shared, per_member, epoch):
    ens, _ = run_case("mask", kind, d, B, G, reg_type=reg_type, shared=shared, per_member=per_member, epoch=epoch)
    assert ens.order == (1 if G >= 8 else 0) and ens.dk == ops.small_aug_pitch(d)
    assert ops.small_aug_tiles(d) == {14: (2, 1), 5: (1, 1), 20: (4, 2), 40: (8, 4)}[d]


EDDI_CASES = [
    ("reg", "kl_reg", 10, 12, 37, 3, False, True, 1),    # (1, 1); partial last tile; per-member snapshot and front-end Adam
    ("van", None, 20, 12, 16, 9, True, False, 1),        # (2, 1); order 1 surplus; shared batch
    ("reg", "ml_reg", 10, 40, 16, 2, False, False, 1400),  # (1, 4); third eps plane
]


@pytest.mark.parametrize("kind,reg_type,K,d,B,G,shared,per_member,epoch", EDDI_CASES)
def test_eddi_members_equal_their_twins(kind, reg_type, K, d, B, G, shared, per_member, epoch):
    ens, _ = run_case("eddi", kind, d, B, G, K=K, reg_type=reg_type, shared=shared, per_member=per_member, epoch=epoch)
    assert ops.small_eddi_tiles(d, K) == {(10, 12): (1, 1), (20, 12): (2, 1), (10, 40): (1, 4)}[(K, d)]
    assert not torch.equal(ens.snap[0, :ens.lay.n_front], ens.snap[1, :ens.lay.n_front])  # (a snapshot per member)


@pytest.mark.parametrize("K,d", [(16, 32), (32, 20), (20, 64)])
def test_eddi_remaining_instantiations(K, d):
    """(DTI, DT) = (1, 2), (2, 2), (2, 4): one step each."""
    run_case("eddi", "reg", d, 16, 2, K=K, steps=1)
    assert ops.small_eddi_tiles(d, K) == {(16, 32): (1, 2), (32, 20): (2, 2), (20, 64): (2, 4)}[(K, d)]


def test_eddi_width_14_takes_injected_draws_and_refuses_to_draw():
    """obs_dim 14: the kernel's rows have 16 columns, the stand-alone stream is drawn at 14.  All draws injected: the twin
    comparison; none: VpcError before any launch, parameters and rng_offset untouched."""
    ens, _ = run_case("eddi", "reg", 14, 16, 2, inject=True)
    assert ens.dk == 16 and ens.rng_offset == 0
    before = (ens.params.clone(), ens.rng_offset, ens.step_count)
    x, mask = data(2, 16, 14, 3)
    with pytest.raises(vpc.VpcError, match="multiple of 4"):
        ens.step(x, mask, alpha=0.7)
    assert torch.equal(ens.params, before[0]) and (ens.rng_offset, ens.step_count) == before[1:]


# ------------------------------------------------------------------ 2. anchors captured from the reference
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _load_eddi(g, cls, *extra, prefix="param0."):
    model = cls(g["x"].shape[1], 500, int(g["K"]), int(g["L"]), TP, "exp", *extra)
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(prefix)})
    return model.to(DEV)


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_eddi_golden_trajectory(kind):
    """Members 0 and 1 start from the reference's parameters and are fed its draws: its five losses (1e-4) and final
    parameters (5e-5), the bounds of tests/test_eddi_small_gpu.py::test_adam_trajectory.  Member 2 has another alpha (reg)
    resp. beta (vanilla: alpha does not enter its loss): it leaves the reference and equals its own twin."""
    g = load_golden(f"eddi_traj_{kind}_d14.npz")
    B = g["x"].shape[0]
    need_rows(B)
    load = (lambda: _load_eddi(g, vpc.Reg_EDDI, "kl_reg")) if kind == "reg" else (lambda: _load_eddi(g, vpc.vanilla_EDDI))
    models, twin_m = [load() for _ in range(3)], load()
    ens = vpc.EDDIEnsembleTrainer(models, lr=1e-3, seeds=[0, 1, 2])
    twin = vpc.EDDITrainer(twin_m, lr=1e-3, seed=2)
    alphas, betas = ([0.5, 0.5, 0.8], 1.0) if kind == "reg" else (0.5, [1.0, 1.0, 0.6])
    x, m = _dev(g["x"]), _dev(g["mask"])
    for s in range(len(g["losses"])):
        eps = _dev(g["eps"][s])
        draws = dict(mask_p=_dev(g["mask_p"][s]), eps_q=eps[0], eps_p=eps[1]) if kind == "reg" else dict(eps_q=eps[0])
        ens.step(x, m, epoch=s + 1, alpha=alphas, beta=betas, **draws)
        twin.step(x, m, epoch=s + 1, alpha=0.8 if kind == "reg" else 0.5, beta=1.0 if kind == "reg" else 0.6, **draws)
        assert twin.last_path == "small"
        losses, ref = ens.loss_values(), float(g["losses"][s])
        print(kind, s, losses, ref)
        for gi in (0, 1):
            assert abs(losses[gi] - ref) <= 1e-4 * abs(ref), (s, gi, losses[gi], ref)
        assert abs(losses[2] - ref) > 1e-4 * abs(ref), (s, losses[2], ref)
        assert_member_equals_twin(ens, 2, twin, f"traj {kind} step {s} member 2")
    for gi in (0, 1):
        sd = models[gi].state_dict()
        for k, v in g.items():
            if k.startswith("param5."):
                a, b = sd[k[7:]].double().cpu(), torch.from_numpy(v).double()
                err, scale = float((a - b).abs().max()), max(1.0, float(b.abs().max()))
                assert err <= 5e-5 * scale, (gi, k, err, scale)
    assert torch.equal(ens.params[0], ens.params[1])


def test_mask_golden_step():
    """maskaugm_d14.npz (B = 48, d = 14) through one injected step of a Reg_VAE_mask and a vanilla_VAE_mask ensemble: loss 2e-5,
    every gradient tensor 2e-4 of its maximum (tests/test_small_augm_gpu.py::test_reference_vectors)."""
    g = load_golden("maskaugm_d14.npz")
    need_rows(48)
    x, mk, mp = (_dev(np.array(g[k])) for k in ("x", "mask", "mask_p"))

    def members(kind):
        out = []
        for _ in range(2):
            m = build("mask", kind, 14)
            sd = m.state_dict()
            pre = f"{'reg' if kind == 'reg' else 'vanilla'}.param."
            sd.update({k[len(pre):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(pre) and "prior" not in k})
            m.load_state_dict(sd)
            out.append(m.to(DEV))
        return out

    def check(ens, tag):
        for gi in range(2):
            loss, ref = float(ens.out9[gi, 0]), float(g[f"{tag}.loss"])
            print(tag, gi, "loss", loss, "ref", ref)
            assert np.isfinite(loss) and abs(loss - ref) <= 2e-5 * abs(ref), (tag, gi, loss, ref)
            flat, off = ens.grad[gi].cpu().numpy(), 0
            for k, p in zip(O.PARAM_KEYS, ens.models[gi].trainable()):
                got, want = flat[off:off + p.numel()].reshape(p.shape).astype(np.float64), np.asarray(g[f"{tag}.grad.{k}"], np.float64)
                err = float(np.max(np.abs(got - want)) / (np.max(np.abs(want)) + 1e-30))
                print(tag, gi, k, err)
                assert err < 2e-4, (tag, gi, k, err)
                off += p.numel()
            assert off == flat.size

    ens = vpc.MaskEnsembleTrainer(members("reg"))
    ens.step(x, mk, mp, _dev(np.array(g["reg.eps_q"])), _dev(np.array(g["reg.eps_p"])), alpha=0.7, beta=0.9)
    check(ens, "reg")
    ens = vpc.MaskEnsembleTrainer(members("van"))
    ens.step(x, mk, eps_q=_dev(np.array(g["vanilla.eps_q"])), beta=0.9)
    check(ens, "vanilla")


# ------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("family", ["mask", "eddi"])
def test_members_are_independent(family):
    """The first row of the family's table twice; the second time member 1 has other data and another seed: member 0's
    parameters, moments, gradient and loss terms are bit for bit what they were."""
    d = 14 if family == "mask" else 12
    _, a = run_case(family, "reg", d, 37, 3, per_member=True)
    _, b = run_case(family, "reg", d, 37, 3, per_member=True, perturb=1)
    for ta, tb in zip(a[0], b[0]):
        assert torch.equal(ta, tb)
    for ta, tb in zip(a[2], b[2]):
        assert torch.equal(ta, tb)
    assert not torch.equal(a[1][0], b[1][0])


# ------------------------------------------------------------------ 4. train_sweep
def test_train_sweep_equals_train_member_by_member(tmp_path, monkeypatch):
    d = 12
    need_rows(16)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(32, d, generator=g)
    mask = torch.rand(32, d, generator=g) < 0.7
    loader = [(x[0:16], mask[0:16]), (x[16:32], mask[16:32])]
    cfgs = [dict(vae_type="reg_vae1_mask_augm", alpha=0.5, seed=5), dict(vae_type="vanilla_EDDI1", seed=1),
            dict(vae_type="reg_vae2_mask_augm", alpha=0.8, seed=6), dict(vae_type="vanilla_EDDI2", seed=2)]
    torch.manual_seed(3)
    base = [build("mask", "reg", d), build("eddi", "van", d), build("mask", "reg", d), build("eddi", "van", d)]
    args = (30, d, 500, 10, 1, L, "synth", TP, "exp")
    (tmp_path / "sweep").mkdir()
    (tmp_path / "solo").mkdir()
    monkeypatch.chdir(tmp_path / "sweep")
    made = []
    for name in ("MaskEnsembleTrainer", "EDDIEnsembleTrainer"):
        cls = getattr(E, name)
        monkeypatch.setattr(vpc.harness, name, lambda ms, _cls=cls, **kw: made.append(_cls.__name__) or _cls(ms, **kw))
    out = vpc.train_sweep((loader, None), cfgs, *args, 20, 10, max_epochs=1, device=torch.device(DEV), reg_type="kl_reg",
                          verbose=False, models=[copy.deepcopy(m) for m in base])
    assert sorted(made) == ["EDDIEnsembleTrainer", "MaskEnsembleTrainer"]
    for c, m0, trained in zip(cfgs, base, out):
        path = vpc.checkpoint_path("exp", "synth", c["vae_type"], 30, c.get("alpha", 1.0), 30, "kl_reg")
        monkeypatch.chdir(tmp_path / "sweep")
        assert os.path.exists(path), path
        sweep_sd = torch.load(path, map_location="cpu", weights_only=True)
        monkeypatch.chdir(tmp_path / "solo")
        vpc.train((loader, None), *args, c["vae_type"], 20, 10, max_epochs=1, device=torch.device(DEV), alpha=c.get("alpha", 1.0),
                  p_missingness=30, reg_type="kl_reg", seed=c["seed"], verbose=False, model=copy.deepcopy(m0))
        solo = torch.load(path, map_location="cpu", weights_only=True)
        assert list(sweep_sd) == list(solo)
        for k in solo:
            assert torch.equal(sweep_sd[k], solo[k]), (c["vae_type"], k)
            assert torch.equal(trained.state_dict()[k].cpu(), solo[k]), (c["vae_type"], k)
        assert any(not torch.equal(solo[k], v) for k, v in m0.state_dict().items())  # it trained


# ------------------------------------------------------------------ 5. limits
def test_limits_raise_instead_of_launching():
    rows = ops.step_small_max_rows()
    if rows < 16:
        pytest.skip("the small-batch step is switched off")
    torch.manual_seed(0)
    tiles = (rows + 15) // 16
    many = E.MAX_BLOCKS // tiles + 1
    for family, cls in (("mask", vpc.MaskEnsembleTrainer), ("eddi", vpc.EDDIEnsembleTrainer)):
        ens = cls([build(family, "van", 4).to(DEV) for _ in range(2)])
        B = rows + 1
        with pytest.raises(vpc.VpcError, match="rows"):
            ens.step(torch.rand(B, 4, device=DEV), torch.ones(B, 4, dtype=torch.bool, device=DEV))
        if many <= 64:
            big = cls([build(family, "van", 4).to(DEV) for _ in range(many)])
            with pytest.raises(vpc.VpcError, match="workgroups"):
                big.step(torch.rand(rows, 4, device=DEV), torch.ones(rows, 4, dtype=torch.bool, device=DEV))
        with pytest.raises(vpc.VpcError, match="cover the plain"):
            ens.evaluator()
        # a member stride one block short: the wrappers raise "bad argument", nothing is launched
        x, mask = torch.rand(2, 32, 4, device=DEV), torch.ones(2, 32, 4, dtype=torch.uint8, device=DEV)
        ens.step(x, mask)  # (two tiles per member; allocates the workspaces used below)
        lay, st = ens.lay, list(ens._strides)
        st[ops.MS_X], st[ops.MS_MASK] = 32 * 4, 32 * 4
        short = list(st)
        short[ops.MS_PARTE] = 2 * lay.enc_part - 4
        head = (x, mask, None, ens.eps_buf, ens.img[0, :lay.enc_img], ens.img[0, lay.enc_img:], ens.table_dev, 2, 1, 1, 0, 0, 0,
                1.0 / 32, 0.0, ens.partE, ens.partD, ens.loss_part)
        with pytest.raises(vpc.VpcError, match="bad argument"):
            if family == "mask":
                ops.step_small_multi_aug_f32(*head, short, 32, 4, 4, L)
            else:
                ops.step_small_multi_eddi_f32(*head, short, 32, 4, 4, L, lay.K, ens.params[0, lay.n_params:], ens.partF, ens.snap)
        if family == "eddi":
            with pytest.raises(vpc.VpcError, match="bad argument"):
                ops.reduce_step_adam_eddi_multi(ens.partE, ens.partD, ens.loss_part, 2, lay.enc_part, lay.dec_part, short, ens.inv,
                                                ens.table_dev, 2, ens.grad, lay.n_params, 32, 4, ens.out9, ens.accum, ens.params,
                                                ens.exp_avg, ens.exp_avg_sq, 0.9, 0.999, 1e-8, 1, ens.pidx, ens.img, ens.partF,
                                                ens.snap, lay.K, 4)
    torch.cuda.synchronize()
