"""GPU parity of the MIWAE path (MIWAE / Reg_MIWAE, csrc/vpc_miw.hip) through the C ABI:
  * API forward, loss, every parameter gradient and the llh_eval branch against vectors recorded from the reference
    (tests/golden/miwae_*.npz), B > S and B not a multiple of S, so the reference's row / sample pairing is exercised,
  * the loss kernel alone against the float64 oracle (tests/miwae_oracle.py) at ragged shapes, both pairings,
  * the per-row pairing against single-row calls, 5-step Adam trajectories on the API path and on MIWTrainer,
  * device draws, harness.train / model_loader / eval_miwae with the reference's file names.
Tolerances: loss 1e-4 relative, gradients 2e-4 of the tensor's max (the MNAR path's)."""
import os

import numpy as np
import pytest
import torch

import miwae_oracle as O
from conftest import load_golden
from miwae_cases import api_loss as _api_loss, rand_inputs as _rand_inputs, raw_to_act as _raw_to_act

pytestmark = pytest.mark.gpu
TP = {"batch_size": 64, "patience": 1}


@pytest.fixture(scope="module")
def mw():
    import vpc_amd
    from vpc_amd import miwae
    return miwae


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, ref, tol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = float((got - ref).abs().max() / (ref.abs().max() + 1e-30))
    assert err <= tol, (what, err)


def _load_model(mw, g, cls, prefix="param."):
    torch.manual_seed(0)
    model = cls(g["x"].shape[1], 500, 10, int(g["L"]), TP, int(g["S"]), 1)
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(prefix)})
    return model.cuda()


@pytest.mark.parametrize("name", ["miwae_reg_d14", "miwae_reg_d40", "miwae_van_d14", "miwae_van_d40"])
def test_api_vs_reference(mw, name):
    g = load_golden(name + ".npz")
    reg = "reg" in name
    model = _load_model(mw, g, mw.Reg_MIWAE if reg else mw.MIWAE)
    x, m = _dev(g["x"]), _dev(g["mask"])
    mp = _dev(g["mask_p"]) if reg else None
    eps = _dev(g["eps"])
    cases = [(a, f"loss.a{a}", f"a{a}") for a in (1.0, 0.5, 0.0)] if reg else [(0.0, "loss", "v")]
    for alpha, lk, gk in cases:
        model.zero_grad()
        tl, outs = _api_loss(model, x, m, mp, eps, alpha)
        assert abs(tl.item() - g[lk]) <= 1e-4 * abs(g[lk]), (alpha, tl.item(), float(g[lk]))
        tl.backward()
        for k, p in model.named_parameters():
            _close(p.grad, torch.from_numpy(g[f"grad.{gk}.{k}"]), 2e-4, (alpha, k))
    names = (["mean_p", "scale_p", "x_mean_p", "x_scale_p", "deg_free_p", "mean_q", "scale_q", "x_mean_q", "x_scale_q",
              "deg_free_q"] if reg else ["mean", "scale", "x_mean", "x_scale", "deg_free"])
    for n, t in zip(names, outs):
        _close(t, torch.from_numpy(g["fwd." + n]), 2e-5, n)
    with torch.no_grad():
        el = _dev(g["eps_llh"])
        if reg:
            o = outs
            xm, tl, t3 = model.loss(x, o[2], o[3], o[4], o[0], o[1], o[7], o[8], o[9], o[5], o[6], m, mp, 1, alpha=0.5,
                                    llh_eval=True, eps=[el[0], el[1]])
        else:
            o = outs
            xm, tl, t3 = model.loss(x, o[2], o[3], o[4], o[0], o[1], m, 1, llh_eval=True, eps=el[0])
    assert abs(tl.item() - g["llh_loss"]) <= 1e-4 * abs(g["llh_loss"])
    assert abs(t3.item() - g["llh_third"]) <= 1e-4 * abs(g["llh_third"])
    _close(xm, torch.from_numpy(g["llh_xm"]), 2e-5, "llh_xm")


@pytest.mark.parametrize("pairing", ["reference", "per_row"])
@pytest.mark.parametrize("raw", [0, 1])
def test_loss_kernel_vs_oracle(mw, pairing, raw):
    """vpc_miw_loss alone at a ragged shape (d = 70, B = 33, S = 7, L = 5), on activated and on raw decoder heads."""
    B, S, d, Ld = 33, 7, 70, 5
    x, m, mp, oq, op, e = _rand_inputs(B, S, d, Ld, 9)
    pid = mw.PAIR_REFERENCE if pairing == "reference" else mw.PAIR_PER_ROW
    for reg in (True, False):
        alpha = 0.3
        leaves = []

        def pas(o):
            Yr = torch.from_numpy(o[0]).double().requires_grad_()
            act = [t.reshape(B, S, d) for t in _raw_to_act(o[0], d)]
            if raw:  # differentiate through the head transforms
                Ya = torch.cat([torch.sigmoid(Yr[:, :d]), torch.nn.functional.softplus(Yr[:, d:2 * d]) + 0.001,
                                torch.nn.functional.softplus(Yr[:, 2 * d:]) + 3], 1)
                act = [Ya[:, i * d:(i + 1) * d].reshape(B, S, d) for i in range(3)]
                leaf_y = Yr
            else:
                act = [a.clone().requires_grad_() for a in act]
                leaf_y = act
            mean = torch.from_numpy(o[1]).double().requires_grad_()
            scale = torch.from_numpy(o[2]).double().requires_grad_()
            leaves.append((leaf_y, mean, scale))
            return tuple(act), mean, scale

        q = pas(oq)
        p = pas(op) if reg else None
        eps2 = [torch.from_numpy(e[0]), torch.from_numpy(e[1])]
        ref, _ = O.loss(torch.from_numpy(x), torch.from_numpy(m), torch.from_numpy(mp) if reg else None, q, p, eps2,
                        alpha, pairing)
        ref.backward()
        # the kernel's inputs
        dev_y = lambda o: _dev(o[0]) if raw else _dev(np.concatenate([t.reshape(B * S, d).numpy() for t in
                                                                       _raw_to_act(o[0], d)], 1).astype(np.float32))
        Yq, Yp = dev_y(oq), dev_y(op)
        hq, hp = _dev(np.concatenate([oq[1], oq[2]], 1)), _dev(np.concatenate([op[1], op[2]], 1))
        Gq, Gp = torch.empty(B * S, 3 * d, device="cuda"), torch.empty(B * S, 3 * d, device="cuda")
        ghq, ghp = torch.empty(B, 2 * Ld, device="cuda"), torch.empty(B, 2 * Ld, device="cuda")
        out8 = torch.empty(8, dtype=torch.float64, device="cuda")
        ed = _dev(e)
        mw.miw_loss(_dev(x), _dev(m), _dev(mp) if reg else None, Yq, Yp if reg else None, 3 * d, raw, hq,
                    hp if reg else None, ed[0], ed[1] if reg else None, Gq, Gp if reg else None, 3 * d, ghq,
                    ghp if reg else None, None, mw.miw_loss_scratch(B, S, "cuda"), out8, None, None, B, S, d, Ld, alpha,
                    pid)
        assert abs(out8[0].item() - ref.item()) <= 2e-5 * abs(ref.item()), (reg, out8[0].item(), ref.item())
        for k, (G, gh) in enumerate([(Gq, ghq), (Gp, ghp)][:2 if reg else 1]):
            ly, mean, scale = leaves[k]
            gref = ly.grad if raw else torch.cat([a.grad.reshape(B * S, d) for a in ly], 1)
            for i, head in enumerate(("mean", "scale", "df")):  # each head block on its own max: the df block is the smallest
                _close(G[:, i * d:(i + 1) * d], gref[:, i * d:(i + 1) * d], 5e-5, ("dY", head, reg, k))
            _close(gh[:, :Ld], mean.grad, 5e-5, ("dmean", reg, k))
            _close(gh[:, Ld:], scale.grad, 5e-5, ("dscale", reg, k))


def test_per_row_equals_single_rows(mw):
    """PAIR_PER_ROW on N rows (loss terms and the llh_eval imputation) equals N single-row calls."""
    B, S, d, Ld = 6, 9, 12, 4
    x, m, mp, oq, op, e = _rand_inputs(B, S, d, Ld, 4)
    X, Mq, Mp, ed = _dev(x), _dev(m), _dev(mp), _dev(e)
    Yq, Yp = _dev(oq[0]), _dev(op[0])
    hq, hp = _dev(np.concatenate([oq[1], oq[2]], 1)), _dev(np.concatenate([op[1], op[2]], 1))
    imp = torch.empty(B, d, device="cuda")
    out8 = torch.empty(8, dtype=torch.float64, device="cuda")
    mw.miw_loss(X, Mq, Mp, Yq, Yp, 3 * d, 1, hq, hp, ed[0], ed[1], None, None, 3 * d, None, None, imp,
                mw.miw_loss_scratch(B, S, "cuda"), out8, None, None, B, S, d, Ld, 0.5, mw.PAIR_PER_ROW)
    tot = 0.0
    for j in range(B):
        r = slice(j * S, (j + 1) * S)
        imp1 = torch.empty(1, d, device="cuda")
        o1 = torch.empty(8, dtype=torch.float64, device="cuda")
        mw.miw_loss(X[j:j + 1], Mq[j:j + 1], Mp[j:j + 1], Yq[r], Yp[r], 3 * d, 1, hq[j:j + 1], hp[j:j + 1],
                    ed[0, j:j + 1], ed[1, j:j + 1], None, None, 3 * d, None, None, imp1,
                    mw.miw_loss_scratch(1, S, "cuda"), o1, None, None, 1, S, d, Ld, 0.5, mw.PAIR_REFERENCE)
        assert torch.allclose(imp1[0], imp[j], rtol=1e-6, atol=1e-7), j
        tot += o1[0].item()
    assert abs(out8[0].item() - tot / B) <= 1e-5 * abs(tot / B)


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_api_adam_trajectory(mw, kind):
    """model.forward / loss / backward + optim.Adam as train.py:102-117, draws and mask_p injected."""
    g = load_golden(f"miwae_traj_{kind}_d14.npz")
    model = _load_model(mw, g, mw.Reg_MIWAE if kind == "reg" else mw.MIWAE, "param0.")
    model.flatten_parameters()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    x, m = _dev(g["x"]), _dev(g["mask"])
    for s in range(len(g["losses"])):
        mp = _dev(g["mask_p"][s]) if kind == "reg" else None
        tl, _ = _api_loss(model, x, m, mp, _dev(g["eps"][s]), 0.5)
        opt.zero_grad()
        tl.backward()
        opt.step()
        assert abs(tl.item() - g["losses"][s]) <= 1e-4 * abs(g["losses"][s]), (s, tl.item(), g["losses"][s])
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith("param5."):
            _close(sd[k[7:]], torch.from_numpy(v), 5e-5, k)


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_trainer_trajectory(mw, kind):
    """MIWTrainer (stacked q/p GEMMs, raw-head loss, flat grads, flat Adam) reproduces the reference's trajectory."""
    g = load_golden(f"miwae_traj_{kind}_d14.npz")
    model = _load_model(mw, g, mw.Reg_MIWAE if kind == "reg" else mw.MIWAE, "param0.")
    tr = mw.MIWTrainer(model, lr=1e-3)
    x, m = _dev(g["x"]), _dev(g["mask"]).bool()
    total = 0.0
    for s in range(len(g["losses"])):
        tr.step(x, m, mask_p=_dev(g["mask_p"][s]) if kind == "reg" else None, eps=_dev(g["eps"][s]), alpha=0.5)
        assert abs(tr.loss_value() - g["losses"][s]) <= 1e-4 * abs(g["losses"][s]), (s, tr.loss_value())
        total += g["losses"][s]
    assert abs(tr.epoch_total() - total) <= 1e-4 * abs(total)
    sd = model.state_dict()
    for k, v in g.items():
        if k.startswith("param5."):
            _close(sd[k[7:]], torch.from_numpy(v), 5e-5, k)


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_trainer_device_draws(mw, kind):
    """Device-drawn mask_p is a sub-mask of mask, a seed reproduces the run bit for bit, and the loss goes down."""
    cls = mw.Reg_MIWAE if kind == "reg" else mw.MIWAE
    B, d = 64, 12
    gen = torch.Generator(device="cuda").manual_seed(2)
    x = torch.rand(B, d, device="cuda", generator=gen)
    m = torch.rand(B, d, device="cuda", generator=gen) < 0.6
    runs = []
    for _ in range(2):
        torch.manual_seed(7)
        model = cls(d, 500, 10, 10, TP, 20, 1).cuda()
        tr = mw.MIWTrainer(model, lr=3e-3, seed=11)
        losses = []
        for s in range(40):
            tr.step(x, m, alpha=0.5, p_missingness=30)
            if kind == "reg" and s == 0:
                assert bool(((tr.mask_p != 0) <= m).all()) and 0 < float(tr.mask_p.sum()) < float(m.sum())
            losses.append(tr.loss_value())
        runs.append((losses, model._flat.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])
    ls = runs[0][0]
    assert np.mean(ls[-5:]) < np.mean(ls[:5]), ls


def test_world_size_and_cpu_raise(mw):
    import vpc_amd
    model = mw.MIWAE(12, 500, 10, 10, TP, 5, 1).cuda()
    with pytest.raises(vpc_amd.VpcError):
        mw.MIWTrainer(model, world_size=2, rank=0)
    with pytest.raises(vpc_amd.VpcError):
        mw.MIWAE(12, 500, 10, 10, TP, 5, 1).forward(torch.rand(4, 12), torch.ones(4, 12))
    with pytest.raises(vpc_amd.VpcError):
        mw.Reg_MIWAE(300, 500, 10, 10, TP, 5, 1)


def test_model_loader_dispatch(mw):
    import vpc_amd
    keys = [f"seq_{p}.{i}.{w}" for p in ("encoder", "decoder") for i in (0, 2, 4) for w in ("weight", "bias")]
    for vae_type, cls in (("reg_MIWAE1", mw.Reg_MIWAE), ("vanilla_MIWAE2", mw.MIWAE)):
        model = vpc_amd.model_loader("train", 12, 500, 10, 10, 50, "wine", TP, 10, 20, 100,
                                     "UCI_experiments_consistency_missingness", "kl_reg", vae_type)
        assert type(model) is cls
        assert list(model.state_dict()) == keys
    with pytest.raises(NotImplementedError):
        vpc_amd.model_loader("train", 12, 500, 10, 10, 50, "wine", TP, 10, 20, 100, "exp", "kl_reg", "vanilla_flow1")


def test_harness_train_miwae(mw, tmp_path, monkeypatch):
    """train() for both MIWAE names, fused (MIWTrainer) and API path: reference-named checkpoints that load back."""
    import vpc_amd
    from torch.utils.data import DataLoader, TensorDataset
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    x = torch.rand(96, 12)
    m = torch.rand(96, 12) < 0.7
    loader = DataLoader(TensorDataset(x, m), batch_size=32, shuffle=False)
    for vae_type in ("reg_MIWAE1", "vanilla_MIWAE1"):
        for fused in (True, False):
            torch.manual_seed(1)
            model = vpc_amd.train((loader, None), 50, 12, 500, 10, 1, 10, "toy", TP, "exp", vae_type, 5, 1,
                                  max_epochs=2, alpha=0.5, p_missingness=30, reg_type="kl_reg", fused=fused,
                                  verbose=False)
            ck = vpc_amd.checkpoint_path("exp", "toy", vae_type, 50, 0.5, 30, "kl_reg")
            assert os.path.exists(ck)
            again = vpc_amd.model_loader("test", 12, 500, 10, 10, 50, "toy", TP, 2, 5, 1, "exp", "kl_reg", vae_type,
                                         alpha=0.5, p_missingness=30)
            for (k, a), (_, b) in zip(model.state_dict().items(), again.state_dict().items()):
                assert torch.equal(a.cpu(), b.cpu()), (vae_type, fused, k)


@pytest.mark.parametrize("kind", ["reg", "van"])
def test_eval_miwae_checkpoint_interop(mw, kind, tmp_path, monkeypatch):
    """A checkpoint in the reference's naming scheme loads through model_loader('test'); eval_miwae (evaluate.py:72-133)
    lands within the spread of the RMSEs the reference wrote for it over six seeds, under the reference's file name."""
    import vpc_amd
    g = load_golden(f"miwae_eval_{kind}_d14.npz")
    vae_type = "reg_MIWAE1" if kind == "reg" else "vanilla_MIWAE1"
    monkeypatch.chdir(tmp_path)
    ck = vpc_amd.checkpoint_path("exp", "toy", vae_type, 40, alpha=0.5, p_missingness=30, reg_type="kl_reg")
    assert os.path.basename(ck) == str(g["checkpoint_file"])
    os.makedirs(os.path.dirname(ck))
    torch.save({k[6:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("param.")}, ck)
    x, mask = torch.from_numpy(g["x"]), torch.from_numpy(g["mask"])
    loaders = [([(x[:16], mask[:16]), (x[16:], mask[16:])], "test")]
    res = vpc_amd.eval_miwae(loaders, 40, 14, 500, 10, int(g["M"]), int(g["L"]), "toy", TP, "exp", vae_type, 100,
                             int(g["valid_k"]), 1, alpha=0.5, p_missingness=30, reg_type="kl_reg",
                             max_decoder_rows=2000)
    ref = g["rmse"]
    lo, hi = ref.min() - 3 * ref.std() - 1e-3 * ref.mean(), ref.max() + 3 * ref.std() + 1e-3 * ref.mean()
    assert lo <= res["test"].item() <= hi, (res["test"].item(), ref)
    fam = "".join(c for c in vae_type if not c.isdigit())
    assert os.listdir(os.path.join("experiments", "exp", "toy", "rest", fam)) == [str(g["result_file"])]
