"""Golden vectors for the flow models' config 5 reward, produced by running the REFERENCE itself
(src/experiment_main/evaluate.py: R_lindley_chain_ratio_version :637-665 and active_learning_func :300-511).

    cd <repo> && VPC_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_flow_reward.py

Authoring container only: imports the reference checkout (never copied, never shipped) and stores DATA only.

  flow_reward_{reg_d12,van_d9}.npz   state_dict, x, mask, im [M, n, d] (M forwards of the model), R [n, d-1] from the
                                     reference's R_lindley_chain_ratio_version called for every candidate as
                                     active_learning_func does (:416-422), and the draws: Normal.rsample is wrapped to
                                     record each draw in call order, and the draws are scattered into the dense layout
                                     eps [d-1, M, 4, n, 10] (call order Ia, Ib, IIa, IIb; rows outside loc(u) zero).
                                     reg: d 12, hid 64, n 24, M 3; van: d 9, hid 72 (ragged), n 16, M 2; both after a
                                     short training run.  Masks: some columns observed per row, two rows with the target
                                     marked observed (the carry-over of evaluate.py:653-658 is visible there), one column
                                     observed in every row (empty loc).
  flow_reward_quirk_reg.npz          the reg case with INJECTED draws (as make_golden_flow.py's gen_quirk): one (u, m, call)
                                     group has every |eps| > 1 on loc(u), so torch.any(inside) (VAE.py:1698) is false for
                                     that encoder call only; rows outside loc(u) hold inside values there.
  flow_active_reg_d8.npz             the reference's own active_learning_func on 'reg_flow1' (d 8, hid 64, n 12, M 3,
                                     Repeat 1): x_mean_q of every forward call in order, the reward draws of every step in
                                     the dense layout, R_hist, action, information curve, im and the four file names.

Each reward file also stores `delta`: 8 x the largest difference between a layer-2 / layer-3 bin position of the
reference's fp32 run (unconstrained_linear_spline's inputs, recorded through a wrapper) and of the float64 oracle over
the file's evaluations.  The generator asserts that the oracle alone flags at most 5 % of the unobserved entries with it
(pick another seed otherwise) and that every unflagged entry meets the bound of tests/flow_reward_oracle.py.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = os.environ["VPC_REFERENCE"]
OUT = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))
tv = types.ModuleType("torchvision")
tv.datasets = types.ModuleType("torchvision.datasets")
tv.transforms = types.ModuleType("torchvision.transforms")
sys.modules["torchvision"] = tv
sys.modules["torchvision.datasets"] = tv.datasets
sys.modules["torchvision.transforms"] = tv.transforms

import src.models.VAE as RV  # noqa: E402
import src.experiment_main.evaluate as EV  # noqa: E402
import flow_reward_oracle as FR  # noqa: E402

TP = {"batch_size": 64, "patience": 100}
L = 10


class Draws:
    """Normal.rsample wrapped: records every draw in call order, or (inject=list) returns the given draws in order.
    `muted` (set around model.forward) keeps the forwards' draws out of the record."""

    def __init__(self, inject=None):
        self.rec, self.inject, self.muted = [], None if inject is None else list(inject), False

    def __enter__(self):
        self.orig = torch.distributions.Normal.rsample
        me = self

        def rsample(self_, sample_shape=torch.Size()):
            if me.inject is not None and not me.muted:
                return me.inject.pop(0).clone()
            v = me.orig(self_, sample_shape)
            if not me.muted:
                me.rec.append(v.detach().numpy().copy())
            return v

        torch.distributions.Normal.rsample = rsample
        return self

    def __exit__(self, *a):
        torch.distributions.Normal.rsample = self.orig


class SplineInputs:
    """unconstrained_linear_spline wrapped (a module attribute; the reference source is not modified): records the inputs
    of every call, three per encoder call."""

    def __enter__(self):
        self.orig, self.rec = RV.unconstrained_linear_spline, []

        def spline(inputs, *a, **kw):
            self.rec.append(inputs.detach().numpy().copy())
            return self.orig(inputs, *a, **kw)

        RV.unconstrained_linear_spline = spline
        return self

    def __exit__(self, *a):
        RV.unconstrained_linear_spline = self.orig


def scatter(draws, mask, M):
    """Draws in call order (u, m, call; |loc(u)| rows each) -> dense [d-1, M, 4, n, 10], zero outside loc(u)."""
    n, d = mask.shape
    eps = np.zeros((d - 1, M, 4, n, L), np.float32)
    it = iter(draws)
    for u in range(d - 1):
        loc = np.where(mask[:, u] == 0)[0]
        for m in range(M):
            for c in range(4):
                eps[u, m, c, loc] = next(it)
    assert next(it, None) is None
    return eps


def gather(eps, mask, M):
    out = []
    for u in range(mask.shape[1] - 1):
        loc = np.where(mask[:, u] == 0)[0]
        for m in range(M):
            for c in range(4):
                out.append(torch.from_numpy(eps[u, m, c, loc].copy()))
    return out


def make_data(n, d, g):
    base = torch.rand(n + 256, 3, generator=g)
    mix = torch.rand(3, d, generator=g)
    data = torch.sigmoid(3.0 * (base @ mix / mix.sum(0) - 0.5)) + 0.05 * torch.rand(n + 256, d, generator=g)
    data = (data - data.min(0).values) / (data.max(0).values - data.min(0).values)
    return data[n:], data[:n].clone()


def trained(kind, d, H, xtr, g, steps=60):
    model = (RV.REG_VAEFlow if kind == "reg" else RV.VAEFlow)(d, H, 10, L, TP)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    mtr = torch.rand(256, d, generator=g) < 0.7
    for s in range(steps):
        if kind == "reg":
            mp = mtr & (torch.rand(256, d) < 0.7)
            o = model.forward(xtr, mtr, mp)
            _, tl = model.loss(xtr, o[6], o[7], o[4], o[5], o[2], o[3], o[0], o[1], mtr, mp, 0.5)
        else:
            o = model.forward(xtr, mtr)
            _, tl = model.loss(xtr, o[2], o[3], o[0], o[1], mtr)
        opt.zero_grad(); tl.backward(); opt.step()
    return model


def forwards(model, kind, x, mask, M):
    with torch.no_grad():
        if kind == "reg":
            return torch.stack([model.forward(x, mask, mask)[6] for _ in range(M)], 0)
        return torch.stack([model.forward(x, mask)[2] for _ in range(M)], 0)


def reference_R(model, x, mask, M, im, inject=None):
    n, d = x.shape
    R = -1e4 * torch.ones(n, d - 1)
    with torch.no_grad(), Draws(inject) as dr, SplineInputs() as sp:
        for u in range(d - 1):  # evaluate.py:416-422
            loc = np.where(mask[:, u] == 0)[0]
            R[loc, u] = EV.R_lindley_chain_ratio_version(u, x, mask, M, model, im, loc).float()
    return R.numpy(), dr.rec, sp.rec


def measure_delta(P, x, mask, im, eps, spline_inputs):
    """8 x the largest |bin position (reference, fp32) - bin position (oracle, float64)| over layers 2 and 3 of every
    evaluation (layer 3 only where both runs chose the same layer-2 bin: past a flip the inputs are unrelated)."""
    trace = []
    orig = FR.encoder_zlp

    def enc(P_, x_, m_, e_):
        zlp, cache = orig(P_, x_, m_, e_)
        trace.append(cache)
        return zlp, cache

    FR.encoder_zlp = enc
    try:
        res = FR.reward_matrix(P, x, mask, im, eps)
    finally:
        FR.encoder_zlp = orig
    calls = [spline_inputs[i:i + 3] for i in range(0, len(spline_inputs), 3)]
    calls = [c for c in calls if c[0].shape[0] > 0]
    assert len(calls) == len(trace)
    worst = 0.0
    for c, cache in zip(calls, trace):
        if cache is None:
            continue
        steps = cache[3]
        bp32 = [(np.asarray(v, np.float32) + np.float32(1)) / np.float32(2) * np.float32(L) for v in c]
        bp64 = [b + al for b, al, _, _ in steps]
        worst = max(worst, float(np.abs(bp32[1] - bp64[1]).max()))
        same = np.minimum(np.floor(bp32[1]), L - 1) == steps[1][0]
        if same.any():
            worst = max(worst, float(np.abs(bp32[2] - bp64[2])[same].max()))
    return 8 * worst, res


def make_mask(n, d, g, target_rows=(1, 4), full_col=5):
    mask = (torch.rand(n, d, generator=g) < 0.35).float()
    mask[:, -1] = 0
    for r in target_rows:
        mask[r, -1] = 1
    mask[:, full_col] = 1
    return mask


def gen_reward(kind, d, H, n, M, seed, name, quirk=False, tries=40):
    """The first seed from `seed` on whose inputs the oracle flags at most 5 % of the unobserved entries."""
    for s in range(seed, seed + tries):
        if _gen_reward(kind, d, H, n, M, s, name, quirk):
            return
    raise AssertionError(f"{name}: no seed in [{seed}, {seed + tries}) keeps the flagged share within 5 %")


def _gen_reward(kind, d, H, n, M, seed, name, quirk):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    xtr, x = make_data(n, d, g)
    model = trained(kind, d, H, xtr, g)
    mask = make_mask(n, d, g)
    im = forwards(model, kind, x, mask, M)
    inject = None
    if quirk:
        eps = torch.randn(d - 1, M, 4, n, L, generator=g).numpy()
        u, m, c = 2, 1, 3
        loc = np.where(mask.numpy()[:, u] == 0)[0]
        grp = eps[u, m, c]
        grp[:] = np.clip(grp, -0.9, 0.9)                                   # rows outside loc(u): inside values
        grp[loc] = np.sign(grp[loc] + 1e-9) * (1.05 + np.abs(grp[loc]))  # loc(u): every draw outside [-1, 1]
        inject = gather(eps, mask.numpy(), M)
    R, draws, spl = reference_R(model, x, mask, M, im, inject)
    if not quirk:
        eps = scatter(draws, mask.numpy(), M)
    P = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    delta, res = measure_delta(P, x.numpy(), mask.numpy(), im.numpy(), eps, spl)
    err, bound, share = FR.compare(R, res["R"], res["edge"], res["S"], delta)
    print(name, "seed", seed, "delta", delta, "S", res["S"], "oracle vs reference", err, "bound", bound, "flagged", share)
    if share > FR.MAX_FLAGGED:
        return False
    assert err <= bound
    assert np.array_equal(R == -1e4, res["R"] == -1e4)
    out = {"param." + k: v for k, v in P.items()}
    out.update(x=x.numpy(), mask=mask.numpy(), im=im.numpy(), eps=eps.astype(np.float32), R=R, delta=np.float64(delta),
               hid=np.int64(H), M=np.int64(M))
    if quirk:
        out["quirk_group"] = np.array([2, 1, 3])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    return True


def gen_active(d=8, H=64, n=12, M=3, seed=515):
    torch.manual_seed(seed)
    np.random.seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    vae_type, fam = "reg_flow1", "reg_flow"
    xtr, x = make_data(n, d, g)
    model = trained("reg", d, H, xtr, g, steps=100)
    test_mask = torch.rand(n, d, generator=g) < 0.7
    out = {"param." + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    calls = []
    orig_loader = EV.model_loader
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp, Draws() as dr:
        def loader(*a, **kw):
            m = orig_loader(*a, **kw)
            fwd = m.forward

            def rec(*fa, **fk):
                dr.muted = True
                try:
                    r = fwd(*fa, **fk)
                finally:
                    dr.muted = False
                calls.append(r[6].detach().numpy().copy())  # x_mean_q
                return r

            m.forward = rec
            return m

        os.chdir(tmp)
        try:
            for sub in ("checkpoints", "rest"):
                os.makedirs(os.path.join("experiments", "exp", "toy", sub, fam))
            torch.save(model.state_dict(), f"experiments/exp/toy/checkpoints/{fam}/checkpoint_{vae_type}_1.0_30_kl_reg_30_"
                                           "missing_rate_full_reg_test.pt")
            EV.model_loader = loader
            torch.manual_seed(seed + 7)
            EV.active_learning_func(None, x, test_mask, 30, d, H, 10, M, L, "toy", TP, "exp", vae_type, 100, 1, 1,
                                    alpha=1.0, p_missingness=30, reg_type="kl_reg", Repeat=1)
            rest = f"experiments/exp/toy/rest/{fam}"
            files = sorted(os.listdir(rest))
            res = {}
            for f in files:
                key = [k for k in ("information_curve_CHAI", "action_CHAI", "R_hist_CHAI", "im_CHAI") if k in f][0]
                res[key] = torch.load(os.path.join(rest, f))
        finally:
            EV.model_loader = orig_loader
            os.chdir(cwd)
    steps = d - 1
    assert len(files) == 4 and len(calls) == M + steps * 2 * M
    action = res["action_CHAI"][0].numpy()
    mask = np.zeros((n, d), np.float32)
    it = iter(dr.rec)
    eps = []
    for t in range(steps):
        per = []
        for u in range(d - 1):
            per += [next(it) for _ in range(4 * M)]
        eps.append(scatter([p for p in per], mask, M))
        mask[np.arange(n), action[:, t].astype(int)] += 1
    assert next(it, None) is None
    out.update(x=x.numpy(), test_mask=test_mask.numpy(), fwd_xmean=np.stack(calls).astype(np.float32),
               reward_eps=np.stack(eps), im=res["im_CHAI"][0].numpy().astype(np.float32),
               R_hist=res["R_hist_CHAI"][0].numpy(), action=action,
               info_curve=res["information_curve_CHAI"][0, 0].numpy(), files=np.array(files), M=np.int64(M),
               hid=np.int64(H))
    np.savez_compressed(os.path.join(OUT, f"flow_active_reg_d{d}.npz"), **out)
    print("flow_active", "info curve", out["info_curve"], "first actions", action[:3, :4])


if __name__ == "__main__":
    gen_reward("reg", 12, 64, 24, 3, 2024, "flow_reward_reg_d12")
    gen_reward("van", 9, 72, 16, 2, 2025, "flow_reward_van_d9")
    gen_reward("reg", 12, 64, 24, 3, 2026, "flow_reward_quirk_reg", quirk=True)
    gen_active()
