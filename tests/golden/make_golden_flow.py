"""Golden vectors for the flow path (VAEFlow / REG_VAEFlow, Data/imputation_args.json runs vanilla_flow* / reg_flow*),
produced by running the REFERENCE itself.

    cd <repo> && VPC_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_flow.py [--eval]

Authoring container only: imports the reference checkout (never copied, never shipped) and stores DATA only.

  flow_{reg,van}_d12.npz / _d40.npz   state_dict + key order, inputs (x, bool masks), the normal draw of every encoder
                                      call (peeked from torch's RNG), the forward outputs, the loss at alpha in
                                      {1.0, 0.5, 0.0} (reg) with every non-None parameter gradient, the evaluate stage
                                      (reg, d12: with gradients) and the llh_eval values.  d12: hid 64, B 37; d40: hid 72
                                      (ragged), B 64
  flow_quirk_reg.npz                  B = 1, the q pass with inside and outside draws, the p pass with every |eps| > 1:
                                      torch.any(inside) is false for that encoder call only (VAE.py:1698)
  flow_traj_{reg,van}_d12.npz         5 Adam steps as train.py:77-117 runs them, mask_p and draws recorded
  flow_eval_{reg,van}_d12.npz         (--eval) the reference's eval_vae (evaluate.py:136-297) on a checkpoint in its own
                                      naming scheme: the result file names and the values it wrote for several seeds
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ["VPC_REFERENCE"]
OUT = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
tv = types.ModuleType("torchvision")
tv.datasets = types.ModuleType("torchvision.datasets")
tv.transforms = types.ModuleType("torchvision.transforms")
sys.modules["torchvision"] = tv
sys.modules["torchvision.datasets"] = tv.datasets
sys.modules["torchvision.transforms"] = tv.transforms

from src.models.VAE import REG_VAEFlow, VAEFlow  # noqa: E402

TP = {"batch_size": 64, "patience": 100}
L = 10
FWD_REG = ["z_p", "z_log_prob_p", "x_mean_p", "x_logvar_p", "z_q", "z_log_prob_q", "x_mean_q", "x_logvar_q"]
FWD_VAN = ["z", "z_log_prob", "x_mean", "x_logvar"]


def peek_normals(shapes):
    st = torch.get_rng_state()
    eps = [torch.empty(s).normal_() for s in shapes]
    torch.set_rng_state(st)
    return eps


def sd_np(model):
    return {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}


def grads_np(model, tag):
    return {f"grad.{tag}.{k}": p.grad.detach().numpy().copy() for k, p in model.named_parameters()
            if p.grad is not None}


def make_inputs(B, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, d, generator=g)
    mask = torch.rand(B, d, generator=g) < 0.7
    mask_p = mask & (torch.rand(B, d, generator=g) < 0.5)
    return x, mask, mask_p


def _head(model, x, mask, extra):
    out = {"param." + k: v for k, v in sd_np(model).items()}
    out["keys"] = np.array(list(model.state_dict().keys()))
    out.update(x=x.numpy(), mask=mask.numpy(), hid=np.int64(model.hid_dim), **extra)
    return out


def gen_reg(d, H, B, seed, eval_grads=True, tag=None):
    torch.manual_seed(seed)
    model = REG_VAEFlow(d, H, 10, L, TP)
    x, mask, mask_p = make_inputs(B, d, seed + 1)
    out = _head(model, x, mask, {"mask_p": mask_p.numpy()})
    eps = peek_normals([(B, L)] * 2)  # encoder q, encoder p (forward order, VAE.py:2118-2121)
    for alpha in (1.0, 0.5, 0.0):
        st = torch.get_rng_state()
        model.zero_grad()
        o = model.forward(x, mask, mask_p)
        pl, tl = model.loss(x, o[6], o[7], o[4], o[5], o[2], o[3], o[0], o[1], mask, mask_p, alpha, stage="train")
        tl.backward()
        out[f"loss.a{alpha}"] = np.float64(tl.item())
        out.update(grads_np(model, f"a{alpha}"))
        torch.set_rng_state(st)
    if eval_grads:
        st = torch.get_rng_state()
        model.zero_grad()
        o = model.forward(x, mask, mask_p)
        pl, tl = model.loss(x, o[6], o[7], o[4], o[5], o[2], o[3], o[0], o[1], mask, mask_p, 0.5, stage="evaluate")
        tl.backward()
        out["loss.eval"] = np.float64(tl.item())
        out.update(grads_np(model, "eval"))
        torch.set_rng_state(st)
    with torch.no_grad():
        o = model.forward(x, mask, mask_p)
        for n, t in zip(FWD_REG, o):
            out["fwd." + n] = t.numpy()
        for stage in ("train", "evaluate"):
            r = model.loss(x, o[6], o[7], o[4], o[5], o[2], o[3], o[0], o[1], mask, mask_p, 0.5, llh_eval=True,
                           stage=stage)
            out[f"llh.{stage}"] = np.array([float(v) for v in r], dtype=np.float64)
    out["eps"] = np.stack([e.numpy() for e in eps])
    name = tag or f"flow_reg_d{d}"
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, {k: float(v) for k, v in out.items() if k.startswith("loss.")})


def gen_van(d, H, B, seed):
    torch.manual_seed(seed)
    model = VAEFlow(d, H, 10, L, TP)
    x, mask, _ = make_inputs(B, d, seed + 1)
    out = _head(model, x, mask, {})
    (eps,) = peek_normals([(B, L)])
    st = torch.get_rng_state()
    model.zero_grad()
    o = model.forward(x, mask)
    pl, tl = model.loss(x, o[2], o[3], o[0], o[1], mask)
    tl.backward()
    out["loss"] = np.float64(tl.item())
    out["print_loss"] = np.float64(pl.item())
    out.update(grads_np(model, "v"))
    torch.set_rng_state(st)
    with torch.no_grad():
        o = model.forward(x, mask)
        for n, t in zip(FWD_VAN, o):
            out["fwd." + n] = t.numpy()
        r = model.loss(x, o[2], o[3], o[0], o[1], mask, llh_eval=True)
        out["llh"] = np.array([float(v) for v in r], dtype=np.float64)
    out["eps"] = eps.numpy()[None]
    np.savez_compressed(os.path.join(OUT, f"flow_van_d{d}.npz"), **out)
    print("flow_van", d, out["loss"])


class _Inject:
    """Normal.rsample returns the given draws in order (the quirk case needs a p-pass draw with every |eps| > 1)."""

    def __init__(self, draws):
        self.draws = list(draws)

    def __enter__(self):
        self.orig = torch.distributions.Normal.rsample
        draws = self.draws
        torch.distributions.Normal.rsample = lambda self_, sample_shape=torch.Size(): draws.pop(0).clone()
        return self

    def __exit__(self, *a):
        torch.distributions.Normal.rsample = self.orig


def gen_quirk(d=12, H=64, seed=91):
    torch.manual_seed(seed)
    model = REG_VAEFlow(d, H, 10, L, TP)
    x, mask, mask_p = make_inputs(1, d, seed + 1)
    out = _head(model, x, mask, {"mask_p": mask_p.numpy()})
    eq = torch.tensor([[0.3, -1.7, 0.9, 2.2, -0.4, 1.0, -1.0, 0.05, 1.3, -0.8]])
    ep = torch.tensor([[1.2, -1.5, 2.0, -1.1, 1.01, -3.0, 1.4, -1.2, 2.5, -1.05]])
    for alpha in (1.0, 0.5):
        model.zero_grad()
        with _Inject([eq, ep]):
            o = model.forward(x, mask, mask_p)
        pl, tl = model.loss(x, o[6], o[7], o[4], o[5], o[2], o[3], o[0], o[1], mask, mask_p, alpha, stage="train")
        tl.backward()
        out[f"loss.a{alpha}"] = np.float64(tl.item())
        out.update(grads_np(model, f"a{alpha}"))
    for n, t in zip(FWD_REG, o):
        out["fwd." + n] = t.detach().numpy()
    out["eps"] = torch.stack([eq, ep]).numpy()
    np.savez_compressed(os.path.join(OUT, "flow_quirk_reg.npz"), **out)
    print("flow_quirk", {k: float(v) for k, v in out.items() if k.startswith("loss.")})


def gen_traj(kind, d=12, H=64, B=37, steps=5, seed=4545, alpha=0.5):
    torch.manual_seed(seed)
    model = (REG_VAEFlow if kind == "reg" else VAEFlow)(d, H, 10, L, TP)
    opt = torch.optim.Adam(model.parameters(), lr=0.001)  # train.py:21
    x, mask, _ = make_inputs(B, d, seed + 1)
    out = {"param0." + k: v for k, v in sd_np(model).items()}
    out.update(x=x.numpy(), mask=mask.numpy(), hid=np.int64(H), alpha=np.float64(alpha))
    g = torch.Generator().manual_seed(seed + 2)
    losses, eps_all, mp_all = [], [], []
    for s in range(steps):
        if kind == "reg":  # train.py:53-55, 77-81
            mask_p = mask & (torch.rand(B, d, generator=g) < 0.7)
            mp_all.append(mask_p.numpy())
            eps = peek_normals([(B, L)] * 2)
            o = model.forward(x, mask, mask_p)
            _, tl = model.loss(x, o[6], o[7], o[4], o[5], o[2], o[3], o[0], o[1], mask, mask_p, alpha, stage="train")
        else:  # train.py:82-85
            eps = peek_normals([(B, L)])
            o = model.forward(x, mask)
            _, tl = model.loss(x, o[2], o[3], o[0], o[1], mask)
        eps_all.append(np.stack([e.numpy() for e in eps]))
        opt.zero_grad()
        tl.backward()
        opt.step()
        losses.append(tl.item())
    out.update({"param5." + k: v for k, v in sd_np(model).items()})
    out.update(losses=np.array(losses, dtype=np.float64), eps=np.stack(eps_all))
    if mp_all:
        out["mask_p"] = np.stack(mp_all)
    np.savez_compressed(os.path.join(OUT, f"flow_traj_{kind}_d{d}.npz"), **out)
    print("flow_traj", kind, losses)


def gen_eval(kind, d=12, H=64, N=40, M=2, seeds=(0, 1, 2, 3, 4, 5), seed=808):
    """The reference's own eval_vae on a checkpoint written in its naming scheme (batches of 24 + 16 rows), repeated
    over several seeds: the spread of its Monte-Carlo estimate is the tolerance of the interop test."""
    import tempfile
    from src.experiment_main.evaluate import eval_vae
    torch.manual_seed(seed)
    vae_type = "reg_flow1" if kind == "reg" else "vanilla_flow1"
    model = (REG_VAEFlow if kind == "reg" else VAEFlow)(d, H, 10, L, TP)
    opt = torch.optim.Adam(model.parameters(), lr=0.003)
    x, mask, _ = make_inputs(N, d, seed + 1)
    for s in range(60):  # a few steps so that the imputations are not trivial
        if kind == "reg":
            mp = mask & (torch.rand(N, d) < 0.7)
            o = model.forward(x, mask, mp)
            _, tl = model.loss(x, o[6], o[7], o[4], o[5], o[2], o[3], o[0], o[1], mask, mp, 0.5)
        else:
            o = model.forward(x, mask)
            _, tl = model.loss(x, o[2], o[3], o[0], o[1], mask)
        opt.zero_grad(); tl.backward(); opt.step()
    out = {"param." + k: v for k, v in sd_np(model).items()}
    fam = "".join(c for c in "_".join(vae_type.split("_")[:2]) if not c.isdigit())
    loaders = [([(x[:24], mask[:24]), (x[24:], mask[24:])], "test")]
    vals = []
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for sub in ("checkpoints", "rest", "elbos"):
                os.makedirs(os.path.join("experiments", "exp", "toy", sub, fam))
            if kind == "reg":
                ck = f"experiments/exp/toy/checkpoints/{fam}/checkpoint_{vae_type}_0.5_30_kl_reg_40_missing_rate_full_reg_test.pt"
            else:
                ck = f"experiments/exp/toy/checkpoints/{fam}/checkpoint_{vae_type}_40_missing_rate_test.pt"
            torch.save(model.state_dict(), ck)
            for sd in seeds:
                torch.manual_seed(sd)
                np.random.seed(sd)
                eval_vae(loaders, 40, d, H, 10, M, L, "toy", TP, "exp", vae_type, 100, 1, 1, alpha=0.5,
                         p_missingness=30, reg_type="kl_reg")
                files = sorted(os.path.join(sub, fam, f) for sub in ("rest", "elbos")
                               for f in os.listdir(f"experiments/exp/toy/{sub}/{fam}"))
                assert len(files) == 4, files
                vals.append([torch.load(os.path.join("experiments/exp/toy", f)).item() for f in files])
            out["result_files"] = np.array([os.path.basename(f) for f in files])
            out["checkpoint_file"] = np.array(os.path.basename(ck))
        finally:
            os.chdir(cwd)
    out.update(x=x.numpy(), mask=mask.numpy(), values=np.array(vals, dtype=np.float64), M=np.int64(M), hid=np.int64(H))
    np.savez_compressed(os.path.join(OUT, f"flow_eval_{kind}_d{d}.npz"), **out)
    print("flow_eval", kind, out["result_files"], np.array(vals))


if __name__ == "__main__" and "--eval" in sys.argv:
    gen_eval("reg")
    gen_eval("van")
    sys.exit(0)

if __name__ == "__main__":
    gen_reg(12, 64, 37, 71)
    gen_reg(40, 72, 64, 72, eval_grads=False)
    gen_van(12, 64, 37, 81)
    gen_van(40, 72, 64, 82)
    gen_quirk()
    gen_traj("reg")
    gen_traj("van")
