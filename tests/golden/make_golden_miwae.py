"""Golden vectors for the MIWAE path (MIWAE / Reg_MIWAE, Data/imputation_args.json runs 1-6), produced by running the
REFERENCE itself.

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_miwae.py [--eval]

Authoring container only: imports the reference checkout (never copied, never shipped) and stores DATA only.

  miwae_{reg,van}_d{14,40}.npz   state_dict, inputs (x, bool masks), every normal draw (forward q / p, loss q / p), the
                                 forward outputs, the loss at alpha in {1.0, 0.5, 0.0} (reg) with every parameter
                                 gradient, the llh_eval outputs.  B > S and B not a multiple of S: the reference's
                                 row / sample pairing is exercised
  miwae_traj_{reg,van}_d14.npz   5 Adam steps as train.py:102-117 runs them
  miwae_eval_{reg,van}_d14.npz   (--eval) the reference's eval_miwae (evaluate.py:72-133) on a checkpoint in its own
                                 naming scheme, the result file name and the RMSE it wrote for several seeds (spread)
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("VPC_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
tv = types.ModuleType("torchvision")
tv.datasets = types.ModuleType("torchvision.datasets")
tv.transforms = types.ModuleType("torchvision.transforms")
sys.modules["torchvision"] = tv
sys.modules["torchvision.datasets"] = tv.datasets
sys.modules["torchvision.transforms"] = tv.transforms

from src.models.VAE import MIWAE, Reg_MIWAE  # noqa: E402

TP = {"batch_size": 64, "patience": 100}


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


def gen_reg(d, L, S, B, seed, alphas=(1.0, 0.5, 0.0)):
    torch.manual_seed(seed)
    model = Reg_MIWAE(d, 500, 10, L, TP, S, 1)
    x, mask, mask_p = make_inputs(B, d, seed + 1)
    out = {"param." + k: v for k, v in sd_np(model).items()}
    out.update(x=x.numpy(), mask=mask.numpy(), mask_p=mask_p.numpy(), S=np.int64(S), L=np.int64(L))
    eps = peek_normals([(B, S, L)] * 4)  # forward q, forward p, loss q, loss p
    names = ["mean_p", "scale_p", "x_mean_p", "x_scale_p", "deg_free_p", "mean_q", "scale_q", "x_mean_q", "x_scale_q",
             "deg_free_q"]
    for alpha in alphas:
        st = torch.get_rng_state()
        model.zero_grad()
        o = model.forward(x, mask, mask_p)
        pl, tl = model.loss(x, o[2], o[3], o[4], o[0], o[1], o[7], o[8], o[9], o[5], o[6], mask, mask_p, 7, alpha=alpha)
        tl.backward()
        out[f"loss.a{alpha}"] = np.float64(tl.item())
        out.update(grads_np(model, f"a{alpha}"))
        torch.set_rng_state(st)
    o = model.forward(x, mask, mask_p)
    for n, t in zip(names, o):
        out["fwd." + n] = t.detach().numpy()
    out["eps"] = np.stack([e.numpy() for e in eps])
    eps_llh = peek_normals([(B, S, L)] * 2)
    with torch.no_grad():
        xm, tl, t3 = model.loss(x, o[2], o[3], o[4], o[0], o[1], o[7], o[8], o[9], o[5], o[6], mask, mask_p, 7,
                                alpha=0.5, llh_eval=True)
    out.update(llh_xm=xm.numpy(), llh_loss=np.float64(tl.item()), llh_third=np.float64(t3.item()),
               eps_llh=np.stack([e.numpy() for e in eps_llh]))
    np.savez_compressed(os.path.join(OUT, f"miwae_reg_d{d}.npz"), **out)
    print("miwae_reg", d, {k: float(v) for k, v in out.items() if k.startswith("loss.")})


def gen_van(d, L, S, B, seed):
    torch.manual_seed(seed)
    model = MIWAE(d, 500, 10, L, TP, S, 1)
    x, mask, _ = make_inputs(B, d, seed + 1)
    out = {"param." + k: v for k, v in sd_np(model).items()}
    out.update(x=x.numpy(), mask=mask.numpy(), S=np.int64(S), L=np.int64(L))
    eps = peek_normals([(B, S, L)] * 2)  # forward, loss
    model.zero_grad()
    o = model.forward(x, mask)
    pl, tl = model.loss(x, o[2], o[3], o[4], o[0], o[1], mask, 3)
    tl.backward()
    out["loss"] = np.float64(tl.item())
    out.update(grads_np(model, "v"))
    for n, t in zip(["mean", "scale", "x_mean", "x_scale", "deg_free"], o):
        out["fwd." + n] = t.detach().numpy()
    out["eps"] = np.stack([e.numpy() for e in eps])
    (eps_llh,) = peek_normals([(B, S, L)])
    with torch.no_grad():
        xm, tl2, t3 = model.loss(x, o[2], o[3], o[4], o[0], o[1], mask, 3, llh_eval=True)
    out.update(llh_xm=xm.numpy(), llh_loss=np.float64(tl2.item()), llh_third=np.float64(t3.item()),
               eps_llh=eps_llh.numpy()[None])
    np.savez_compressed(os.path.join(OUT, f"miwae_van_d{d}.npz"), **out)
    print("miwae_van", d, out["loss"])


def gen_traj(kind, d=14, L=10, S=5, B=13, steps=5, seed=4343):
    torch.manual_seed(seed)
    model = (Reg_MIWAE if kind == "reg" else MIWAE)(d, 500, 10, L, TP, S, 1)
    opt = torch.optim.Adam(model.parameters(), lr=0.001)  # train.py:21
    x, mask, _ = make_inputs(B, d, seed + 1)
    out = {"param0." + k: v for k, v in sd_np(model).items()}
    out.update(x=x.numpy(), mask=mask.numpy(), S=np.int64(S), L=np.int64(L))
    g = torch.Generator().manual_seed(seed + 2)
    losses, eps_all, mp_all = [], [], []
    for s in range(steps):
        if kind == "reg":
            mask_p = mask & (torch.rand(B, d, generator=g) < 0.5)
            mp_all.append(mask_p.numpy())
            eps = peek_normals([(B, S, L)] * 4)
            o = model.forward(x, mask, mask_p)
            _, tl = model.loss(x, o[2], o[3], o[4], o[0], o[1], o[7], o[8], o[9], o[5], o[6], mask, mask_p, s + 1,
                               beta_annealing=False, beta=1.0, alpha=0.5)
        else:
            eps = peek_normals([(B, S, L)] * 2)
            o = model.forward(x, mask)
            _, tl = model.loss(x, o[2], o[3], o[4], o[0], o[1], mask, s + 1)
        eps_all.append(np.stack([e.numpy() for e in eps]))
        opt.zero_grad()
        tl.backward()
        opt.step()
        losses.append(tl.item())
    out.update({"param5." + k: v for k, v in sd_np(model).items()})
    out.update(losses=np.array(losses, dtype=np.float64), eps=np.stack(eps_all))
    if mp_all:
        out["mask_p"] = np.stack(mp_all)
    np.savez_compressed(os.path.join(OUT, f"miwae_traj_{kind}_d{d}.npz"), **out)
    print("miwae_traj", kind, losses)


def gen_eval(kind, d=14, L=10, N=24, valid_k=200, M=2, seeds=(0, 1, 2, 3, 4, 5), seed=707):
    """The reference's own eval_miwae on a checkpoint written in its naming scheme (two batches of 16 + 8 rows), repeated
    over several seeds: the spread of its Monte-Carlo estimate is the tolerance of the interop test."""
    import tempfile
    from src.experiment_main.evaluate import eval_miwae
    torch.manual_seed(seed)
    vae_type = "reg_MIWAE1" if kind == "reg" else "vanilla_MIWAE1"
    model = (Reg_MIWAE if kind == "reg" else MIWAE)(d, 500, 10, L, TP, 20, 1)
    opt = torch.optim.Adam(model.parameters(), lr=0.003)
    x, mask, _ = make_inputs(N, d, seed + 1)
    for s in range(60):  # a few steps so that the imputations are not trivial
        if kind == "reg":
            mp = mask & (torch.rand(N, d) < 0.5)
            o = model.forward(x, mask, mp)
            _, tl = model.loss(x, o[2], o[3], o[4], o[0], o[1], o[7], o[8], o[9], o[5], o[6], mask, mp, s + 1, alpha=0.5)
        else:
            o = model.forward(x, mask)
            _, tl = model.loss(x, o[2], o[3], o[4], o[0], o[1], mask, s + 1)
        opt.zero_grad(); tl.backward(); opt.step()
    out = {"param." + k: v for k, v in sd_np(model).items()}
    fam = "".join(c for c in vae_type if not c.isdigit())
    loaders = [([(x[:16], mask[:16]), (x[16:], mask[16:])], "test")]
    rmses = []
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for sub in ("checkpoints", "rest"):
                os.makedirs(os.path.join("experiments", "exp", "toy", sub, fam))
            if kind == "reg":
                ck = f"experiments/exp/toy/checkpoints/{fam}/checkpoint_{vae_type}_0.5_30_kl_reg_40_missing_rate_full_reg_test.pt"
            else:
                ck = f"experiments/exp/toy/checkpoints/{fam}/checkpoint_{vae_type}_40_missing_rate_test.pt"
            torch.save(model.state_dict(), ck)
            for sd in seeds:
                torch.manual_seed(sd)
                np.random.seed(sd)
                eval_miwae(loaders, 40, d, 500, 10, M, L, "toy", TP, "exp", vae_type, 100, valid_k, 1, alpha=0.5,
                           p_missingness=30, reg_type="kl_reg")
                files = os.listdir(f"experiments/exp/toy/rest/{fam}")
                assert len(files) == 1, files
                rmses.append(torch.load(os.path.join(f"experiments/exp/toy/rest/{fam}", files[0])).item())
            out["result_file"] = np.array(files[0])
            out["checkpoint_file"] = np.array(os.path.basename(ck))
        finally:
            os.chdir(cwd)
    out.update(x=x.numpy(), mask=mask.numpy(), rmse=np.array(rmses, dtype=np.float64), valid_k=np.int64(valid_k),
               M=np.int64(M), L=np.int64(L))
    np.savez_compressed(os.path.join(OUT, f"miwae_eval_{kind}_d{d}.npz"), **out)
    print("miwae_eval", kind, rmses, files[0])


if __name__ == "__main__" and "--eval" in sys.argv:
    gen_eval("reg")
    gen_eval("van")
    sys.exit(0)

if __name__ == "__main__":
    gen_reg(14, 10, 5, 13, 51)
    gen_reg(40, 6, 3, 8, 52)
    gen_van(14, 10, 5, 13, 61)
    gen_van(40, 6, 3, 8, 62)
    gen_traj("reg")
    gen_traj("van")
