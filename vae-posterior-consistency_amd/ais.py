"""Annealed importance sampling with adaptive-step HMC: the reference's src/utils/AIS.py on the persistent kernel of
csrc/vpc_ais.hip (engine="persistent") or, for every other Gaussian decoder, on the generic GEMM layer ops with the HMC
kernels of csrc/vpc_aisg.hip around them (engine="gemm").

    linear_schedule, sigmoidial_schedule, log_mean_exp    AIS.py:19-25, 65-77 (host side)
    ais_chains       one batch: the temperature loop of AIS.py:155-217 -> per-chain logw, z, epsilon, accept_hist
    ais_trajectory   AIS.py:94-234 (positional parameters and defaults of the reference), writes the reference's two files
    eval_ais         AIS.py:80-91

Quirks of the reference, kept and named:
  * `likelihood="reference"` (default): AIS.py:125 passes neg_gaussian_log_likelihood - the sum over all d columns of
    MINUS the Gaussian log-density, no mask - as the log likelihood, so the chain anneals towards p(z) p(x|z)^-1.
    `likelihood="corrected"` flips that one sign (real AIS); the arithmetic is otherwise identical.
  * chains are laid out by safe_repeat (chain c = row c % nb, sample c // nb), but the final latents are saved as
    `current_z.reshape(nb, n_sample, L)` (AIS.py:225): entry [i, s] of the saved tensor is chain i * n_sample + s, which
    belongs to row (i * n_sample + s) % nb, not to row i.  The saved file keeps that layout; `ais_chains` returns the
    chain-major [B, L] array, from which `z.view(n_sample, nb, L).transpose(0, 1)` is the per-row view.
  * ais_trajectory's model_loader call (AIS.py:120-121) has the wrong arity in the reference; here the keywords
    harness.model_loader needs are keyword arguments, and `model=` skips loading.

There is no CPU fallback: CPU tensors raise.  engine="persistent" (the default) covers the latent -> 50 -> 100 -> d sigmoid
chain with the constant x_logvar (obs_dim <= 128, or <= 64 for the mask-augmented classes; latent_dim <= 15) and raises for
every other model.  engine="gemm" covers every family whose decoder returns (mean, logvar) - what the reference's
ais_trajectory needs (AIS.py:125-140) - at obs_dim <= 1024, hidden width <= 512, latent_dim <= 64:
    REG_notMIWAE_v2 / notMIWAE_myversion   2 ELU layers, merged [x_mean | x_logvar] head, Sigmoid / Hardtanh(-10, 0)
    VAEFlow / REG_VAEFlow                  4 ELU layers, sigmoid mean head, logvar = -8
    Reg_EDDI_mnist / vanilla_EDDI_mnist    3 ReLU layers, sigmoid head, the scalar x_logvar
    Reg_VAE / vanilla_VAE (+ _mask), Reg_EDDI / vanilla_EDDI at any width: the 50-100 ReLU chain, the scalar x_logvar
and takes mask= [nb, d] (0/1): the likelihood of the observed columns only.  engine="auto": the persistent kernel where it
applies and no mask is given, else gemm.  MIWAE / Reg_MIWAE raise under every engine: their decoder returns three tensors
(a Student-t) and the reference's AIS cannot run on it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import VpcError, check, lib, ptr, stream_ptr
from .eddi_mnist import _EDDIMnistBase
from .flow import _FlowBase
from .models import _VAEBase
from .notmiwae import _NMBase

ENGINES = ("persistent", "gemm", "auto")

# Temperatures per launch when the caller does not say.  It has to come from a measurement of one launch at the largest
# benchmarked shape (tools/bench_ais.py "launch" records -> profiles/ais.jsonl); none has been taken yet,
# so there is no number here: None = the whole schedule in one launch.
DEFAULT_TEMPS_PER_LAUNCH = None


def linear_schedule(T):
    """T evenly spaced temperatures from 0 to 1 (AIS.py:19-20)."""
    return np.linspace(0.0, 1.0, num=T)


def sigmoidial_schedule(T, delta=4):
    """The sigmoid-shaped schedule of the BDMC paper, section 6 (AIS.py:65-77): a logistic curve over t = 1..T with
    slope delta, shifted and scaled so that it starts at 0 and ends at 1.  Returns a list of T floats."""
    e = np.exp(delta * (2.0 * np.arange(1, T + 1, dtype=np.float64) / T - 1.0))
    s = e / (1.0 + e)
    return [float(b) for b in (s - s[0]) / (s[-1] - s[0])]


def log_mean_exp(x):
    """log of the row means of exp(x) for x [rows, n], stabilised by the row maximum (AIS.py:23-25)."""
    top = x.max(dim=1).values
    return (x - top.unsqueeze(1)).exp().mean(dim=1).log() + top


def _decoder_image(model):
    """(decoder image, d, L, x_logvar) of a supported model; VpcError otherwise."""
    d, Ld = getattr(model, "obs_dim", None), getattr(model, "latent_dim", None)
    # _wide: the model runs on the generic GEMM path and has no packed decoder image.  That is obs_dim > 128 or
    # latent_dim > 15, and for the mask-augmented classes (encoder input [x*mask | mask]) already obs_dim > 64.
    if not isinstance(model, _VAEBase) or isinstance(model, _EDDIMnistBase) or getattr(model, "_wide", False) or \
            not lib().vpc_ais_applicable(1, int(d), int(Ld)):
        raise VpcError(
            "AIS covers the models whose decoder is the latent -> 50 -> 100 -> d sigmoid chain with the constant x_logvar "
            "on the register-chained kernels: Reg_VAE / vanilla_VAE and Reg_EDDI / vanilla_EDDI at obs_dim <= 128, "
            "Reg_VAE_mask / vanilla_VAE_mask at obs_dim <= 64, latent_dim <= 15: "
            f"got {type(model).__name__}(obs_dim={d}, latent_dim={Ld})")
    return model._dec_img(), d, Ld, model._x_logvar_value


def _decoder_chain(model):
    """(layers of linear.chain, d, L, x_logvar) of a model's decoder for the GEMM engine; x_logvar None = the chain's last
    layer is the merged [mean | logvar] head.  The layers are the model's own parameters (the views its API path runs
    on), not a packed copy: nothing here can go stale."""
    d, Ld = getattr(model, "obs_dim", None), getattr(model, "latent_dim", None)
    if isinstance(model, _NMBase):
        return model._chains()[1], d, Ld, None
    if isinstance(model, (_FlowBase, _VAEBase)):  # (_VAEBase: the dense classes at any width and both point-net pairs)
        return model._chains()[1], d, Ld, float(model.obs_logvar) if isinstance(model, _FlowBase) else model._x_logvar_value
    raise VpcError("AIS needs a decoder that returns a Gaussian (mean, logvar) (AIS.py:125-140): "
                   f"{type(model).__name__} has none (MIWAE / Reg_MIWAE return the three tensors of a Student-t)")


def _pick_engine(model, engine, mask):
    if engine not in ENGINES:
        raise ValueError(f"engine must be one of {ENGINES}")
    if engine == "persistent" and mask is not None:
        raise VpcError("mask= needs engine='gemm' (or 'auto'): the persistent kernel sums over all d columns")
    if engine != "auto":
        return engine
    if mask is None:
        try:
            _decoder_image(model)
            return "persistent"
        except VpcError:
            pass
    return "gemm"


def _run_gemm(model, x, mask, sched, T, B, nb, z0, v, u, seed, sign, leapfrog_steps, init_step_size, grad_clip, tpl):
    layers, d, Ld, xlv = _decoder_chain(model)
    n = len(layers)
    for w, b, _, _, _, _ in layers:
        L.require_cuda(w, b)
    Ks, Ns = (C.c_int * n)(*[int(l[2]) for l in layers]), (C.c_int * n)(*[int(l[3]) for l in layers])
    acts = (C.c_int * n)(*[int(l[4]) for l in layers])
    ws_, bs_ = L.ptr_array([l[0] for l in layers]), L.ptr_array([l[1] for l in layers])
    floats = int(lib().vpc_aisg_workspace_floats(B, Ld, n, Ns))
    work = torch.empty(max(floats, 4), device=x.device)
    j = 1
    while j < T:
        k = min(int(tpl), T - j)
        check(lib().vpc_aisg_run(ptr(x), ptr(mask), ws_, bs_, Ks, Ns, acts, n, int(layers[-1][5]),
                                 0.0 if xlv is None else float(xlv), ptr(sched), T, j, k, int(j == 1), ptr(work), floats,
                                 ptr(z0), ptr(v), ptr(u), int(seed), sign, int(leapfrog_steps), float(init_step_size),
                                 float(grad_clip), B, nb, d, Ld, stream_ptr()), "vpc_aisg_run")
        j += k
    r4 = lambda m: (m + 3) & ~3
    z = work[:B * Ld].view(B, Ld).clone()
    o = r4(B * Ld)
    eps, hist, logw = (work[o + i * r4(B):o + i * r4(B) + B].clone() for i in range(3))  # (not views: `work` is large)
    return logw, z, eps, hist


def ais_draws(B, latent_dim, T, seed, device="cuda"):
    """(z0 [B, L], v [T-1, B, L], u [T-1, B]): the draws ais_chains(seed=seed) generates inside the kernel."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise VpcError("this path runs only on the GPU (HIP kernels, no CPU fallback)")
    z0 = torch.empty(B, latent_dim, device=dev)
    v = torch.empty(T - 1, B, latent_dim, device=dev)
    u = torch.empty(T - 1, B, device=dev)
    check(lib().vpc_ais_draws(ptr(z0), ptr(v), ptr(u), B, latent_dim, T, int(seed), stream_ptr()), "vpc_ais_draws")
    return z0, v, u


def ais_chains(model, x, schedule, n_sample, mode="forward", post_z=None, likelihood="reference", seed=None, draws=None,
               init_step_size=0.01, leapfrog_steps=10, grad_clip=1e4, temps_per_launch=None, engine="persistent", mask=None):
    """One batch of AIS chains (AIS.py:155-217).  x [nb, d] on the GPU; B = nb * n_sample chains in safe_repeat order.
    engine: "persistent" | "gemm" | "auto" (module docstring); mask [nb, d] (0/1, gemm engine): the likelihood sums over
    the observed columns of each row only.
    draws: optional (z0 [B, L] or None, v [T-1, B, L] or None, u [T-1, B] or None) injected instead of the kernel's
    own Philox draws (seed; None = a fresh one from torch's generator).  mode="backward" starts from the repeated post_z
    [nb, L] (AIS.py:173).  Returns per-chain (logw [B], z [B, L], epsilon [B], accept_hist [B])."""
    if mode not in ("forward", "backward"):
        raise ValueError("Should have forward/backward mode")
    if likelihood not in ("reference", "corrected"):
        raise ValueError("likelihood must be 'reference' or 'corrected'")
    if not isinstance(x, torch.Tensor):
        raise VpcError("x must be a torch tensor on the GPU")
    L.require_cuda(x, post_z, mask)
    engine = _pick_engine(model, engine, mask)
    if engine == "persistent":
        img, d, Ld, xlv = _decoder_image(model)
        L.require_cuda(img)
    else:
        _, d, Ld, _ = _decoder_chain(model)
    if x.dim() != 2 or x.shape[1] != d:
        raise VpcError(f"x must be [nb, {d}]")
    dev = x.device
    x = x.float().contiguous()
    nb = x.shape[0]
    B = nb * int(n_sample)
    if mask is not None:
        if tuple(mask.shape) != (nb, d):
            raise VpcError(f"mask must be [{nb}, {d}]")
        mask = mask.to(dev).float().contiguous()
    sched = torch.as_tensor(np.asarray(schedule, dtype=np.float64), dtype=torch.float32).to(dev)
    T = sched.numel()
    if T < 2 or B < 1:
        raise VpcError("AIS needs at least two temperatures and one chain")
    z0 = v = u = None
    if draws is not None:
        z0, v, u = draws
    if mode == "backward":
        if post_z is None:
            raise ValueError("mode='backward' needs post_z")
        z0 = post_z.to(dev).float().repeat(n_sample, 1)
    for t, shape, name in ((z0, (B, Ld), "z0"), (v, (T - 1, B, Ld), "v"), (u, (T - 1, B), "u")):
        if t is not None:
            L.require_cuda(t)
            if tuple(t.shape) != shape:
                raise VpcError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
    z0, v, u = [None if t is None else t.float().contiguous() for t in (z0, v, u)]
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    tpl = temps_per_launch or DEFAULT_TEMPS_PER_LAUNCH or T - 1
    sign = 1.0 if likelihood == "reference" else -1.0
    if engine == "gemm":
        return _run_gemm(model, x, mask, sched, T, B, nb, z0, v, u, seed, sign, leapfrog_steps, init_step_size, grad_clip,
                         tpl)
    state = torch.empty(int(lib().vpc_ais_state_floats(B)), device=dev)
    j = 1
    while j < T:
        n = min(int(tpl), T - j)
        check(lib().vpc_ais_run(ptr(x), ptr(img), ptr(sched), T, j, n, int(j == 1), ptr(state), ptr(z0), ptr(v), ptr(u),
                                int(seed), sign, int(leapfrog_steps), float(init_step_size), float(grad_clip), float(xlv),
                                B, nb, d, Ld, stream_ptr()), "vpc_ais_run")
        j += n
    z = state[:16 * B].view(B, 16)[:, :Ld].contiguous()
    eps, hist, logw = (state[(16 + k) * B:(17 + k) * B] for k in range(3))
    return logw, z, eps, hist


def _paths(vae_type, data_type, missing_rate, max_epochs, stage):
    """AIS.py:230-233."""
    root = "experiments/" + vae_type + "/" + data_type
    tail = str(missing_rate) + "_missing/" + str(max_epochs) + "_epochs/" + stage
    return root + "/elbos/" + tail + "_ais.pt", root + "/latents/" + tail + "_ais_true_latents.pt"


def ais_trajectory(loader, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters, max_epochs,
                   vae_type, stage, num_samples, num_estimates, mode="forward", schedule=np.linspace(0., 1., 500),
                   n_sample=100, device=torch.device("cuda"), *, model=None, experiment_type="exp", reg_type="kl_reg",
                   alpha=1.0, p_missingness=30, likelihood="reference", seed=None, draws=None, init_step_size=0.01,
                   leapfrog_steps=10, grad_clip=1e4, temps_per_launch=None, engine="persistent", masks=None):
    """AIS.py:94-234.  loader yields (batch [nb, d], post_z); returns the reference's list of per-batch means and writes
    `<stage>_ais.pt` (their mean) and `<stage>_ais_true_latents.pt` ([sum nb, n_sample, L], the reference's reshape of
    the chain-major z - see the module docstring).  draws: one tuple per batch (a list), or None; masks: one [nb, d]
    mask per batch (a list), or None; seed: batch i uses seed + i."""
    device = torch.device(device)
    if device.type != "cuda":
        raise VpcError("this path runs only on the GPU (HIP kernels, no CPU fallback)")
    from .harness import _model_for_eval, _save
    model = _model_for_eval(model, device, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters,
                            max_epochs, num_samples, num_estimates, experiment_type, reg_type, vae_type, alpha, p_missingness)
    assert mode == "forward" or mode == "backward", "Should have forward/backward mode"
    model.eval()
    print("In %s mode" % mode)
    logws, latents = [], []
    for i, (batch, post_z) in enumerate(loader):
        nb = batch.size(0)
        logw, z, _, _ = ais_chains(model, batch.float().to(device), schedule, n_sample, mode=mode,
                                   post_z=post_z.to(device) if mode == "backward" else None, likelihood=likelihood,
                                   seed=None if seed is None else int(seed) + i, draws=None if draws is None else draws[i],
                                   init_step_size=init_step_size, leapfrog_steps=leapfrog_steps, grad_clip=grad_clip,
                                   temps_per_launch=temps_per_launch, engine=engine,
                                   mask=None if masks is None else masks[i])
        lw = log_mean_exp(logw.view(n_sample, -1).transpose(0, 1))  # AIS.py:220
        if mode == "backward":
            lw = -lw
        logws.append(lw.mean())
        latents.append(z.reshape(nb, n_sample, model.latent_dim))  # AIS.py:225
        print("last batch stats %.4f" % lw.mean().item())
    f_ais, f_lat = _paths(vae_type, data_type, missing_rate, max_epochs, stage)
    _save(torch.stack(logws).mean(), f_ais)
    _save(torch.cat(latents, 0), f_lat)
    return logws


def eval_ais(train_loader, valid_loader, test_loader, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type,
             training_parameters, max_epochs, vae_type, num_samples, num_estimates, mode="forward",
             schedule=np.linspace(0., 1., 500), n_sample=100, device=torch.device("cuda"), **kw):
    """AIS.py:80-91: each of the three arguments is a (loader, stage) pair."""
    for loader in [train_loader, valid_loader, test_loader]:
        loader, stage = loader
        ais_trajectory(loader, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters, max_epochs,
                       vae_type, stage, num_samples, num_estimates, mode=mode, schedule=schedule, n_sample=n_sample,
                       device=device, **kw)
