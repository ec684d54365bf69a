"""Active variable selection (BASELINE config 5): the information reward of
src/experiment_main/evaluate.py:514-634 on the GPU.

`reward_matrix` replaces the whole candidate loop of active_learning_func (evaluate.py:424-433) by three kernel
launches (vpc_reward_matrix for the plain Reg_VAE / vanilla_VAE with obs_dim <= 128; vpc_reward_matrix_ex for the
mask-augmented, the wide and the EDDI models); `R_lindley_chain`, `chaini_I`, `chaini_II` keep the reference's
signatures so that evaluate.py can call them unchanged.

The flow models (VAEFlow / REG_VAEFlow) take the ratio-version reward of evaluate.py:637-708 instead:
`flow_reward_matrix` (vpc_flow_reward_matrix, csrc/vpc_flowreward.hip), the drop-ins `R_lindley_chain_ratio_version`,
`chaini_I_ratio_version`, `chaini_II_ratio_version`, and the loop `active_learning_flow`.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib as L
from ._lib import check, lib, ptr, stream_ptr
from .ensemble import W23_FLOATS, EDDIEnsembleAcquirer, EnsembleAcquirer, MaskEnsembleAcquirer
from .harness import _save_results, _sweep_configs, _sweep_models, draw_mask_p, eval_groups, family_eval_groups, model_loader
from .images import PackedImage
from .ops import _f32c, as_mask_u8, pack_weights


# first-layer kinds of vpc_reward_matrix_ex (include/vpc.h)
REWARD_DENSE, REWARD_DENSE_MASK, REWARD_POINTNET = 0, 1, 2
_H1, _H2 = 100, 50


def _is_pointnet(vae):
    from .eddi import _EDDIBase
    return isinstance(vae, _EDDIBase)


def _is_flow(vae):
    from .flow import _FlowBase
    return isinstance(vae, _FlowBase)


def _w23_image(vae):
    """[W2 | W3] of the encoder, packed as the encoder kernels' image holds it.  Models with an encoder image (plain and
    mask-augmented VAEs with an input of <= 128 columns) lend theirs; the wide models and the EDDI trunk (pnp_encoder2,
    whose own image is never packed) get a W2/W3-only image of their own, re-packed when the parameter key changes
    (images.py).  Layers 2-3 do not depend on the input width, so the tables of any small layout pack it."""
    flat = vae.flatten_parameters()
    L.require_cuda(flat)
    if not _is_pointnet(vae) and not vae._wide:
        return vae._enc_img()[vae._lay().enc_img - W23_FLOATS:]
    img = vae.__dict__.get("_w23_img")
    if img is None or img.buf.device != flat.device:
        lay = L.layout(16, vae.latent_dim)
        o = lay.enc_img - W23_FLOATS
        w2 = _H1 * 16 + _H1  # flat offset of seq_encoder.2.weight in that layout
        n23 = _H2 * _H1 + _H2 + 2 * vae.latent_dim * (_H2 + 1)
        idx = torch.from_numpy(lay.pack_idx[w2:w2 + n23] - o).to(flat.device)
        lo = sum(p.numel() for p in vae.trainable()[:2])
        img = PackedImage(torch.from_numpy(lay.img_template[o:lay.enc_img].copy()).to(flat.device),
                          lambda fl, buf: pack_weights(fl[lo:lo + n23], idx, buf))
        vae.__dict__["_w23_img"] = img
    return img.get(vae._param_key(), flat)


def reward_matrix(vae, x, mask, im):
    """R [n, d-1]: reward of revealing feature u for row n (-1e4 where already observed).
    x [n, d]; mask [n, d] (bool / float 0-1 / uint8); im [M, n, d] MC imputations; target = last column.
    Every 'reg_vae*' / 'vanilla_vae*' (mask-augmented and wide included) and '*_EDDI*' model of model_loader with
    latent_dim <= 15."""
    L.require_cuda(x, im)
    if _is_flow(vae):
        return flow_reward_matrix(vae, x, mask, im)
    if getattr(vae, "_eddi_mnist", False):
        raise L.VpcError("reward_matrix: Reg_EDDI_mnist / vanilla_EDDI_mnist are not supported (active learning at image "
                         "width is not a reference configuration)")
    if vae.latent_dim > 15:
        raise L.VpcError("reward_matrix: latent_dim <= 15 is supported (the mean / logvar heads are one 16-row tile)")
    if _is_pointnet(vae) or vae.mask_augm or vae._wide:
        return _reward_matrix_ex(vae, x, mask, im)
    n, d = x.shape
    M = im.shape[0]
    lay = vae._lay()
    dev = x.device
    vae._images()
    w1, b1 = vae.trainable()[0], vae.trainable()[1]
    sizes = [C.c_long() for _ in range(3)]
    check(lib().vpc_reward_scratch(n, d, M, *[C.byref(s) for s in sizes]), "vpc_reward_scratch")
    pre = torch.empty(sizes[0].value, device=dev)
    stat = torch.empty(sizes[1].value, device=dev)
    w1t = torch.empty(sizes[2].value, device=dev)
    R = torch.empty(n, d - 1, device=dev)
    check(lib().vpc_reward_matrix(ptr(_f32c(x)), ptr(as_mask_u8(mask.to(dev))), ptr(_f32c(im)), ptr(w1.data), ptr(b1.data),
                                  ptr(vae._enc_img()), ptr(pre), ptr(stat), ptr(w1t), ptr(R), n, d, lay.L, M,
                                  stream_ptr()), "vpc_reward_matrix")
    return R


def _reward_matrix_ex(vae, x, mask, im):
    """reward_matrix for the mask-augmented, wide and EDDI encoders (vpc_reward_matrix_ex)."""
    n, d = x.shape
    M = im.shape[0]
    dev = x.device
    w23 = _w23_image(vae)
    t = vae.trainable()
    w1, b1 = t[0], t[1]
    K, AC = 0, None
    if _is_pointnet(vae):
        from .eddi import eddi_fold
        kind, K = REWARD_POINTNET, vae.emb_dim
        AC = torch.empty(2, K, d, device=dev)
        eddi_fold(*[p.data for p in t[12:16]], AC, d, K)
    else:
        kind = REWARD_DENSE_MASK if vae.mask_augm else REWARD_DENSE
    sizes = [C.c_long() for _ in range(3)]
    check(lib().vpc_reward_scratch_ex(kind, n, d, M, K, *[C.byref(s) for s in sizes]), "vpc_reward_scratch_ex")
    pre = torch.empty(sizes[0].value, device=dev)
    stat = torch.empty(sizes[1].value, device=dev)
    w1t = torch.empty(sizes[2].value, device=dev)
    R = torch.empty(n, d - 1, device=dev)
    check(lib().vpc_reward_matrix_ex(kind, ptr(_f32c(x)), ptr(as_mask_u8(mask.to(dev))), ptr(_f32c(im)), ptr(w1.data),
                                     ptr(b1.data), ptr(AC), K, ptr(w23), ptr(pre), ptr(stat), ptr(w1t), ptr(R), n, d,
                                     vae.latent_dim, M, stream_ptr()), "vpc_reward_matrix_ex")
    return R


# ------------------------------------------------------------------------------------------------ flow models
FLOW_REWARD_WS_FLOATS = 64 << 20  # default bound of the per-chunk workspace (256 MB)


def flow_reward_chunk(n, d, hid, M, budget_floats=FLOW_REWARD_WS_FLOATS):
    """Candidates per chunk so that the chunk's part of the workspace stays within `budget_floats`."""
    per_u = 2 * M * n * (((hid + 3) & ~3) + 100 + 20) + M * n + 4 * M
    return max(1, min(d - 1, budget_floats // per_u))


def flow_reward_draws(n, d, M, seed, device=None):
    """eps [d-1, M, 4, n, 10] ~ N(0, 1): the draws flow_reward_matrix(seed=seed) uses (vpc_flow_reward_draws)."""
    dev = torch.device(device) if device is not None else torch.device("cuda")
    eps = torch.empty(d - 1, M, 4, n, 10, device=dev)
    check(lib().vpc_flow_reward_draws(ptr(eps), n, d, M, int(seed), stream_ptr()), "vpc_flow_reward_draws")
    return eps


def flow_reward_matrix(vae, x, mask, im, eps=None, seed=None, chunk=None):
    """R [n, d-1] of a VAEFlow / REG_VAEFlow: the reward of evaluate.py:637-708 for every candidate of every row
    (-1e4 where already observed), vpc_flow_reward_matrix.  x [n, d]; mask [n, d]; im [M, n, d]; target = last column.
    eps: the draws of the 4 encoder calls per (candidate, sample) as a dense [d-1, M, 4, n, 10] tensor (call order Ia,
    Ib, IIa, IIb; rows outside loc(u) ignored); None: drawn on the device from `seed` (None: torch's generator picks
    one).  chunk: candidates per pass through the workspace (None: flow_reward_chunk); R does not depend on it."""
    if not _is_flow(vae):
        raise TypeError("flow_reward_matrix supports VAEFlow and REG_VAEFlow")
    L.require_cuda(x, im, eps)
    n, d = x.shape
    M = im.shape[0]
    hid = vae.hid_dim
    dev = x.device
    if d != vae.obs_dim or tuple(im.shape) != (M, n, d) or tuple(mask.shape) != (n, d):
        raise L.VpcError(f"flow_reward_matrix: x {tuple(x.shape)}, mask {tuple(mask.shape)}, im {tuple(im.shape)} do "
                         f"not fit obs_dim {vae.obs_dim}")
    if hid > 512:
        raise L.VpcError(f"flow_reward_matrix: hid_dim {hid} > 512 is not supported")
    if eps is not None and tuple(eps.shape) != (d - 1, M, 4, n, 10):
        raise L.VpcError(f"flow_reward_matrix: eps {tuple(eps.shape)}, expected {(d - 1, M, 4, n, 10)}")
    if eps is None and seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    chunk = flow_reward_chunk(n, d, hid, M) if chunk is None else int(chunk)
    v = vae._views()
    size = C.c_long()
    check(lib().vpc_flow_reward_scratch(n, d, hid, M, chunk, C.byref(size)), "vpc_flow_reward_scratch")
    ws = torch.empty(size.value, device=dev)
    R = torch.empty(n, d - 1, device=dev)
    mf = _f32c((mask.to(dev) != 0))
    check(lib().vpc_flow_reward_matrix(ptr(_f32c(x)), ptr(mf), ptr(_f32c(im)), *[ptr(v[k]) for k in vae._ENC_NAMES],
                                       ptr(None if eps is None else _f32c(eps)), int(seed or 0), ptr(ws), size.value,
                                       ptr(R), n, d, hid, M, chunk, stream_ptr()), "vpc_flow_reward_matrix")
    return R


def R_lindley_chain_ratio_version(i, x, mask, M, vae, im, loc, eps=None):
    """Same signature / result as evaluate.py:637-665 (rows `loc`, candidate `i`).  Prefer flow_reward_matrix: it
    returns every candidate of every row for the price of this one call.  eps (an addition): the candidate's draws
    [M, 4, len(loc), 10] in call order."""
    loc_t = torch.as_tensor(loc, device=x.device, dtype=torch.long)
    dense = None
    if eps is not None:
        dense = torch.zeros(x.shape[1] - 1, *eps.shape, device=x.device)
        dense[i] = eps
    R = flow_reward_matrix(vae, x[loc_t].float(), mask[loc_t], im[:M][:, loc_t].float(), eps=dense)
    return R[:, i]


def _ratio(x, mask, i, vae, eps, target_observed):
    tm = mask.clone().float()
    if target_observed:
        tm[:, -1] = 1
    e = (None, None) if eps is None else eps
    with torch.no_grad():
        _, lp = vae._encode(x, tm, eps=e[0])
        tm[:, i] = 1
        _, lp_i = vae._encode(x, tm, eps=e[1])
    return torch.abs(lp - lp_i).sum(1)


def chaini_I_ratio_version(x, mask, i, vae, eps=None):
    """evaluate.py:669-684 on the API path: two vae.encoder calls.  eps (an addition): their draws [2, rows, 10]."""
    return _ratio(x, mask, i, vae, eps, False)


def chaini_II_ratio_version(x, mask, i, vae, eps=None):
    """evaluate.py:688-708: the same with the target marked observed."""
    return _ratio(x, mask, i, vae, eps, True)


def R_lindley_chain(i, x, mask, M, vae, im, loc):
    """Same signature / result as evaluate.py:514-542 (rows `loc`, candidate `i`).  Prefer reward_matrix: it
    returns every candidate of every row for the price of this one call."""
    loc_t = torch.as_tensor(loc, device=x.device, dtype=torch.long)
    R = reward_matrix(vae, x[loc_t], mask[loc_t], im[:M][:, loc_t])
    return R[:, i]


def _kl(mean, logvar, mean_i, logvar_i):
    # evaluate.py:582-583: first term divided by v = exp(logvar / 2), as in the reference
    return 0.5 * torch.sum(torch.square(mean_i - mean) / torch.exp(logvar / 2) + torch.exp(logvar_i - logvar) - 1.0
                           - logvar_i + logvar, 1)


def chaini_I(x, mask, i, vae):
    """evaluate.py:546-586 on the encoder kernels (API path)."""
    tm = mask.clone()
    with torch.no_grad():
        _, mean, logvar = vae.encoder(x, tm, sample=False)
        tm[:, i] = 1
        _, mean_i, logvar_i = vae.encoder(x, tm, sample=False)
    return _kl(mean, logvar, mean_i, logvar_i)


def chaini_II(x, mask, i, vae):
    """evaluate.py:590-634."""
    tm = mask.clone()
    tm[:, -1] = 1
    with torch.no_grad():
        _, mean, logvar = vae.encoder(x, tm, sample=False)
        tm[:, i] = 1
        _, mean_i, logvar_i = vae.encoder(x, tm, sample=False)
    return _kl(mean, logvar, mean_i, logvar_i)


# ------------------------------------------------------------------------------------------------ the acquisition loop
def active_result_paths(experiment_type, data_type, vae_type, missing_rate, alpha=1.0, p_missingness=30, reg_type="ml_reg"):
    """The four files active_learning_func writes (evaluate.py:457-511), reference naming."""
    fam = "".join(c for c in "_".join(vae_type.split("_")[:2]) if not c.isdigit())
    rest = os.path.join("experiments", experiment_type, data_type, "rest", fam)
    if "vanilla" in vae_type:
        mk = lambda key, sep: os.path.join(rest, f"{vae_type}_{missing_rate}_missing_rate{sep}UCI_{key}_default_test.pt")  # noqa: E731
        return dict(information_curve_CHAI=mk("information_curve_CHAI", "_"), action_CHAI=mk("action_CHAI", "__"),
                    R_hist_CHAI=mk("R_hist_CHAI", "__"), im_CHAI=mk("im_CHAI", "__"))
    suf = f"_{alpha}_{p_missingness}_{reg_type}_{missing_rate}_missing_rate_default_full_reg_test.pt"
    return {k: os.path.join(rest, f"{vae_type}_UCI_{k}{suf}")
            for k in ("information_curve_CHAI", "action_CHAI", "R_hist_CHAI", "im_CHAI")}


def mc_forward(model, x, mask, mask_p, M, stage="evaluate"):
    """x_mean_q of M independent forward passes as ONE batched pass over M stacked copies of the rows (the eps of
    Normal.rsample are i.i.d. per row, so M calls of model.forward on n rows == one call on M n rows): [M, n, d]."""
    n, d = x.shape
    xr, mr = x.repeat(M, 1), mask.repeat(M, 1)
    o = model.forward(xr, mr, mask_p.repeat(M, 1), stage) if model.regularised else model.forward(xr, mr)
    return o[model.X_MEAN_Q].reshape(M, n, d)


def active_learning_func(data_loader_train, test_data, test_mask, missing_rate, obs_dim, hid_dim, K, M, latent_dim,
                         data_type, training_parameters, experiment_type, vae_type, max_epochs, valid_k, num_estimates,
                         device=None, alpha=1.0, stage="evaluate", p_missingness=30, reg_type="ml_reg", beta=1.0,
                         beta_annealing=False, alpha_annealing=True, Repeat=5, model=None, save=True, verbose=False,
                         _forward=None, max_steps=None):
    """Active variable selection, src/experiment_main/evaluate.py:300-511 (same positional signature; `model`, `save`,
    `verbose`, `_forward`, `max_steps` (stop after that many acquisitions; the rest of the outputs stays zero) are additions).  Per repeat: all features start unobserved (the target - last column - stays
    unobserved throughout); at each of the obs_dim - 1 steps M Monte-Carlo forward passes impute the rows (`im`), the
    information reward of revealing each candidate feature is evaluated for every row - ONE vpc_reward_matrix call instead
    of the reference's (obs_dim - 1) R_lindley_chain calls with 4 M encoder passes each - the best candidate per row is
    revealed (argmax, evaluate.py:435-440), and the target MSE of M further passes goes to the information curve.
    The M passes run as one batched forward (mc_forward).  `_forward(mask) -> x_mean_q [n, d]` replaces a single forward
    pass (tests replay the outputs recorded from the reference, whose eps come from the global RNG).
    Returns dict(information_curve_CHAI [Repeat, n, d], action_CHAI [Repeat, n, d-1], R_hist_CHAI [Repeat, d-1, n, d-1],
    im_CHAI [Repeat, d-1, M, n, d]) and (save=True) writes the reference's four files."""
    if _is_flow(model):
        raise NotImplementedError("active_learning_func: the flow models' reward (R_lindley_chain_ratio_version, "
                                  "evaluate.py) is not on the accelerated path")

    def load():
        return model_loader("test", obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters,
                            max_epochs, valid_k, num_estimates, experiment_type, reg_type, vae_type, alpha=alpha,
                            p_missingness=p_missingness, alpha_annealing=alpha_annealing)

    def passes(mdl, x, cur_mask, mask_p):
        if _forward is not None:
            return torch.stack([_forward(cur_mask).to(x.device) for _ in range(M)], 0)
        return mc_forward(mdl, x, cur_mask, mask_p, M, stage)

    out = _acquisition_loop(test_data, test_mask, obs_dim, M, device, p_missingness, Repeat, model, load, passes,
                            lambda mdl, x, mask, im, t: reward_matrix(mdl, x, mask, im), verbose, max_steps)
    return _save_active(out, save, experiment_type, data_type, vae_type, missing_rate, alpha, p_missingness, reg_type)


def _acquisition_loop(test_data, test_mask, obs_dim, M, device, p_missingness, Repeat, model, load, passes, reward,
                      verbose, max_steps):
    """The loop body of evaluate.py:340-455 shared by active_learning_func and active_learning_flow.
    load() -> a model for a repeat without one; passes(mdl, x, mask, mask_p) -> x_mean [M, n, d];
    reward(mdl, x, mask, im, step) -> R [n, d-1]."""
    dev = torch.device(device) if device is not None else torch.device("cuda")
    n_test, d = test_data.shape[0], obs_dim
    info = torch.zeros(Repeat, n_test, d)
    action = torch.zeros(Repeat, n_test, d - 1)
    R_hist = torch.zeros(Repeat, d - 1, n_test, d - 1)
    im_hist = torch.zeros(Repeat, d - 1, M, n_test, d)
    x = test_data.reshape(-1, d).float().to(dev)
    tmask = test_mask.to(dev)
    eye = torch.eye(d, device=dev)
    with torch.no_grad():
        for r in range(Repeat):
            mdl = (load() if model is None or r > 0 else model).to(dev)
            mask_p = draw_mask_p(mdl, tuple(test_data.shape), tmask, p_missingness, dev)  # evaluate.py:349-350
            mask = torch.zeros(n_test, d, device=dev)

            def target_mse(xm):  # mean over the M passes of F.mse_loss on the target column (evaluate.py:390-392)
                return ((xm[:, :, -1] - x[None, :, -1]) ** 2).mean(1).mean()

            info[r, :, 0] = target_mse(passes(mdl, x, mask, mask_p)).cpu()
            for t in range(d - 1 if max_steps is None else min(max_steps, d - 1)):
                if verbose:
                    print("Repeat = {:.1f}".format(r)); print("Strategy = {:.1f}".format(2)); print("Step = {:.1f}".format(t))
                im = passes(mdl, x, mask, mask_p)
                R = reward(mdl, x, mask, im, t)
                i_opt = R.argmax(1)
                mask = mask + eye[i_opt]
                info[r, :, t + 1] = target_mse(passes(mdl, x, mask, mask_p)).cpu()
                action[r, :, t] = i_opt.cpu().float()
                R_hist[r, t] = R.cpu()
                im_hist[r, t] = im.cpu()
    return dict(information_curve_CHAI=info, action_CHAI=action, R_hist_CHAI=R_hist, im_CHAI=im_hist)


def _save_active(out, save, experiment_type, data_type, vae_type, missing_rate, alpha, p_missingness, reg_type):
    if save:
        _save_results(out, active_result_paths(experiment_type, data_type, vae_type, missing_rate, alpha, p_missingness,
                                               reg_type))
    return out


def active_learning_flow(data_loader_train, test_data, test_mask, missing_rate, obs_dim, hid_dim, K, M, latent_dim,
                         data_type, training_parameters, experiment_type, vae_type, max_epochs, valid_k, num_estimates,
                         device=None, alpha=1.0, stage="evaluate", p_missingness=30, reg_type="ml_reg", beta=1.0,
                         beta_annealing=False, alpha_annealing=True, Repeat=5, model=None, save=True, verbose=False,
                         _forward=None, max_steps=None, _reward_eps=None, seed=None):
    """The flow branch of active_learning_func (evaluate.py:300-511 with 'flow' in vae_type: forwards :395-402, reward
    :420-422): same positional signature, outputs and file names, for a VAEFlow / REG_VAEFlow passed as `model=` (every
    repeat uses it: model_loader does not build flow models).  The reward of all candidates is one flow_reward_matrix call
    per step.  The M Monte-Carlo forwards are M model.forward calls (torch.any(inside) is per encoder call).
    `_forward(mask) -> x_mean [n, d]` replaces one forward; `_reward_eps(step) -> eps [d-1, M, 4, n, 10]` replaces the
    reward's draws of an acquisition step (tests replay the reference's); `seed` seeds the device draws otherwise."""
    if not _is_flow(model):
        raise TypeError("active_learning_flow needs a VAEFlow / REG_VAEFlow as model=")
    steps = [0]

    def passes(mdl, x, cur_mask, mask_p):
        if _forward is not None:
            return torch.stack([_forward(cur_mask).to(x.device) for _ in range(M)], 0)
        args = (x, cur_mask, mask_p) if mdl.regularised else (x, cur_mask)  # evaluate.py:396-399
        return torch.stack([mdl.forward(*args)[mdl.X_MEAN_Q] for _ in range(M)], 0)

    def reward(mdl, x, mask, im, t):
        steps[0] += 1
        eps = None if _reward_eps is None else _reward_eps(t).to(x.device)
        return flow_reward_matrix(mdl, x, mask, im, eps=eps, seed=None if seed is None else seed + steps[0])

    out = _acquisition_loop(test_data, test_mask, obs_dim, M, device, p_missingness, Repeat, model, lambda: model, passes,
                            reward, verbose, max_steps)
    return _save_active(out, save, experiment_type, data_type, vae_type, missing_rate, alpha, p_missingness, reg_type)


def active_sweep(data_loader_train, configs, test_data, test_mask, missing_rate, obs_dim, hid_dim, K, M, latent_dim, data_type,
                 training_parameters, experiment_type, max_epochs, valid_k, num_estimates, device=None, stage="evaluate",
                 reg_type="ml_reg", beta=1.0, beta_annealing=False, alpha_annealing=True, Repeat=5, models=None, save=True,
                 max_steps=None):
    """active_learning_func() for a LIST of runs - the loop body of src/experiment_main/active_learning.py (train, then
    active_learning_func, inside `for data_file: for missing: for alpha:`) after train_sweep, as one call; the twin of
    harness.eval_sweep, with its conventions for configs and models.
    Members are grouped with harness.eval_groups: plain Reg_VAE / vanilla_VAE members of one class and reg_type run the whole
    loop through ONE ensemble.EnsembleAcquirer - a fixed number of launches per acquisition step whatever their number, nothing
    read back before the end.  The members that leaves alone are split with harness.family_eval_groups: two or more Reg_VAE_mask /
    vanilla_VAE_mask members of one class, shape and reg_type run through ONE ensemble.MaskEnsembleAcquirer, two or more Reg_EDDI /
    vanilla_EDDI members of one class, shape, emb_dim and reg_type through ONE ensemble.EDDIEnsembleAcquirer, outputs and files
    exactly as for the plain groups.  A mask-augmented or point-net member with no second of its kind, and every other family
    (wide, mnist EDDI), goes alone through active_learning_func, and the flow models through active_learning_flow.
    Returns, per member in the order of configs, the dict active_learning_func returns (information_curve_CHAI [Repeat, n, d] - the scalar curve broadcast over the rows, as the reference stores it -, action_CHAI
    [Repeat, n, d-1] float, R_hist_CHAI [Repeat, d-1, n, d-1], im_CHAI [Repeat, d-1, M, n, d]) and (save=True) writes the
    reference's four files under active_result_paths(...) with that member's alpha / p_missingness.
    What differs from active_learning_func for the members run together: what eval_sweep states for its members (no p pass,
    eps from the member's Philox stream), and a given (or loaded) model serves every repeat - the reference reloads the same
    checkpoint per repeat.  The estimator and its distribution are the same."""
    cfgs = _sweep_configs(configs, models)
    dev = torch.device(device) if device is not None else torch.device("cuda")
    ms = _sweep_models(cfgs, models, dev, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters,
                       max_epochs, valid_k, num_estimates, experiment_type, reg_type, alpha_annealing=alpha_annealing)
    out = [None] * len(cfgs)
    runs = [(EnsembleAcquirer, idx) for idx in eval_groups(ms)[0].values()]
    family_groups, single = family_eval_groups(ms)  # (of the members eval_groups leaves alone)
    for key, idx in family_groups.items():
        if len(idx) >= 2:
            runs.append((MaskEnsembleAcquirer if key[0] == "mask" else EDDIEnsembleAcquirer, idx))
        else:
            single = sorted(single + idx)
    for g in single:
        c = cfgs[g]
        fn = active_learning_flow if _is_flow(ms[g]) else active_learning_func
        out[g] = fn(data_loader_train, test_data, test_mask, missing_rate, obs_dim, hid_dim, K, M, latent_dim, data_type,
                    training_parameters, experiment_type, c["vae_type"], max_epochs, valid_k, num_estimates, dev, c["alpha"],
                    stage, c["p_missingness"], reg_type, beta, beta_annealing, alpha_annealing, Repeat, model=ms[g], save=save,
                    max_steps=max_steps)
    x = test_data.reshape(-1, obs_dim).float().to(dev)
    for acquirer, idx in runs:
        with torch.no_grad():
            acq = acquirer([ms[g] for g in idx], seeds=[cfgs[g]["seed"] for g in idx])
            info, action, R_hist, im_hist = [t.cpu() for t in acq.run(x, M, repeats=Repeat, max_steps=max_steps)]
        n = x.shape[0]
        for k, g in enumerate(idx):
            res = dict(information_curve_CHAI=info[k, :, None, :].expand(Repeat, n, obs_dim).clone(),
                       action_CHAI=action[k].float(), R_hist_CHAI=R_hist[k].clone(), im_CHAI=im_hist[k].clone())
            out[g] = _save_active(res, save, experiment_type, data_type, cfgs[g]["vae_type"], missing_rate, cfgs[g]["alpha"],
                                  cfgs[g]["p_missingness"], reg_type)
    return out
