"""Harness around the model classes: the pieces of the reference's L2/L3 layers that sit on the hot path.

  create_missing_uci   src/utils/utils.py:36-39      per-step Bernoulli keep-mask (device Philox instead of numpy)
  model_loader         src/utils/loaders.py:13-246   vae_type substring dispatch + checkpoint naming
  checkpoint_path      src/experiment_main/train.py:120-131
  train                src/experiment_main/train.py:13-133   epoch / batch loop, Adam(lr=1e-3), save at end
  train_sweep          src/experiment_main/imputation.py:21-39  the drivers' loops over alpha / p_missingness / split around
                                                             train(), as ensembles stepped by one pair of launches (ensemble.py)
  eval_vae             src/experiment_main/evaluate.py:136-297  M MC passes: imputation RMSE on ~mask, ELBO, NLL; engine="batched"
                                                             (flow models): all passes and batches in one launch set
                                                             (flow.FlowEvaluator)
  eval_sweep           src/experiment_main/imputation.py:51-59  eval_vae() of a list of runs, the plain, mask-augmented and
                                                             point-net members in one pair of launches per group and loader
                                                             (ensemble.EnsembleEvaluator and its two family subclasses)
  eval_vae_mnar        src/experiment_main/evaluate.py:13-69   importance-weighted imputation RMSE (MNAR path)
  eval_miwae           src/experiment_main/evaluate.py:72-133   importance-weighted imputation RMSE (MIWAE path)

The families model_loader builds are Reg_VAE, vanilla_VAE and their *_mask variants, Reg_EDDI / vanilla_EDDI (and, for
data_type == 'mnist', Reg_EDDI_mnist / vanilla_EDDI_mnist), REG_notMIWAE_v2, notMIWAE_myversion and MIWAE / Reg_MIWAE.  The flow
models (VAEFlow / REG_VAEFlow, flow.py) are reached through their classes and the `model=` keyword of train() and eval_vae();
model_loader itself still raises NotImplementedError for flow vae_types.

The loops ask the model, not vae_type: trainer_class_for(model) picks the step trainer by class,
model.regularised says whether a mask_p is drawn (draw_mask_p), model.forward_loss is the reference's forward -> loss call
for that family and model.X_MEAN_Q the reconstruction mean in forward's tuple.  vae_type decides file names, the 'with_drop'
data treatment and whether the loader comes alone (MNAR) or as a pair.
"""
from __future__ import annotations

import contextlib
import io
import itertools
import os

import torch

from . import _lib as L
from . import ops
from .chainfamily import stream_seed
from .ensemble import (EDDI, MASK, EDDIEnsembleEvaluator, EDDIEnsembleTrainer, EnsembleEvaluator, EnsembleTrainer,
                       MaskEnsembleEvaluator, MaskEnsembleTrainer, stackable, steps_in_ensemble, sweep_family)
from .fused import FusedTrainer
from .models import Reg_VAE, Reg_VAE_mask, _VAEBase, vanilla_VAE, vanilla_VAE_mask
from .notmiwae import NMTrainer, REG_notMIWAE_v2, _NMBase, notMIWAE_myversion
from .notmiwae import impute_stream as nm_impute_stream
from .eddi import EDDITrainer, Reg_EDDI, _EDDIBase, vanilla_EDDI
from .eddi_mnist import EDDIMnistTrainer, Reg_EDDI_mnist, vanilla_EDDI_mnist, _EDDIMnistBase
from .miwae import MIWAE, MIWTrainer, Reg_MIWAE, _MIWBase, impute_stream, small_max_rows
from .miw_ensemble import MIWEnsembleTrainer
from .miw_ensemble import sweep_key as miw_sweep_key
from .flow import FlowEvaluator, FlowTrainer, _FlowBase
from .flow import small_max_rows as flow_small_max_rows
from .flow_ensemble import MIN_GROUP as FLOW_MIN_GROUP
from .flow_ensemble import FlowEnsembleTrainer
from .flow_ensemble import sweep_key as flow_sweep_key
from .wide import WideTrainer

_seed_counter = [0]


def create_missing_uci(shape, missing_rate, device="cuda", seed=None, offset=0):
    """Keep-mask (True = keep) with P(keep) = 1 - missing_rate/100, drawn on the device (utils.py:36-39).
    The reference draws from numpy's global RNG on the host; only the distribution is reproducible."""
    out = torch.empty(tuple(shape), dtype=torch.uint8, device=device)
    if seed is None:
        _seed_counter[0] += 1
        seed, offset = 0x5EED, _seed_counter[0] * (1 << 32)
    ops.draw_mask(None, out, 1.0 - missing_rate / 100.0, seed, offset)
    return out.view(torch.bool)


def create_missing_uci_drop_eddi(shape, device="cuda", generator=None):
    """Per-element keep-mask of the 'with_drop' variants (utils.py:42-45): keep ~ Bernoulli(1 - min(U, 0.99)) with its own U per
    element, drawn on the device as a float 0 / 1 tensor (the reference draws numpy / scipy variates on the host; only the
    distribution is reproducible - marginally P(keep) = 1 - E[min(U, .99)] = 0.50005)."""
    keep_p = 1.0 - torch.rand(tuple(shape), device=device, generator=generator).clamp_(max=0.99)
    return (torch.rand(tuple(shape), device=device, generator=generator) < keep_p).float()


def _family(vae_type: str) -> str:
    # train.py:122-124: first two '_' tokens of vae_type with the digits removed
    return "".join(ch for ch in "_".join(vae_type.split("_")[:2]) if not ch.isdigit())


def checkpoint_path(experiment_type, data_type, vae_type, missing_rate, alpha=1.0, p_missingness=30, reg_type="kl_reg"):
    """File name used by train() to save and by model_loader(stage != 'train') to load (train.py:120-131)."""
    base = os.path.join("experiments", experiment_type, data_type, "checkpoints", _family(vae_type))
    if "vanilla" in vae_type:
        return os.path.join(base, f"checkpoint_{vae_type}_{missing_rate}_missing_rate_test.pt")
    return os.path.join(base, f"checkpoint_{vae_type}_{alpha}_{p_missingness}_{reg_type}_{missing_rate}"
                              "_missing_rate_full_reg_test.pt")


def model_loader(stage, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters, max_epochs,
                 num_samples, num_estimates, experiment_type, reg_type, vae_type="vae", alpha=1.0, p_missingness=30,
                 beta=0.5, beta_annealing=True, alpha_annealing=True, not_miwae_type="changed"):
    """Same positional signature and substring dispatch as loaders.py:13-246 for the in-scope families."""
    if "flow" in vae_type:
        raise NotImplementedError(f"vae_type {vae_type!r}: only reg_vae* / vanilla_vae* / *_notMIWAE* / *MIWAE* / *_EDDI* "
                                  "are on the accelerated path")
    augm = "mask_augm" in vae_type  # loaders.py:47, 143
    if "reg_notMIWAE" in vae_type:  # loaders.py:89-103
        model = REG_notMIWAE_v2(obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates)
    elif "vanilla_notMIWAE" in vae_type:  # loaders.py:219-233
        model = notMIWAE_myversion(obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates)
    elif "reg_MIWAE" in vae_type:  # loaders.py:135-148
        model = Reg_MIWAE(obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates)
    elif "MIWAE" in vae_type and "notMIWAE" not in vae_type:  # loaders.py:234-244 (the final else: vanilla_MIWAE*)
        model = MIWAE(obs_dim, hid_dim, K, latent_dim, training_parameters, num_samples, num_estimates)
    elif "reg_EDDI" in vae_type and data_type == "mnist":  # loaders.py:104-109
        model = Reg_EDDI_mnist(obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, reg_type, num_samples,
                               num_estimates)
    elif "vanilla_EDDI" in vae_type and data_type == "mnist":  # loaders.py:185-190
        model = vanilla_EDDI_mnist(obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, num_samples,
                                   num_estimates)
    elif "reg_EDDI" in vae_type:  # loaders.py:104-131 (UCI branch)
        model = Reg_EDDI(obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, reg_type, num_samples,
                         num_estimates)
    elif "vanilla_EDDI" in vae_type:  # loaders.py:196-218
        model = vanilla_EDDI(obs_dim, hid_dim, K, latent_dim, training_parameters, experiment_type, num_samples,
                             num_estimates)
    elif "reg_vae" in vae_type:
        model = (Reg_VAE_mask if augm else Reg_VAE)(obs_dim, hid_dim, K, latent_dim, training_parameters,
                                                    experiment_type, reg_type, num_samples, num_estimates)
    elif "vanilla_vae" in vae_type:
        model = (vanilla_VAE_mask if augm else vanilla_VAE)(obs_dim, hid_dim, K, latent_dim, training_parameters,
                                                            experiment_type, num_samples, num_estimates)
    else:
        raise NotImplementedError(f"vae_type {vae_type!r}")
    if stage == "train":
        print("Initializing fresh model")
    else:
        print("Loading saved model")
        path = checkpoint_path(experiment_type, data_type, vae_type, missing_rate, alpha, p_missingness, reg_type)
        model.load_state_dict(torch.load(path, map_location=torch.device("cpu"), weights_only=True))
    return model


def trainer_class_for(model):
    """The step trainer of a model, decided on its class (and, for the dense classes, on `_wide`): image-width EDDI first
    (train.py:31-47), then the generic-GEMM step of an encoder input > 128 columns (wide.py), then the families."""
    if isinstance(model, _EDDIMnistBase):
        return EDDIMnistTrainer
    if getattr(model, "_wide", False):
        return WideTrainer
    for base, cls in ((_FlowBase, FlowTrainer), (_MIWBase, MIWTrainer), (_NMBase, NMTrainer), (_EDDIBase, EDDITrainer),
                      (_VAEBase, FusedTrainer)):
        if isinstance(model, base):
            return cls
    raise TypeError(f"no step trainer for {type(model).__name__}")


def draw_mask_p(model, shape, mask, p_missingness, device):
    """mask_p = create_missing_uci(shape, p) * mask (train.py:53-56; evaluate.py:172-173), as float for the MNAR classes."""
    mask_p = create_missing_uci(shape, p_missingness, device=device) * mask
    return mask_p.float() if isinstance(model, _NMBase) else mask_p


def _rmse_unobserved(x_mean, x, mask):
    """RMSE of x_mean against x over the entries with mask == 0 (bool or float 0 / 1 mask)."""
    inv = ~mask if mask.dtype == torch.bool else (mask == 0)
    return torch.sqrt(torch.sum(torch.square(x_mean * inv - x * inv)) / torch.sum(inv))


def _save(obj, path):
    os.makedirs(os.path.dirname(path), exist_ok=True)  # the reference never creates it
    torch.save(obj, path)


def _save_checkpoint(model, experiment_type, data_type, vae_type, missing_rate, alpha, p_missingness, reg_type):
    _save({k: v.detach().cpu() for k, v in model.state_dict().items()},
          checkpoint_path(experiment_type, data_type, vae_type, missing_rate, alpha, p_missingness, reg_type))


def _model_for_eval(model, device, *loader_args, **loader_kw):
    """`model` if given, else the checkpoint that model_loader('test', ...) reloads; on `device`."""
    if model is None:
        model = model_loader("test", *loader_args, **loader_kw)
    return model.to(device)


# ------------------------------------------------------------------------------------------------ the frame of the sweeps
def _sweep_configs(configs, models=None, loaders=None):
    """A sweep's configs with their defaults filled in; `models` and `loaders`, where given, hold one entry per config."""
    cfgs = [{"alpha": 1.0, "p_missingness": 30, "seed": 0, **c} for c in configs]
    for given, what in ((models, "models"), (loaders, "loaders")):
        if given is not None and len(given) != len(cfgs):
            raise L.VpcError(f"{len(given)} {what} for {len(cfgs)} configurations")
    return cfgs


def _sweep_models(cfgs, models, device, *loader_args, **loader_kw):
    """One model per member on `device`: models[g], else its checkpoint (model_loader('test', *loader_args, vae_type, ...))."""
    return [_model_for_eval(None if models is None else models[g], device, *loader_args, c["vae_type"], alpha=c["alpha"],
                            p_missingness=c["p_missingness"], **loader_kw) for g, c in enumerate(cfgs)]


def _stack_key(model):
    """(class, reg_type), what the members of one ensemble share (ensemble.validate_members); None: not stackable."""
    return (type(model), getattr(model, "reg_type", None)) if stackable(model) else None


def _group(keys):
    """THE split of a sweep, from one key per member: ({key: [member indices]}, [indices whose key is None: they go alone])."""
    groups, alone = {}, []
    for g, k in enumerate(keys):
        (alone if k is None else groups.setdefault(k, [])).append(g)
    return groups, alone


def eval_groups(models):
    """How eval_sweep splits its members: ({(class, reg_type): [member indices]}, [indices evaluated one by one]).  Stackable
    members (ensemble.stackable) of one class and reg_type share an EnsembleEvaluator; every other family goes alone."""
    return _group([_stack_key(m) for m in models])


def family_eval_groups(models, cfgs=None):
    """How eval_sweep splits the members eval_groups leaves alone: ({key: [member indices]}, [indices of no family]).
    Mask-augmented members group by ("mask", class, obs_dim, latent_dim, reg_type), point-net members by ("eddi", class, obs_dim,
    emb_dim, latent_dim, reg_type) - what the members of one MaskEnsembleEvaluator / EDDIEnsembleEvaluator share; membership
    follows Family.require, as in training.  cfgs (the members' configs) is not consulted: a 'with_drop' run's evaluation does
    not differ from any other, so unlike sweep_family nothing excludes it.  eval_sweep evaluates a group of two or more
    together and a group of one through eval_vae."""
    def key(m):
        for name, family in (("mask", MASK), ("eddi", EDDI)):
            try:
                family.require(m)
            except (TypeError, L.VpcError):
                continue
            return (name, type(m)) + tuple(family.shared(m))
        return None

    single = eval_groups(models)[1]
    groups, rest = _group([key(models[g]) for g in single])
    return {k: [single[i] for i in idx] for k, idx in groups.items()}, [single[i] for i in rest]


class _LoadersDiffer(L.VpcError):
    """_lock_step: the loaders ran out at different steps, or the batches of one step differ."""


def _lock_step(loaders, batch_key):
    """Iterate several loaders together: one tuple of batches (one per loader) per step.  All must end at the same step, and
    the batches of a step must agree in batch_key(batch): else _LoadersDiffer."""
    for batches in itertools.zip_longest(*loaders):
        if any(b is None for b in batches):
            raise _LoadersDiffer("per-member loaders must have the same number of batches")
        if len({batch_key(b) for b in batches}) != 1:
            raise _LoadersDiffer("per-member loaders must yield equal batch shapes at every step")
        yield batches


def train(data_loader_train, missing_rate, obs_dim, hid_dim, K, M, latent_dim, data_type, training_parameters,
          experiment_type, vae_type, train_k, num_estimates, max_epochs=1000, device=torch.device("cuda"), alpha=1.0,
          stage="train", p_missingness=30, reg_type="ml_reg", beta=1.0, beta_annealing=False, alpha_annealing=True,
          not_miwae_type="changed", fused=True, seed=0, save=True, verbose=True, model=None):
    """train.py:13-133 for reg_vae* / vanilla_vae* / *_notMIWAE* / *_EDDI* / *MIWAE*, and for a VAEFlow / REG_VAEFlow
    passed as `model` (train.py:77-86; model_loader does not build flows).  With fused=True every batch is one trainer
    step (no per-step host sync: the epoch total is read once per epoch, as the reference only prints it per epoch);
    with fused=False it is the reference's own sequence model.forward -> model.loss -> backward -> optim.Adam
    on the API path (model.forward_loss).  `model` (optional): train this model instead of a fresh one from model_loader;
    its class, not vae_type, picks the trainer and the forward -> loss wiring.  Returns the trained model."""
    if model is None:
        model = model_loader("train", obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters,
                             max_epochs, train_k, num_estimates, experiment_type, reg_type, vae_type, alpha=alpha,
                             p_missingness=p_missingness)
    model.to(device)
    loader = data_loader_train if "notMIWAE" in vae_type else data_loader_train[0]  # train.py:22-25
    # 'with_drop' variants (train.py:32-37, 50-51; vanilla classes only - the reference's regularised branch never draws mask_p
    # beside it): the model sees mask * mask_drop, the keep-mask of create_missing_uci_drop_eddi (utils.py:42-45)
    drop = "with_drop" in vae_type and not model.regularised
    if fused:
        trainer = trainer_class_for(model)(model, lr=0.001, seed=seed)
        train_step = trainer.train_step  # (bound once: the loop is host-paced at the reference's batch)
    else:
        model.flatten_parameters()
        optimizer = torch.optim.Adam(model.parameters(), lr=0.001)  # train.py:21
    for i in range(max_epochs):
        total_loss, epoch = 0.0, i + 1
        for data_sample, mask in loader:
            data_sample, mask = data_sample.to(device), mask.to(device)
            if drop:  # the step on the thinned mask (one more elementwise launch, no host sync)
                mask = mask.to(torch.float32) * create_missing_uci_drop_eddi(data_sample.shape, device=device)
            if fused:
                train_step(data_sample, mask, epoch=epoch, alpha=alpha, beta=beta, beta_annealing=beta_annealing,
                           p_missingness=p_missingness, stage=stage)
                continue
            mask_p = draw_mask_p(model, data_sample.shape, mask, p_missingness, device) if model.regularised else None
            _, (_, train_loss) = model.forward_loss(data_sample, mask, mask_p, epoch=epoch, alpha=alpha, beta=beta,
                                                    beta_annealing=beta_annealing, alpha_annealing=alpha_annealing,
                                                    stage=stage)
            optimizer.zero_grad()
            train_loss.backward()
            optimizer.step()
            total_loss += train_loss.item()
        if fused:
            total_loss = trainer.epoch_total()
        if verbose:
            print("Epoch: [{}/{}], Total Loss: {}".format(i, max_epochs, total_loss))
    if save:
        _save_checkpoint(model, experiment_type, data_type, vae_type, missing_rate, alpha, p_missingness, reg_type)
    print("Training is over!")
    return model


def _family_groups(cfgs, models, data_loader_train, loaders, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type,
                   training_parameters, max_epochs, train_k, num_estimates, experiment_type, reg_type):
    """{member index: key} of the mask-augmented, point-net, MIWAE-path and flow members of a sweep that step in an ensemble:
    those whose key - (family, model class, reg_type, ml_reg term on, emb_dim), or miw_ensemble.sweep_key's ("miw", class, obs_dim,
    latent_dim, num_samples) for a MIWAE / Reg_MIWAE whose first batch takes the small-batch step (VPC_MIW_SMALL), or
    flow_ensemble.sweep_key's ("flow", class, obs_dim, hid_dim) for a VAEFlow / REG_VAEFlow whose first batch takes the few-row
    step (VPC_FLOW_SMALL) - at least one other member shares (flow: FLOW_MIN_GROUP members in all).  Decided BEFORE any member
    is built or trained, so that train_sweep still trains every other member at once, in the order of configs.  A member's
    class is that of models[g], else of a throw-away model_loader() build; the probe and the look at the first batch leave
    torch's generator where it was (the members' initial weights and a shuffling loader's order are what they are without it)."""
    keys = {}
    with torch.random.fork_rng(devices=[]):
        for g, c in enumerate(cfgs):
            vt = c["vae_type"]
            # (a MIWAE-path name is probed only while the small-batch step is on: with VPC_MIW_SMALL unset nothing is built or read)
            miw_name = "MIWAE" in vt and "notMIWAE" not in vt and "with_drop" not in vt and small_max_rows() > 0
            if models is None and not ("mask_augm" in vt or "EDDI" in vt or miw_name):  # (no other vae_type builds these classes)
                continue
            if models is not None:
                m = models[g]
            else:
                with contextlib.redirect_stdout(io.StringIO()):
                    m = model_loader("train", obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters,
                                     max_epochs, train_k, num_estimates, experiment_type, reg_type, vt, alpha=c["alpha"],
                                     p_missingness=c["p_missingness"])
            loader = data_loader_train if loaders is None else loaders[g]
            name = sweep_family(m, vt, loader[0], obs_dim)
            if name is not None:
                keys[g] = (name, type(m), getattr(m, "reg_type", None),
                           getattr(m, "reg_type", None) == "ml_reg" and c["alpha"] != 0.0, getattr(m, "emb_dim", None))
            elif isinstance(m, _MIWBase):
                key = miw_sweep_key(m, vt, loader[0], obs_dim)
                if key is not None:
                    keys[g] = key
            # (a flow member - model_loader builds none: they come in `models` - is probed only while the few-row step is on)
            elif isinstance(m, _FlowBase) and flow_small_max_rows() > 0:
                key = flow_sweep_key(m, vt, loader[0], obs_dim)
                if key is not None:
                    keys[g] = key
    count = {}
    for k in keys.values():
        count[k] = count.get(k, 0) + 1
    return {g: k for g, k in keys.items() if count[k] >= (FLOW_MIN_GROUP if k[0] == "flow" else 2)}


def train_sweep(data_loader_train, configs, missing_rate, obs_dim, hid_dim, K, M, latent_dim, data_type, training_parameters,
                experiment_type, train_k, num_estimates, max_epochs=1000, device=torch.device("cuda"), stage="train",
                reg_type="ml_reg", beta=1.0, beta_annealing=False, alpha_annealing=True, save=True, verbose=True,
                models=None, loaders=None):
    """train() for a LIST of runs that differ in vae_type (the data split), alpha, p_missingness and seed - the drivers' loops
    `for missing in [...]: for alpha in [...]:` around train() (src/experiment_main/imputation.py:21-39) as one call.
    configs: one dict per member with the keys vae_type, alpha (1.0), p_missingness (30), seed (0).  data_loader_train: what
    train() takes, shared by every member; or loaders = one such object per member (different splits), which must yield
    equal batch shapes at every step.  models (optional): one pre-built model per member, as train(model=).
    Plain Reg_VAE / vanilla_VAE members of one class and reg_type step together, one ensemble.EnsembleTrainer.step per batch
    (a mixed list is split into such groups).  Mask-augmented members (Reg_VAE_mask / vanilla_VAE_mask) and point-net members
    (Reg_EDDI / vanilla_EDDI with obs_dim % 4 == 0) are grouped by class, reg_type, whether the ml_reg term is on and, for the
    point-net classes, emb_dim: a group of two or more steps through ensemble.MaskEnsembleTrainer / EDDIEnsembleTrainer, a
    group of one goes through train().  MIWAE / Reg_MIWAE members are grouped by (class, obs_dim, latent_dim, num_samples) while
    VPC_MIW_SMALL routes their first batch to the small-batch step (miwae.small_step_route): a group of two or more steps
    through miw_ensemble.MIWEnsembleTrainer; with the variable unset each goes through train().  VAEFlow / REG_VAEFlow members
    (given in `models`) are grouped by (class, obs_dim, hid_dim) while VPC_FLOW_SMALL routes their first batch to the few-row
    step (flow.small_step_route): a group of flow_ensemble.MIN_GROUP or more steps through flow_ensemble.FlowEnsembleTrainer,
    bit for bit as train() steps each member; with the variable unset each goes through train().  'with_drop' runs of every
    family stay alone (train()'s loop thins their mask with a drop mask of its own at every step), and so do every other
    family, point-net members of another width and batches beyond the small-batch step: train(), one by one.
    Every member is trained as train(..., alpha=, p_missingness=, seed=) alone trains it - bit for bit, except in a MIWAE group
    whose members together have more row blocks than the chip has compute units (miw_ensemble.default_blocks then gives a
    workgroup more rows and a member fewer partial blocks than the stand-alone step takes: the same draws and the same
    math in another summation order of the weight gradients, within 2e-5 of the flat gradient per step) - prints the
    reference's epoch line and is saved under its own checkpoint_path.  Returns the models in the order of configs."""
    cfgs = _sweep_configs(configs, models, loaders)
    fam = _family_groups(cfgs, models, data_loader_train, loaders, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type,
                         training_parameters, max_epochs, train_k, num_estimates, experiment_type, reg_type)
    out, keys = [], []
    for g, c in enumerate(cfgs):
        loader = data_loader_train if loaders is None else loaders[g]
        m = models[g] if models is not None else model_loader(
            "train", obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters, max_epochs, train_k,
            num_estimates, experiment_type, reg_type, c["vae_type"], alpha=c["alpha"], p_missingness=c["p_missingness"])
        out.append(m.to(device))
        # eval_groups' key and whether the third eps plane is drawn (the members of one step agree on it), or None: alone
        keys.append(fam[g] if g in fam else
                    _stack_key(m) + (getattr(m, "reg_type", None) == "ml_reg" and c["alpha"] != 0.0,)
                    if steps_in_ensemble(m, c["vae_type"], loader[0], obs_dim) else None)
        if keys[g] is None:  # at once: before the next member is built
            train(loader, missing_rate, obs_dim, hid_dim, K, M, latent_dim, data_type, training_parameters, experiment_type,
                  c["vae_type"], train_k, num_estimates, max_epochs, device, c["alpha"], stage, c["p_missingness"], reg_type,
                  beta, beta_annealing, alpha_annealing, seed=c["seed"], save=save, verbose=verbose, model=m)
    rows = lambda t: t.to(device).reshape(-1, obs_dim)
    for key, idx in _group(keys)[0].items():
        trainer_cls = {"mask": MaskEnsembleTrainer, "eddi": EDDIEnsembleTrainer, "miw": MIWEnsembleTrainer,
                       "flow": FlowEnsembleTrainer}.get(key[0], EnsembleTrainer)
        ens = trainer_cls([out[g] for g in idx], lr=0.001, seeds=[cfgs[g]["seed"] for g in idx])
        # (MIWTrainer.train_step takes alpha and p_missingness from the schedule, and so does the MIWAE ensemble step)
        # (FlowTrainer.train_step takes alpha, p_missingness and stage: beta stays the step's default)
        schedule = (lambda i: {}) if key[0] == "miw" else (lambda i: dict(stage=stage)) if key[0] == "flow" else \
            (lambda i: dict(epoch=i + 1, beta=beta, beta_annealing=beta_annealing))
        alphas, pms = [cfgs[g]["alpha"] for g in idx], [cfgs[g]["p_missingness"] for g in idx]
        sources = [data_loader_train[0]] if loaders is None else [loaders[g][0] for g in idx]
        for i in range(max_epochs):
            for batches in _lock_step(sources, lambda b: (b[0].shape, b[1].shape)):  # (raises when the loaders differ)
                if loaders is None:  # one batch shared by the members
                    x, mk = rows(batches[0][0]), rows(batches[0][1])
                else:
                    x, mk = torch.stack([rows(b[0]) for b in batches]), torch.stack([rows(b[1]) for b in batches])
                ens.step(x, mk, alpha=alphas, p_missingness=pms, **schedule(i))
            totals = ens.epoch_total()
            if verbose:
                for g, total_loss in zip(idx, totals):
                    print("Epoch: [{}/{}], Total Loss: {}".format(i, max_epochs, total_loss))
        for g in idx:
            if save:
                _save_checkpoint(out[g], experiment_type, data_type, cfgs[g]["vae_type"], missing_rate, cfgs[g]["alpha"],
                                 cfgs[g]["p_missingness"], reg_type)
            print("Training is over!")
    return out


def result_paths(experiment_type, data_type, vae_type, loader_stage, missing_rate, alpha=0.5, p_missingness=30,
                 reg_type="ml_reg"):
    """File names eval_vae writes (evaluate.py:247-297): rmse, vae_elbo, negative_llh(_q), negative_llh(_q)_imputed."""
    fam = _family(vae_type)
    rest = os.path.join("experiments", experiment_type, data_type, "rest", fam)
    elbo = os.path.join("experiments", experiment_type, data_type, "elbos", fam)
    pre = f"{loader_stage}_{vae_type}"
    if "vanilla" in vae_type:
        suf = f"_{missing_rate}_missing_rate_test.pt"
        return dict(rmse=os.path.join(rest, pre + "_rmse" + suf), elbo=os.path.join(elbo, pre + "_vae_elbo" + suf),
                    negll=os.path.join(rest, pre + "_negative_llh" + suf),
                    negll_imp=os.path.join(rest, pre + "_negative_llh_imputed" + suf))
    suf = f"_{alpha}_{p_missingness}_{reg_type}_{missing_rate}_missing_rate_full_reg_test.pt"
    return dict(rmse=os.path.join(rest, pre + "_rmse" + suf), elbo=os.path.join(elbo, pre + "_vae_elbo" + suf),
                negll=os.path.join(rest, pre + "_negative_llh_q" + suf),
                negll_imp=os.path.join(rest, pre + "_negative_llh_q_imputed" + suf))


def _save_results(res, paths):  # the files of one result dict: res[k] under paths[k]
    for k, pth in paths.items():
        _save(res[k], pth)


def eval_vae(list_loaders, missing_rate, obs_dim, hid_dim, K, M, latent_dim, data_type, training_parameters,
             experiment_type, vae_type, max_epochs, valid_k, num_estimates, device=torch.device("cuda"), alpha=0.5,
             stage="evaluate", p_missingness=30, reg_type="ml_reg", beta=1.0, beta_annealing=False,
             alpha_annealing=True, model=None, save=True, engine="chain", seed=None):
    """evaluate.py:136-297 for reg_vae* / vanilla_vae* and, given as `model`, VAEFlow / REG_VAEFlow (the flow branch,
    evaluate.py:189-200): reload the checkpoint (or use `model`), and for every
    (loader, loader_stage): M Monte-Carlo passes of forward + loss(llh_eval=True, stage) per batch; RMSE of the
    imputations on the UNobserved entries, mean ELBO, NLL on observed and on imputed entries.  Returns
    {loader_stage: dict(rmse, elbo, negll, negll_imp)} and (save=True) writes the reference's four files.

    engine="chain" (the default) walks the passes and batches as the reference does.  engine="batched" (flow models only,
    given as `model`): per (loader, loader_stage) the loader is iterated once per pass, the batches are gathered on the
    device and ONE flow.FlowEvaluator.evaluate call computes every pass x batch (12 library calls whatever M is), one .cpu().
    No p pass and no mask_p draw (FlowEvaluator says why), eps from the Philox stream of `seed`, beta = 1 as the reference's
    drivers leave it for the flows; same estimator, same files.  No fallback: a model of another family raises VpcError, and
    so does REG_VAEFlow with stage="train", whose loss reads the p pass."""
    if engine not in ("chain", "batched"):
        raise L.VpcError(f"engine={engine!r}: 'chain' or 'batched'")
    out = {}
    with torch.no_grad():
        model = _model_for_eval(model, device, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters,
                                max_epochs, valid_k, num_estimates, experiment_type, reg_type, vae_type, alpha=alpha,
                                p_missingness=p_missingness)
        if engine == "batched":
            if not isinstance(model, _FlowBase):
                raise L.VpcError(f"engine='batched' evaluates VAEFlow and REG_VAEFlow, not {type(model).__name__} "
                                 "(eval_sweep evaluates the other families' sweeps together)")
            if model.regularised and stage == "train":
                raise L.VpcError("engine='batched' with stage='train': REG_VAEFlow's train-stage loss reads the p pass "
                                 "(VAE.py:2081-2097), which the batched engine does not run")
            ev = FlowEvaluator(model, seed=seed)
            for loader, loader_stage in list_loaders:
                gathered = _gather_passes([loader], M, obs_dim, device)
                if gathered is None:
                    raise L.VpcError(f"loader stage {loader_stage!r}: a Monte-Carlo pass without a batch")
                r = ev.evaluate(*gathered).cpu()
                out[loader_stage] = dict(rmse=r[0].clone(), elbo=r[1].clone(), negll=r[2].clone(), negll_imp=r[3].clone())
                if save:
                    _save_results(out[loader_stage], result_paths(experiment_type, data_type, vae_type, loader_stage,
                                                                  missing_rate, alpha, p_missingness, reg_type))
            return out
        for loader, loader_stage in list_loaders:
            recon, res, res_negll, res_negll_imp = [], [], [], []
            for _ in range(M):
                elbos, negls, negls_imp, temp_recon = [], [], [], []
                for data_sample, mask in loader:
                    data_sample, mask = data_sample.to(device), mask.to(device)
                    mask_p = draw_mask_p(model, data_sample.shape, mask, p_missingness, device) if model.regularised else None
                    o, (_, train_loss, negl, negl_imp) = model.forward_loss(
                        data_sample, mask, mask_p, epoch=max_epochs, alpha=alpha, beta=beta, beta_annealing=beta_annealing,
                        alpha_annealing=alpha_annealing, stage=stage, llh_eval=True)
                    temp_recon.append(_rmse_unobserved(torch.squeeze(o[model.X_MEAN_Q]), data_sample.view(-1, obs_dim),
                                                       mask.reshape(-1, obs_dim)))
                    elbos.append(train_loss)
                    negls.append(torch.as_tensor(negl, device=device, dtype=torch.float32))
                    negls_imp.append(torch.as_tensor(negl_imp, device=device, dtype=torch.float32))
                recon.append(torch.stack(temp_recon).mean())
                res.append(torch.mean(torch.stack(elbos)))
                res_negll.append(torch.mean(torch.stack(negls)))
                res_negll_imp.append(torch.mean(torch.stack(negls_imp)))
            r = dict(rmse=torch.stack(recon).mean(), elbo=torch.stack(res).mean(), negll=torch.stack(res_negll).mean(),
                     negll_imp=torch.stack(res_negll_imp).mean())
            out[loader_stage] = {k: v.cpu() for k, v in r.items()}
            if save:
                _save_results(out[loader_stage], result_paths(experiment_type, data_type, vae_type, loader_stage, missing_rate,
                                                              alpha, p_missingness, reg_type))
    return out


def _gather_passes(sources, M, obs_dim, device):
    """Iterate every loader of `sources` (one shared loader, or one per member) once per MC pass, as eval_vae does, and put
    the batches of all passes behind each other on the device.  -> (x, mask, batches): x / mask [R, d] for one source, else
    [G, R, d]; batches = M lists of (row_lo, row_hi) into them.  None when the members' loaders do not yield the same batch
    sizes at every step (one evaluate call needs one layout)."""
    xs, ms, ranges, r = [[] for _ in sources], [[] for _ in sources], [], 0
    try:
        for _ in range(M):
            pr = []
            for bs in _lock_step(sources, lambda b: b[0].reshape(-1, obs_dim).shape[0]):
                for k, b in enumerate(bs):
                    xs[k].append(b[0].to(device).reshape(-1, obs_dim))
                    ms[k].append(b[1].to(device).reshape(-1, obs_dim))
                n = xs[0][-1].shape[0]
                pr.append((r, r + n))
                r += n
            if not pr:
                return None
            ranges.append(pr)
    except _LoadersDiffer:
        return None
    x, mk = [torch.cat(v) for v in xs], [torch.cat(v) for v in ms]
    return (x[0], mk[0], ranges) if len(sources) == 1 else (torch.stack(x), torch.stack(mk), ranges)


def eval_sweep(list_loaders, configs, missing_rate, obs_dim, hid_dim, K, M, latent_dim, data_type, training_parameters,
               experiment_type, max_epochs, valid_k, num_estimates, device=torch.device("cuda"), stage="evaluate",
               reg_type="ml_reg", beta=1.0, beta_annealing=False, alpha_annealing=True, models=None, loaders=None, save=True,
               engine="chain"):
    """eval_vae() for a LIST of runs - the evaluation that follows every train() of the drivers' loops
    (src/experiment_main/imputation.py:51-59 around evaluate.py:136-297) as one call; the twin of train_sweep, with its
    conventions for configs.  list_loaders: what eval_vae takes, shared by every member; or loaders = one such list per
    member.  models (optional): one model per member, else each member's checkpoint through model_loader('test', ...).
    Plain Reg_VAE / vanilla_VAE members of one class and reg_type are evaluated together: per (loader, loader_stage) the
    loader is iterated once per MC pass (a shuffling loader gives every pass its own partition into batches), the batches
    are gathered on the device and ONE ensemble.EnsembleEvaluator.evaluate call computes every member x pass x batch.  Two or
    more Reg_VAE_mask / vanilla_VAE_mask members of one class, shape and reg_type, and two or more Reg_EDDI / vanilla_EDDI members
    of one class, shape, emb_dim and reg_type (family_eval_groups), are evaluated the same way through MaskEnsembleEvaluator /
    EDDIEnsembleEvaluator.  Who goes through eval_vae one by one: a mask-augmented or point-net member with no second of its kind
    or past its family's kernels (2 obs_dim > 128; obs_dim > 64 or emb_dim > 32), every other family (wide, mnist EDDI, MNAR,
    MIWAE; flow under the default engine), and the members of a group whose per-member loaders differ in their batch sizes.  Returns, per member in the order of configs, what eval_vae returns, and (save=True) writes
    the reference's four files under result_paths(...) with that member's alpha / p_missingness.
    What differs from eval_vae for the members evaluated together: no p pass and no mask_p draw (VAE.py:410-420 never reads
    them, and under Philox there is no stream position to preserve); eps comes from the member's Philox stream (seed =
    the config's seed), not from torch.randn; a shared loader is iterated once per pass for the whole group, not once per
    member.  The estimator and its distribution are the same.
    engine="batched": every VAEFlow / REG_VAEFlow member goes through eval_vae(engine="batched", seed = the config's seed) - still
    one member after the other (DESIGN.md section 2.35 says why there is no member axis), each in 12 library calls per loader
    stage; every other member is routed as under the default "chain"."""
    if engine not in ("chain", "batched"):
        raise L.VpcError(f"engine={engine!r}: 'chain' or 'batched'")
    cfgs = _sweep_configs(configs, models, loaders)
    member_loaders = (lambda g: loaders[g]) if loaders is not None else (lambda g: list_loaders)
    ms = _sweep_models(cfgs, models, device, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters,
                       max_epochs, valid_k, num_estimates, experiment_type, reg_type)
    out = [None] * len(cfgs)

    def alone(g):
        c = cfgs[g]
        out[g] = eval_vae(member_loaders(g), missing_rate, obs_dim, hid_dim, K, M, latent_dim, data_type, training_parameters,
                          experiment_type, c["vae_type"], max_epochs, valid_k, num_estimates, device, c["alpha"], stage,
                          c["p_missingness"], reg_type, beta, beta_annealing, alpha_annealing, model=ms[g], save=save,
                          **(dict(engine="batched", seed=c["seed"]) if engine == "batched" and isinstance(ms[g], _FlowBase)
                             else {}))

    def together(idx, evaluator_class):
        """THE evaluation of a group: the passes gathered per loader stage, one evaluate call per stage, the results written."""
        stages = [s for _, s in member_loaders(idx[0])]
        gathered = [_gather_passes([list_loaders[li][0]] if loaders is None else [loaders[g][li][0] for g in idx], M, obs_dim,
                                   device) for li in range(len(stages))]
        if any(t is None for t in gathered) or any([s for _, s in member_loaders(g)] != stages for g in idx):
            for g in idx:
                alone(g)
            return
        with torch.no_grad():
            ev = evaluator_class([ms[g] for g in idx], seeds=[cfgs[g]["seed"] for g in idx])
            for g in idx:
                out[g] = {}
            for loader_stage, (x, mk, ranges) in zip(stages, gathered):
                r = ev.evaluate(x, mk, M=M, batches=ranges, epoch=max_epochs, beta=beta, beta_annealing=beta_annealing).cpu()
                for k, g in enumerate(idx):
                    res = out[g][loader_stage] = dict(rmse=r[k, 0].clone(), elbo=r[k, 1].clone(), negll=r[k, 2].clone(),
                                                      negll_imp=r[k, 3].clone())
                    if save:
                        _save_results(res, result_paths(experiment_type, data_type, cfgs[g]["vae_type"], loader_stage,
                                                        missing_rate, cfgs[g]["alpha"], cfgs[g]["p_missingness"], reg_type))

    groups, single = eval_groups(ms)
    family = {k: idx for k, idx in family_eval_groups(ms, cfgs)[0].items() if len(idx) >= 2}
    grouped = {g for idx in family.values() for g in idx}
    for g in single:
        if g not in grouped:
            alone(g)
    for idx in groups.values():
        together(idx, EnsembleEvaluator)
    for key, idx in family.items():
        together(idx, MaskEnsembleEvaluator if key[0] == "mask" else EDDIEnsembleEvaluator)
    return out


def mnar_result_path(experiment_type, data_type, vae_type, alpha=0.5, p_missingness=30, reg_type="ml_reg",
                     not_miwae_type="changed"):
    """File eval_vae_mnar writes (evaluate.py:56-69)."""
    rest = os.path.join("experiments", experiment_type, data_type, "rest", "".join(c for c in vae_type if not c.isdigit()))
    if "vanilla" in vae_type:
        return os.path.join(rest, f"{vae_type}_rmse_{not_miwae_type}_large_batch_test.pt")
    return os.path.join(rest, f"{vae_type}_rmse_{alpha}_{p_missingness}_{reg_type}_full_reg_large_batch_v2_test.pt")


def eval_vae_mnar(data_test, mask_test, missing_rate, obs_dim, hid_dim, K, M, latent_dim, data_type,
                  training_parameters, experiment_type, vae_type, max_epochs, valid_k, num_estimates,
                  device=torch.device("cuda"), alpha=0.5, stage="evaluate", p_missingness=30, reg_type="ml_reg",
                  beta=1.0, beta_annealing=False, alpha_annealing=True, not_miwae_type="changed", model=None,
                  save=True, max_decoder_rows=1 << 20, engine="chain", seed=None):
    """evaluate.py:13-69: M repetitions of the self-normalised importance-weighted imputation with valid_k samples
    per row, RMSE on the missing entries.  The reference walks the test set ONE ROW per forward (and redraws a
    full-size mask for each row); here rows are processed in chunks of max_decoder_rows / valid_k per launch
    sequence, one mask_p draw per repetition - the same estimator, row-independent, so the result has the same
    distribution.  Returns the RMSE (0-dim CPU tensor) and, with save=True, writes the reference's result file.

    engine="stream": every repetition is ONE notmiwae.impute_stream call over all rows (two launches, no decoder row in
    memory): no max_decoder_rows loop, and no mask_p draw - the imputation does not read it (impute_stream's docstring).
    The draws are Philox streams of `seed` (None: one from torch's generator); the offset starts at 0 and advances by the
    number of rows after every repetition (trainer.impute_draw_counter), so no two calls of a run share a counter.  A model
    outside the kernel's limits (obs_dim <= 128, latent_dim <= 16) raises VpcError: there is no fallback to the chain."""
    if engine not in ("chain", "stream"):
        raise L.VpcError(f"eval_vae_mnar: engine {engine!r} (engines: 'chain', 'stream')")
    with torch.no_grad():
        model = _model_for_eval(model, device, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters,
                                max_epochs, valid_k, num_estimates, experiment_type, reg_type, vae_type, alpha=alpha,
                                p_missingness=p_missingness, not_miwae_type=not_miwae_type)
        data_test = data_test.to(device).float().reshape(-1, obs_dim)
        mask_test = mask_test.to(device).float().reshape(-1, obs_dim)
        N = data_test.shape[0]
        rows = max(1, max_decoder_rows // max(1, model.num_samples))
        temp_recon = []
        if engine == "stream":
            seed = stream_seed(seed)
        offset = 0
        for rep in range(M):
            if engine == "stream":
                XM = nm_impute_stream(model, data_test, mask_test, seed=seed, offset=offset)  # model.num_samples, as the chain
                offset += N  # the call used the counter rows offset .. offset + N - 1
                temp_recon.append(_rmse_unobserved(XM, data_test, mask_test))
                continue
            XM = torch.zeros_like(data_test)
            mask_p = draw_mask_p(model, data_test.shape, mask_test, p_missingness, device)  # (for both classes: evaluate.py:30-31)
            for lo in range(0, N, rows):
                _, (xm, _, _) = model.forward_loss(
                    data_test[lo:lo + rows], mask_test[lo:lo + rows], mask_p[lo:lo + rows] if model.regularised else None,
                    epoch=max_epochs, alpha=alpha, beta=beta, beta_annealing=beta_annealing, alpha_annealing=alpha_annealing,
                    stage=stage, llh_eval=True)
                XM[lo:lo + rows] = xm
            temp_recon.append(_rmse_unobserved(XM, data_test, mask_test))
        recon = torch.stack(temp_recon).mean().cpu()
        if save:
            _save(recon, mnar_result_path(experiment_type, data_type, vae_type, alpha, p_missingness, reg_type, not_miwae_type))
    return recon


def miwae_result_path(experiment_type, data_type, vae_type, loader_stage, alpha=0.5, p_missingness=30, reg_type="ml_reg"):
    """File eval_miwae writes (evaluate.py:120-133): the literal '50_missing_rate' whatever the missing rate."""
    rest = os.path.join("experiments", experiment_type, data_type, "rest", _family(vae_type))
    if "vanilla" in vae_type:
        return os.path.join(rest, f"{loader_stage}_{vae_type}_rmse_50_missing_rate_test.pt")
    return os.path.join(rest, f"{loader_stage}_{vae_type}_rmse_{alpha}_{p_missingness}_{reg_type}"
                              "_full_reg_50_missing_rate_test.pt")


def eval_miwae(list_loaders, missing_rate, obs_dim, hid_dim, K, M, latent_dim, data_type, training_parameters,
               experiment_type, vae_type, max_epochs, valid_k, num_estimates, device=torch.device("cuda"), alpha=0.5,
               stage="evaluate", p_missingness=30, reg_type="ml_reg", beta=1.0, beta_annealing=False,
               alpha_annealing=True, model=None, save=True, max_decoder_rows=1 << 23, engine="chain", seed=None):
    """evaluate.py:72-133: for every (loader, loader_stage), M repetitions; per batch a mask_p draw (Reg_MIWAE) and the
    llh_eval imputation of every row with valid_k samples; the RMSE on ~mask per BATCH, averaged over the batches, then
    over the repetitions.  The reference imputes one row per forward; here max_decoder_rows // valid_k rows go through
    one launch sequence with the per-row pairing, which equals the single-row calls.  Returns {loader_stage: rmse} (0-dim
    CPU tensors) and, with save=True, writes the reference's result files (miwae_result_path).

    engine="stream": every batch is ONE miwae.impute_stream call (two launches, no decoder row in memory): no
    max_decoder_rows loop, and no mask_p draw - the imputation does not read it (impute_stream's docstring).  The draws are
    Philox streams of `seed` (None: one from torch's generator); the offset starts at 0 and advances by the batch's rows
    after every call (trainer.impute_draw_counter), so no two calls of a run share a counter.  A model outside the
    kernel's limits (obs_dim <= 32, latent_dim <= 16) raises VpcError: there is no fallback to the chain."""
    if engine not in ("chain", "stream"):
        raise L.VpcError(f"eval_miwae: engine {engine!r} (engines: 'chain', 'stream')")
    out = {}
    with torch.no_grad():
        model = _model_for_eval(model, device, obs_dim, hid_dim, K, latent_dim, missing_rate, data_type, training_parameters,
                                max_epochs, valid_k, num_estimates, experiment_type, reg_type, vae_type, alpha=alpha,
                                p_missingness=p_missingness)
        rows = max(1, max_decoder_rows // max(1, valid_k))
        if engine == "stream":
            seed = stream_seed(seed)
        offset = 0
        for loader, loader_stage in list_loaders:
            recon = []
            for _ in range(M):
                XM = []
                for data_sample, mask in loader:
                    x = data_sample.to(device).float().reshape(-1, obs_dim)
                    mask = mask.to(device).reshape(-1, obs_dim)
                    if engine == "stream":
                        xm = impute_stream(model, x, mask, num_samples=valid_k, seed=seed, offset=offset)
                        offset += x.shape[0]  # the call used the counter rows offset .. offset + B - 1
                        XM.append(_rmse_unobserved(xm, x, mask))
                        continue
                    mp = draw_mask_p(model, x.shape, mask, p_missingness, device) if model.regularised else None
                    xm = torch.empty_like(x)
                    for lo in range(0, x.shape[0], rows):
                        xm[lo:lo + rows] = model.impute(x[lo:lo + rows], mask[lo:lo + rows],
                                                        None if mp is None else mp[lo:lo + rows], num_samples=valid_k)
                    XM.append(_rmse_unobserved(xm, x, mask))
                recon.append(torch.stack(XM).mean())
            out[loader_stage] = torch.stack(recon).mean().cpu()
            if save:
                _save(out[loader_stage], miwae_result_path(experiment_type, data_type, vae_type, loader_stage, alpha,
                                                           p_missingness, reg_type))
    return out
