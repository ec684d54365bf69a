"""What each model family states about itself and what the harness decides from it: `regularised`, `X_MEAN_Q`, the trainer
class harness.trainer_class_for picks, and the predicate ensemble.stack_models and harness.train_sweep share.  Every expected
value is a literal written out here.  CPU only: models are built, nothing is launched."""
import pytest
import torch

import vpc_amd as vpc
from vpc_amd import ensemble, harness

TP = {"batch_size": 8, "patience": 1}
D, L, K, H = 6, 10, 4, 16  # obs_dim, latent_dim, EDDI emb_dim, flow hid_dim

# (id, factory, trainer class, regularised, X_MEAN_Q (None: the class does not define it), joins an ensemble)
CASES = [
    ("Reg_VAE", lambda: vpc.Reg_VAE(D, 500, 10, L, TP, "e", "kl_reg"), vpc.FusedTrainer, True, 6, True),
    ("vanilla_VAE", lambda: vpc.vanilla_VAE(D, 500, 10, L, TP, "e"), vpc.FusedTrainer, False, 2, True),
    ("Reg_VAE_mask", lambda: vpc.Reg_VAE_mask(D, 500, 10, L, TP, "e", "kl_reg"), vpc.FusedTrainer, True, 6, False),
    ("vanilla_VAE_mask", lambda: vpc.vanilla_VAE_mask(D, 500, 10, L, TP, "e"), vpc.FusedTrainer, False, 2, False),
    ("Reg_VAE_d129", lambda: vpc.Reg_VAE(129, 500, 10, L, TP, "e", "kl_reg"), vpc.WideTrainer, True, 6, False),
    ("Reg_EDDI", lambda: vpc.Reg_EDDI(D, 500, K, L, TP, "e", "kl_reg"), vpc.EDDITrainer, True, 6, False),
    ("vanilla_EDDI", lambda: vpc.vanilla_EDDI(D, 500, K, L, TP, "e"), vpc.EDDITrainer, False, 2, False),
    ("Reg_EDDI_mnist", lambda: vpc.Reg_EDDI_mnist(D, 500, K, L, TP, "e", "kl_reg"), vpc.EDDIMnistTrainer, True, 6, False),
    ("vanilla_EDDI_mnist", lambda: vpc.vanilla_EDDI_mnist(D, 500, K, L, TP, "e"), vpc.EDDIMnistTrainer, False, 2, False),
    ("REG_notMIWAE_v2", lambda: vpc.REG_notMIWAE_v2(D, 128, 10, L, TP, 3, 1), vpc.NMTrainer, True, None, False),
    ("notMIWAE_myversion", lambda: vpc.notMIWAE_myversion(D, 128, 10, L, TP, 3, 1), vpc.NMTrainer, False, None, False),
    ("Reg_MIWAE", lambda: vpc.Reg_MIWAE(D, 500, 10, L, TP, 3, 1), vpc.MIWTrainer, True, None, False),
    ("MIWAE", lambda: vpc.MIWAE(D, 500, 10, L, TP, 3, 1), vpc.MIWTrainer, False, None, False),
    ("REG_VAEFlow", lambda: vpc.REG_VAEFlow(D, H, 10, L, TP), vpc.FlowTrainer, True, 6, False),
    ("VAEFlow", lambda: vpc.VAEFlow(D, H, 10, L, TP), vpc.FlowTrainer, False, 2, False),
]


@pytest.mark.parametrize("name,make,trainer,regularised,x_mean_q,stackable", CASES, ids=[c[0] for c in CASES])
def test_family_statements(name, make, trainer, regularised, x_mean_q, stackable):
    m = make()
    assert harness.trainer_class_for(m) is trainer
    assert type(m).regularised is regularised
    # the MNAR and MIWAE classes take their imputation from loss() / impute(), not from forward()'s tuple
    assert getattr(type(m), "X_MEAN_Q", None) == x_mean_q
    assert callable(type(m).forward_loss)
    assert ensemble.stackable(m) is stackable


def test_trainer_class_for_refuses_other_modules():
    with pytest.raises(TypeError):
        harness.trainer_class_for(torch.nn.Linear(2, 2))
    assert ensemble.stackable(torch.nn.Linear(2, 2)) is False


def test_wide_comes_after_mnist_and_before_the_families():
    # an image-width EDDI model is never `_wide`, whatever its obs_dim; a wide dense model is, whatever its class
    assert harness.trainer_class_for(vpc.vanilla_EDDI_mnist(784, 500, 20, L, TP, "e")) is vpc.EDDIMnistTrainer
    assert harness.trainer_class_for(vpc.vanilla_VAE_mask(65, 500, 10, L, TP, "e")) is vpc.WideTrainer
    assert harness.trainer_class_for(vpc.vanilla_VAE(14, 500, 10, 16, TP, "e")) is vpc.WideTrainer
