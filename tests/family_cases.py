"""The reference's forward -> loss call of every model family, written out by hand in the reference's positional order, and
one small model of every class.  test_forward_loss_gpu.py, test_train_loop_gpu.py and test_eval_loop_gpu.py check the
package's forward_loss / train / eval_* against these; nothing here calls forward_loss."""
import torch

import vpc_amd as vpc

TP = {"batch_size": 16, "patience": 1}
L = 10


def dense_reg(m, x, mask, mask_p, *, epoch, alpha, beta, beta_annealing, alpha_annealing, stage, **extra):
    # train.py:87-94 / evaluate.py:210-216 (Reg_VAE, Reg_VAE_mask, Reg_EDDI, Reg_EDDI_mnist, REG_notMIWAE_v2)
    o = m.forward(x, mask, mask_p, stage=stage)
    return o, m.loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mask, mask_p, epoch, beta_annealing=beta_annealing,
                     beta=beta, alpha=alpha, alpha_annealing=alpha_annealing, stage=stage, **extra)


def dense_van(m, x, mask, mask_p, *, epoch, alpha, beta, beta_annealing, alpha_annealing, stage, **extra):
    # train.py:95-101 / evaluate.py:219-227 (vanilla_VAE, vanilla_VAE_mask, vanilla_EDDI, vanilla_EDDI_mnist, notMIWAE_myversion)
    o = m.forward(x, mask)
    return o, m.loss(x, o[2], o[3], o[0], o[1], epoch, mask, beta_annealing=beta_annealing, beta=beta, stage=stage, **extra)


def miw_reg(m, x, mask, mask_p, *, epoch, alpha, beta, beta_annealing, alpha_annealing, stage, **extra):
    # train.py:102-108 / evaluate.py:97-103
    o = m.forward(x, mask, mask_p)
    return o, m.loss(x, o[2], o[3], o[4], o[0], o[1], o[7], o[8], o[9], o[5], o[6], mask, mask_p, epoch,
                     beta_annealing=beta_annealing, beta=beta, alpha=alpha, **extra)


def miw_van(m, x, mask, mask_p, *, epoch, alpha, beta, beta_annealing, alpha_annealing, stage, **extra):
    o = m.forward(x, mask)
    if extra:  # evaluate.py:106-112
        return o, m.loss(x, o[2], o[3], o[4], o[0], o[1], mask, epoch, beta_annealing=beta_annealing, beta=beta, **extra)
    return o, m.loss(x, o[2], o[3], o[4], o[0], o[1], mask, epoch)  # train.py:109-113


def flow_reg(m, x, mask, mask_p, *, epoch, alpha, beta, beta_annealing, alpha_annealing, stage, **extra):
    # train.py:77-81 / evaluate.py:189-195
    o = m.forward(x, mask, mask_p)
    return o, m.loss(x, o[6], o[7], o[4], o[5], o[2], o[3], o[0], o[1], mask, mask_p, alpha, stage=stage, **extra)


def flow_van(m, x, mask, mask_p, *, epoch, alpha, beta, beta_annealing, alpha_annealing, stage, **extra):
    # train.py:82-85 / evaluate.py:196-200
    o = m.forward(x, mask)
    return o, m.loss(x, o[2], o[3], o[0], o[1], mask, **extra)


# class name -> (factory(d), the reference's call, obs_dim, batch rows)
FAMILIES = {
    "Reg_VAE": (lambda d: vpc.Reg_VAE(d, 500, 10, L, TP, "e", "kl_reg"), dense_reg, 14, 16),
    "vanilla_VAE": (lambda d: vpc.vanilla_VAE(d, 500, 10, L, TP, "e"), dense_van, 14, 16),
    "Reg_VAE_mask": (lambda d: vpc.Reg_VAE_mask(d, 500, 10, L, TP, "e", "ml_reg"), dense_reg, 14, 16),
    "vanilla_VAE_mask": (lambda d: vpc.vanilla_VAE_mask(d, 500, 10, L, TP, "e"), dense_van, 14, 16),
    "Reg_EDDI": (lambda d: vpc.Reg_EDDI(d, 500, 10, L, TP, "e", "kl_reg"), dense_reg, 14, 16),
    "vanilla_EDDI": (lambda d: vpc.vanilla_EDDI(d, 500, 10, L, TP, "e"), dense_van, 14, 16),
    "Reg_EDDI_mnist": (lambda d: vpc.Reg_EDDI_mnist(d, 500, 20, L, TP, "e", "kl_reg"), dense_reg, 784, 4),
    "vanilla_EDDI_mnist": (lambda d: vpc.vanilla_EDDI_mnist(d, 500, 20, L, TP, "e"), dense_van, 784, 4),
    "REG_notMIWAE_v2": (lambda d: vpc.REG_notMIWAE_v2(d, 500, 10, L, TP, 5, 1), dense_reg, 14, 16),
    "notMIWAE_myversion": (lambda d: vpc.notMIWAE_myversion(d, 500, 10, L, TP, 5, 1), dense_van, 14, 16),
    "Reg_MIWAE": (lambda d: vpc.Reg_MIWAE(d, 500, 10, L, TP, 5, 1), miw_reg, 14, 16),
    "MIWAE": (lambda d: vpc.MIWAE(d, 500, 10, L, TP, 5, 1), miw_van, 14, 16),
    "REG_VAEFlow": (lambda d: vpc.REG_VAEFlow(d, 64, 10, L, TP), flow_reg, 12, 16),
    "VAEFlow": (lambda d: vpc.VAEFlow(d, 64, 10, L, TP), flow_van, 12, 16),
}


def batches(n, B, d, seed=0, float_mask=False):
    """n fixed (x, mask) batches of B rows on the device."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x, m = torch.rand(B, d, generator=g), torch.rand(B, d, generator=g) < 0.7
        out.append((x.cuda(), (m.float() if float_mask else m).cuda()))
    return out


def same(a, b, what=""):
    """Two tuples of tensors / numbers, element by element, exactly."""
    assert len(a) == len(b), what
    for i, (s, t) in enumerate(zip(a, b)):
        if isinstance(s, torch.Tensor):
            assert isinstance(t, torch.Tensor) and s.shape == t.shape and torch.equal(s, t), (what, i)
        else:
            assert not isinstance(t, torch.Tensor) and s == t, (what, i)
