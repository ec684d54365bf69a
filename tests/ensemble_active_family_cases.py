"""Shared by tests/test_ensemble_active_families_{cpu,gpu}.py: the mask-augmented and point-net twins of ensemble_active_cases -
the data of its "loop vs oracle" case at any width, the eps stream, the oracle ports of the two families in float32 and float64
arithmetic, and the CPU stand-in of the GPU test's brief training run.  Not a test module."""
import torch

from family_eval_cases import L, build, params_of
from oracle import eddi_oracle as EO
from oracle import vae_oracle as O

LOOP = dict(n=21, M=8, steps=3, train_rows=4096)
LOOP_SEED = 11      # the data (ensemble_active_cases.loop_data's recipe)
LOOP_EPS_SEED = 5   # the eps stream both loops consume
# the loop cases: (family, obs_dim, emb_dim); the GPU loop test runs the two at d = 40, the input guard all four
LOOP_CASES = [("mask", 40, 0), ("mask", 14, 0), ("eddi", 40, 10), ("eddi", 14, 20)]


def loop_data(d):
    """ensemble_active_cases.loop_data at width d: (x [n, d], training rows [4096, d], training mask [4096, d])."""
    n, rows = LOOP["n"], LOOP["train_rows"]
    g = torch.Generator().manual_seed(LOOP_SEED)
    base, mix = torch.rand(n + rows, 4, generator=g), torch.rand(4, d, generator=g)
    data = torch.sigmoid(3.0 * (base @ mix / mix.sum(0) - 0.5)) + 0.05 * torch.rand(n + rows, d, generator=g)
    data = (data - data.min(0).values) / (data.max(0).values - data.min(0).values)
    mt = torch.rand(rows, d, generator=g) < 0.7
    return data[:n].clone(), data[n:].clone(), mt


def loop_eps(G=1):
    """[G, calls, M n, L]: one stream per member, calls = 1 + 2 steps."""
    g = torch.Generator().manual_seed(LOOP_EPS_SEED)
    return torch.randn(G, 1 + 2 * LOOP["steps"], LOOP["M"] * LOOP["n"], L, generator=g)


def port(family, params):
    """The oracle's float32 port of a family's model."""
    return EO.EDDIPort(params, L) if family == "eddi" else O.TorchPort(params, L, mask_augm=True)


class MaskPort64(O.TorchPort):
    """TorchPort(mask_augm=True) with float64 arithmetic: the same float32 inputs and parameters, every product and sum in double."""

    def __init__(self, params, latent_dim):
        super().__init__({k: v.double() for k, v in params.items()}, latent_dim, mask_augm=True)

    def encoder(self, x, mask, eps=None, sample=True):
        p, F = self.p, torch.nn.functional
        m = mask.double()
        h = torch.stack([x.double() * m, m], 1).reshape(-1, 2 * x.shape[1])  # VAE.py:545-548, as TorchPort states it
        h = torch.relu(F.linear(h, p["seq_encoder.0.weight"], p["seq_encoder.0.bias"]))
        h = torch.relu(F.linear(h, p["seq_encoder.2.weight"], p["seq_encoder.2.bias"]))
        mean, logvar = F.linear(h, p["seq_encoder.4.weight"], p["seq_encoder.4.bias"]).chunk(2, dim=1)
        z = mean + eps.double() * torch.exp(logvar / 2) if sample else mean
        return z, mean, logvar


def port64(family, params):
    """... and its float64 twin (EDDIPort computes in the dtype of its parameters)."""
    return EO.EDDIPort({k: v.double() for k, v in params.items()}, L) if family == "eddi" else MaskPort64(params, L)


def init_params(family, d, K):
    """The parameters of a CPU Reg_VAE_mask / Reg_EDDI built after torch.manual_seed(3)."""
    torch.manual_seed(3)
    return params_of(build(family, "reg", d, K or 10))


def train_on_cpu(family, params, xt, mt, steps=200, batch=256, seed=3):
    """Adam(1e-3) on the oracle port's reg_forward / reg_loss at alpha = 1: the CPU stand-in of the GPU test's brief trainer run
    (same data, same step count; the guard needs a model of that kind, not that model's bits)."""
    g = torch.Generator().manual_seed(seed)
    leaf = O.make_leaf_params(params)
    pt = port(family, leaf)
    opt = torch.optim.Adam(list(leaf.values()), lr=1e-3)
    for t in range(1, steps + 1):
        rows = torch.randint(0, xt.shape[0], (batch,), generator=g)
        x, mk = xt[rows], mt[rows]
        mp = mk & (torch.rand(batch, xt.shape[1], generator=g) < 0.7)
        eq, ep = torch.randn(batch, L, generator=g), torch.randn(batch, L, generator=g)
        mean_p, logvar_p, xp, xlp, mean_q, logvar_q, xq, xlq = pt.reg_forward(x, mk, mp, eq, ep)
        _, loss = pt.reg_loss(x, xp, xlp, mean_p, logvar_p, xq, xlq, mean_q, logvar_q, mk, mp, t, alpha=1.0)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return {k: v.detach().clone() for k, v in leaf.items()}
