"""Shared by tests/test_ensemble_active_cpu.py and tests/test_ensemble_active_gpu.py: the data, the eps stream and the oracle runs of
the "loop vs oracle" case (d = 128, n = 21, M = 8, three acquisition steps), and the float64 twin of the oracle's port that the
input guard compares against.  Not a test module."""
import numpy as np
import torch

from oracle import vae_oracle as O

L = 10
LOOP = dict(d=128, n=21, M=8, steps=3, train_rows=4096)
LOOP_SEED = 11      # the data (test_gpu_loop_at_full_width_vs_oracle's recipe)
LOOP_EPS_SEED = 5   # the eps stream both loops consume


def loop_data():
    """(x [n, d], training rows [4096, d], training mask [4096, d]): correlated columns, so that a briefly trained encoder
    discriminates between candidates."""
    d, n, rows = LOOP["d"], LOOP["n"], LOOP["train_rows"]
    g = torch.Generator().manual_seed(LOOP_SEED)
    base, mix = torch.rand(n + rows, 4, generator=g), torch.rand(4, d, generator=g)
    data = torch.sigmoid(3.0 * (base @ mix / mix.sum(0) - 0.5)) + 0.05 * torch.rand(n + rows, d, generator=g)
    data = (data - data.min(0).values) / (data.max(0).values - data.min(0).values)
    mt = torch.rand(rows, d, generator=g) < 0.7
    return data[:n].clone(), data[n:].clone(), mt


def loop_eps(G=1):
    """[G, calls, M n, L]: one stream per member, calls = 1 + 2 steps."""
    calls = 1 + 2 * LOOP["steps"]
    g = torch.Generator().manual_seed(LOOP_EPS_SEED)
    return torch.randn(G, calls, LOOP["M"] * LOOP["n"], L, generator=g)


class Port64(O.TorchPort):
    """The oracle's port with float64 arithmetic: the same float32 inputs and parameters, every product and sum in double."""

    def __init__(self, params, latent_dim):
        super().__init__({k: v.double() for k, v in params.items()}, latent_dim)

    def encoder(self, x, mask, eps=None, sample=True):
        p, F = self.p, torch.nn.functional
        h = x.double() * mask.double()
        h = torch.relu(F.linear(h, p["seq_encoder.0.weight"], p["seq_encoder.0.bias"]))
        h = torch.relu(F.linear(h, p["seq_encoder.2.weight"], p["seq_encoder.2.bias"]))
        mean, logvar = F.linear(h, p["seq_encoder.4.weight"], p["seq_encoder.4.bias"]).chunk(2, dim=1)
        z = mean + eps.double() * torch.exp(logvar / 2) if sample else mean
        return z, mean, logvar


def oracle_loop(port, x, eps, M, steps):
    """oracle.active_learning_loop with forward call c, pass m drawing eps[c, m n : (m + 1) n] (the draw rows of the ensemble
    loop's tile table).  eps: [calls, M n, L].  The imputations are float32 whatever the port's arithmetic."""
    n = x.shape[0]
    k = [0]

    def fwd(mask):
        c, m = divmod(k[0], M)
        k[0] += 1
        with torch.no_grad():
            z, _, _ = port.encoder(x, mask > 0.5, eps=eps[c, m * n:(m + 1) * n])
            return port.decoder(z)[0].float()

    with torch.no_grad():
        out = O.active_learning_loop(x, M, fwd, lambda xx, mm, im: O.reward_matrix(port, xx, mm, M, im), max_steps=steps)
    assert k[0] == M * (1 + 2 * steps)
    return out


def history_match(a, b):
    """[steps + 1, n] bool: row i has the same action history in a and b BEFORE step t (row t; row `steps`: after the last)."""
    a, b = np.asarray(a), np.asarray(b)
    steps = a.shape[1]
    return np.stack([np.all(a[:, :t] == b[:, :t], axis=1) for t in range(steps + 1)])


def train_on_cpu(params, xt, mt, steps=200, batch=256, seed=3):
    """Adam(1e-3) on the oracle's Reg_VAE step: the CPU stand-in of the GPU test's brief FusedTrainer run (same data, same
    step count; the guard needs a model of that kind, not that model's bits)."""
    g = torch.Generator().manual_seed(seed)
    P = {k: v.clone() for k, v in params.items()}
    m1 = {k: torch.zeros_like(v) for k, v in P.items()}
    m2 = {k: torch.zeros_like(v) for k, v in P.items()}
    for t in range(1, steps + 1):
        rows = torch.randint(0, xt.shape[0], (batch,), generator=g)
        x, mk = xt[rows], mt[rows]
        mp = mk & (torch.rand(batch, xt.shape[1], generator=g) < 0.7)
        eq, ep = torch.randn(batch, L, generator=g), torch.randn(batch, L, generator=g)
        _, grads, _ = O.torch_reg_step(P, L, x, mk, mp, eq, ep, alpha=1.0, epoch=t)
        for k in P:
            m1[k] = 0.9 * m1[k] + 0.1 * grads[k]
            m2[k] = 0.999 * m2[k] + 0.001 * grads[k] ** 2
            P[k] = P[k] - 1e-3 * (m1[k] / (1 - 0.9 ** t)) / ((m2[k] / (1 - 0.999 ** t)).sqrt() + 1e-8)
    return P
