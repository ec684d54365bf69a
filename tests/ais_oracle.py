"""Plain-torch restatement of the AIS chain of the reference (src/utils/AIS.py:155-217, 237-304), parameterised by dtype,
with every draw injected.  Not the reference's code: the arithmetic written out once, on the CPU, for the parity tests.

    params   the six seq_decoder tensors: {"seq_decoder.{0,2,4}.{weight,bias}"}
    sign     +1: the reference's likelihood quirk (log f = -|z|^2/2 + t * NLL), -1: corrected (real AIS)
"""
import math

import numpy as np
import torch

X_LOGVAR = math.log((0.1 * math.sqrt(2)) ** 2)  # VAE.py:379


def linear_schedule(T):
    return np.linspace(0., 1., T)


def sigmoidial_schedule(T, delta=4):
    def sigmoid(x):
        return np.exp(x) / (1. + np.exp(x))

    def bt(t):
        return sigmoid(delta * (2. * t / T - 1.))

    return [(bt(t) - bt(1)) / (bt(T) - bt(1)) for t in range(1, T + 1)]


def log_mean_exp(x):
    m, _ = torch.max(x, 1, keepdim=True)
    return torch.log(torch.mean(torch.exp(x - m), 1)) + m.squeeze(1)


def decoder(params, z):
    h = torch.relu(z @ params["seq_decoder.0.weight"].T + params["seq_decoder.0.bias"])
    h = torch.relu(h @ params["seq_decoder.2.weight"].T + params["seq_decoder.2.bias"])
    return torch.sigmoid(h @ params["seq_decoder.4.weight"].T + params["seq_decoder.4.bias"])


def nll(params, x, z, x_logvar=X_LOGVAR):
    """Sum over ALL d columns of minus the Gaussian log-density (utils.py:149-151)."""
    mean = decoder(params, z)
    return torch.sum(0.5 * (x - mean) ** 2 * math.exp(-x_logvar) + 0.5 * x_logvar + 0.5 * math.log(2 * math.pi), 1)


def run(params, x, schedule, n_sample, z0, v, u, sign=1.0, dtype=torch.float64, init_step_size=0.01,
        leapfrog_steps=10, grad_clip=1e4, x_logvar=X_LOGVAR):
    """x [nb, d]; z0 [B, L]; v [T-1, B, L]; u [T-1, B] with B = nb * n_sample (chain c = row c % nb).
    Returns a dict: logw, z, epsilon, accept_hist [B]; accept, prob, margin (= |prob - u|) [T-1, B]; clamped (number of
    gradient components the clamp changed)."""
    P = {k: torch.as_tensor(p).to(dtype) for k, p in params.items()}
    xb = torch.as_tensor(x).to(dtype).repeat(n_sample, 1)
    z = torch.as_tensor(z0).to(dtype).clone()
    v = torch.as_tensor(v).to(dtype)
    u = torch.as_tensor(u).to(dtype)
    # the temperatures reach the reference's fp32 tensors as fp32 scalars
    sched = [float(np.float32(t)) for t in np.asarray(schedule, dtype=np.float64)]
    B = z.shape[0]
    eps = torch.full((B,), init_step_size, dtype=dtype)
    hist = torch.zeros(B, dtype=dtype)
    logw = torch.zeros(B, dtype=dtype)
    accepts, probs, margins, clamped = [], [], [], 0

    def log_f(zz, t):
        return -0.5 * (zz * zz).sum(1) + t * sign * nll(P, xb, zz, x_logvar)

    for j, (t0, t1) in enumerate(zip(sched[:-1], sched[1:]), 1):
        with torch.no_grad():
            logw = logw + (log_f(z, t1) - log_f(z, t0))

        def grad_U(zz):
            nonlocal clamped
            zz = zz.detach().requires_grad_(True)
            (g,) = torch.autograd.grad((-log_f(zz, t1)).sum(), zz)
            gc = torch.clamp(g, -grad_clip, grad_clip)
            clamped += int((gc != g).sum())
            return gc

        v0 = v[j - 1]
        e = eps.view(-1, 1)
        zz = z
        vv = v0 - grad_U(zz) * e * 0.5
        for i in range(1, leapfrog_steps + 1):
            zz = zz + vv * e
            if i < leapfrog_steps:
                vv = vv - grad_U(zz) * e
        vv = -(vv - grad_U(zz) * e * 0.5)
        with torch.no_grad():
            h_cur = 0.5 * (v0 * v0).sum(1) - log_f(z, t1)
            h_prop = 0.5 * (vv * vv).sum(1) - log_f(zz, t1)
            prob = torch.exp(h_cur - h_prop)
            acc = prob > u[j - 1]
            z = torch.where(acc.view(-1, 1), zz, z).detach()
            hist = hist + acc.to(dtype)
            adapt = torch.where(hist / j > 0.65, torch.tensor(1.02, dtype=dtype), torch.tensor(0.98, dtype=dtype))
            eps = (eps * adapt).clamp(1e-4, 0.5)
        accepts.append(acc)
        probs.append(prob)
        margins.append((prob - u[j - 1]).abs())
    return dict(logw=logw, z=z, epsilon=eps, accept_hist=hist, accept=torch.stack(accepts), prob=torch.stack(probs),
                margin=torch.stack(margins), clamped=clamped)


def batch_mean(logw, n_sample, mode="forward"):
    """AIS.py:220-223."""
    lw = log_mean_exp(logw.view(n_sample, -1).transpose(0, 1))
    return (-lw if mode == "backward" else lw).mean()
