"""Plain-torch restatement of the AIS chain of the reference (src/utils/AIS.py:155-217, 237-304) for ANY Gaussian decoder:
the chain of tests/ais_oracle.py generalised to a decoder description and an optional mask, parameterised by dtype, with
every draw injected.  Not the reference's code: the arithmetic written out once, on the CPU, for the parity tests.

A decoder description is a dict
    weights    [W1, b1, W2, b2, ..] (each W [N, K])
    acts       the activation of every layer: "relu" | "elu" | "sigmoid" | "sigmoid_hardtanh" | "none"
               ("sigmoid_hardtanh": the merged [mean d | logvar d] head, Sigmoid | Hardtanh(-10, 0), VAE.py:2359-2363)
    x_logvar   the scalar log-variance, or None when the last layer is the merged head
The NLL is the sum over the columns of MINUS the Gaussian log-density (utils.py:149-151), each term times mask [nb, d]
(0/1) when one is given.  With a dense description (relu, relu, sigmoid; scalar x_logvar) and no mask every operation is
the one of ais_oracle.run in the same order: the two are bit-equal.
"""
import math

import numpy as np
import torch

ACTS = {"relu": torch.relu, "elu": torch.nn.functional.elu, "sigmoid": torch.sigmoid, "none": lambda t: t}


def describe(weights, acts, x_logvar):
    return dict(weights=list(weights), acts=tuple(acts), x_logvar=x_logvar)


def dense(params, x_logvar):
    """The latent -> 50 -> 100 -> d chain of ais_oracle.decoder from its six seq_decoder tensors."""
    w = [params[f"seq_decoder.{i}.{k}"] for i in (0, 2, 4) for k in ("weight", "bias")]
    return describe(w, ("relu", "relu", "sigmoid"), x_logvar)


def decoder(desc, z):
    """(mean, logvar): logvar a tensor for the merged head, else the description's scalar."""
    h, w = z, desc["weights"]
    for i, act in enumerate(desc["acts"]):
        h = h @ w[2 * i].T + w[2 * i + 1]
        if act == "sigmoid_hardtanh":
            d = h.shape[1] // 2
            return torch.sigmoid(h[:, :d]), torch.nn.functional.hardtanh(h[:, d:], -10.0, 0.0)
        h = ACTS[act](h)
    return h, desc["x_logvar"]


def nll(desc, x, z, mask=None):
    mean, lv = decoder(desc, z)
    if isinstance(lv, torch.Tensor):
        t = 0.5 * (x - mean) ** 2 * torch.exp(-lv) + 0.5 * lv + 0.5 * math.log(2 * math.pi)
    else:
        t = 0.5 * (x - mean) ** 2 * math.exp(-lv) + 0.5 * lv + 0.5 * math.log(2 * math.pi)
    if mask is not None:
        t = t * mask
    return torch.sum(t, 1)


def run(desc, x, schedule, n_sample, z0, v, u, sign=1.0, dtype=torch.float64, init_step_size=0.01, leapfrog_steps=10,
        grad_clip=1e4, mask=None):
    """x [nb, d]; mask [nb, d] or None; z0 [B, L]; v [T-1, B, L]; u [T-1, B] with B = nb * n_sample (chain c = row c % nb).
    Returns a dict: logw, z, epsilon, accept_hist [B]; accept, prob, margin (= |prob - u|) [T-1, B]; clamped (number of
    gradient components the clamp changed)."""
    D = dict(desc, weights=[torch.as_tensor(p).to(dtype) for p in desc["weights"]])
    xb = torch.as_tensor(x).to(dtype).repeat(n_sample, 1)
    mb = None if mask is None else torch.as_tensor(mask).to(dtype).repeat(n_sample, 1)
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
        return -0.5 * (zz * zz).sum(1) + t * sign * nll(D, xb, zz, mb)

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
