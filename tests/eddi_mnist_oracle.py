"""CPU oracle for the MNIST point-net pair Reg_EDDI_mnist / vanilla_EDDI_mnist (reference src/models/VAE.py:10-347).

THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE (only tests/ and bench baselines may import it).

``EDDIMnistPort`` restates the two reference classes op for op on stock PyTorch CPU: the point-net front-end of
``oracle.eddi_oracle.EDDIPort`` (it is the same expression at any width), the trunk K -> 500 -> 500 -> 200 -> 2L, the decoder
L -> 200 -> 500 -> 500 -> d -> Sigmoid, and the losses of Reg_VAE / vanilla_VAE, which these classes share term for term
(VAE.py:92-162 against :403-467) - the vanilla class computing RE_q_imputed in every call (VAE.py:294-295).
``closed_form_step`` is an independent float64 numpy statement of one whole step (folded front-end, hand-derived
gradients of all 20 tensors); ``sampled`` is the strided view the goldens store of the five large matrices.

Pinned by tests/test_eddi_mnist_oracle.py against tests/golden/eddi_mnist_*.npz (tests/golden/make_golden_eddi_mnist.py runs
the reference itself).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle.eddi_oracle import EDDIPort, front_closed_form

MAX_EPOCH = 2800
X_LOGVAR = float(torch.log(torch.square(torch.Tensor([0.1 * np.sqrt(2)]))))  # VAE.py:47: the fp32 value of log 0.02
HL = 0.5 * math.log(2.0 * math.pi)
STRIDE = 97  # the goldens keep every 97th element of the flattened large matrices
SAMPLED = ("pnp_encoder2.2.weight", "pnp_encoder2.4.weight", "seq_decoder.2.weight", "seq_decoder.4.weight",
           "seq_decoder.6.weight")
KEYS = (
    "type_pars1", "type_bias1", "pnp_encoder1.0.weight", "pnp_encoder1.0.bias",
    "pnp_encoder2.0.weight", "pnp_encoder2.0.bias", "pnp_encoder2.2.weight", "pnp_encoder2.2.bias",
    "pnp_encoder2.4.weight", "pnp_encoder2.4.bias", "pnp_encoder2.6.weight", "pnp_encoder2.6.bias",
    "seq_decoder.0.weight", "seq_decoder.0.bias", "seq_decoder.2.weight", "seq_decoder.2.bias",
    "seq_decoder.4.weight", "seq_decoder.4.bias", "seq_decoder.6.weight", "seq_decoder.6.bias",
)
STATE_KEYS = KEYS[:2] + ("prior_mean", "prior_std") + KEYS[2:]  # state_dict order of both classes


def sampled(a):
    """Every STRIDE-th element of the flattened array (numpy or torch)."""
    return a.reshape(-1)[::STRIDE]


def stored(key, a):
    """What a golden holds for tensor `key`: the strided sample for the large matrices, the tensor itself otherwise."""
    return sampled(a) if key in SAMPLED else a


class EDDIMnistPort(EDDIPort):
    def encoder(self, x, mask, eps=None, sample=True):  # VAE.py:62-84
        p = self.p
        h = self.front(x, mask)
        for i in (0, 2, 4):
            h = torch.relu(torch.nn.functional.linear(h, p[f"pnp_encoder2.{i}.weight"], p[f"pnp_encoder2.{i}.bias"]))
        h = torch.nn.functional.linear(h, p["pnp_encoder2.6.weight"], p["pnp_encoder2.6.bias"])
        mean, logvar = h.chunk(2, dim=1)
        if not sample:
            return mean, mean, logvar
        std = torch.exp(logvar / 2)
        z = mean + (torch.randn_like(std) if eps is None else eps) * std
        return z, mean, logvar

    def decoder(self, z):  # VAE.py:86-90
        p = self.p
        g = z
        for i in (0, 2, 4):
            g = torch.relu(torch.nn.functional.linear(g, p[f"seq_decoder.{i}.weight"], p[f"seq_decoder.{i}.bias"]))
        return torch.sigmoid(torch.nn.functional.linear(g, p["seq_decoder.6.weight"], p["seq_decoder.6.bias"])), self.x_logvar


def port_step(params, Ld, x, mask, mask_p, eps, *, reg_type="kl_reg", alpha=0.5, beta=1.0, beta_annealing=False, epoch=1,
              eps_ml=None, dtype=torch.float32):
    """One forward + loss + autograd backward of the port.  mask_p None: the vanilla class.  eps [P, B, L].
    Returns (loss tensor, {key: grad})."""
    p = {k: params[k].detach().clone().to(dtype).requires_grad_(True) for k in KEYS}
    port = EDDIMnistPort(p, Ld, reg_type)
    port.x_logvar = port.x_logvar.to(dtype)
    x = x.to(dtype)
    eps = eps.to(dtype)
    if mask_p is None:
        o = port.vanilla_forward(x, mask, eps[0])
        _, tl = port.vanilla_loss(x, o[2], o[3], o[0], o[1], epoch, mask, beta=beta, beta_annealing=beta_annealing)
    else:
        o = port.reg_forward(x, mask, mask_p, eps[0], eps[1])
        _, tl = port.reg_loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mask, mask_p, epoch, beta=beta,
                              alpha=alpha, beta_annealing=beta_annealing, eps_ml=None if eps_ml is None else eps_ml.to(dtype))
    tl.backward()
    return tl.detach(), {k: v.grad.detach() for k, v in p.items()}


# ------------------------------------------------------------------------------------------------ float64 closed form
def front_chunked(x, mask, E, tb, Wp, cp, dagg=None, rows=256):
    """oracle.eddi_oracle.front_closed_form over chunks of `rows` batch rows: the [B, d, K] float64 intermediates of a
    B = 4096, d = 1024 batch would not fit.  agg rows are independent and the parameter gradients are sums over rows."""
    B = x.shape[0]
    aggs, grads = [], None
    for lo in range(0, B, rows):
        sl = slice(lo, lo + rows)
        r = front_closed_form(x[sl], mask[sl], E, tb, Wp, cp, None if dagg is None else dagg[sl])
        if dagg is None:
            aggs.append(r)
            continue
        aggs.append(r[0])
        grads = r[1] if grads is None else {k: grads[k] + v for k, v in r[1].items()}
    agg = np.concatenate(aggs, 0)
    return agg if dagg is None else (agg, grads)


def front_near_kink(x, E, tb, Wp, cp, tol=1e-4, rows=256):
    """[B, d] bool: entries whose pre-activation x_bj A_j[k] + C_j[k] lies within `tol` of the ReLU kink for some k.  There the
    derivative is not defined and an fp32 evaluation (rounding ~1e-7 |x A| + |C|) may take the other branch than float64 does;
    gradient comparisons against the float64 oracle mask such entries out of the input."""
    x = x.astype(np.float64)
    E, tb, Wp, cp = (t.astype(np.float64) for t in (E, tb, Wp, cp))
    K = E.shape[1]
    A = Wp[:, 0][None, :] + E @ Wp[:, 1:1 + K].T
    C = tb * Wp[:, 1 + K][None, :] + cp[None, :]
    out = np.zeros(x.shape, dtype=bool)
    for lo in range(0, x.shape[0], rows):
        pre = x[lo:lo + rows, :, None] * A[None] + C[None]
        out[lo:lo + rows] = (np.abs(pre) < tol).any(2)
    return out


def _np64(params):
    return {k: np.asarray(params[k].detach().cpu().numpy() if torch.is_tensor(params[k]) else params[k], dtype=np.float64)
            for k in KEYS}


def _mlp_fwd(P, names, h, last, gate_fn=None):
    """Activations and ReLU gates of one MLP.  gate_fn(layer name, pre, S) -> bool gates, S = |input| |W|^T + |b| the
    magnitude sum of each dot product (None: pre > 0)."""
    acts, gates = [h], []
    for i, n in enumerate(names):
        W, b = P[n + ".weight"], P[n + ".bias"]
        pre = acts[-1] @ W.T + b
        if i < len(names) - 1:
            g = pre > 0 if gate_fn is None else gate_fn(n, pre, np.abs(acts[-1]) @ np.abs(W).T + np.abs(b))
            gates.append(g)
            acts.append(np.where(g, pre, 0.0))
        else:
            acts.append(1.0 / (1.0 + np.exp(-pre)) if last == "sigmoid" else pre)
    return acts, gates


def _mlp_bwd(P, names, acts, gates, dy, last, grads):
    """dy = d loss / d output; returns d loss / d input, adds the weight gradients to `grads`."""
    if last == "sigmoid":
        dy = dy * acts[-1] * (1.0 - acts[-1])
    for i in range(len(names) - 1, -1, -1):
        n = names[i]
        grads[n + ".weight"] = grads.get(n + ".weight", 0.0) + dy.T @ acts[i]
        grads[n + ".bias"] = grads.get(n + ".bias", 0.0) + dy.sum(0)
        dy = dy @ P[n + ".weight"]
        if i > 0:
            dy = dy * gates[i - 1]
    return dy


def kink_band(n_terms, S):
    """Half-width of the band around a ReLU kink inside which an fp32 dot product of n_terms terms with magnitude sum S cannot
    be trusted to have the sign of the exact value: 2 sqrt(n) 2^-24 S (a blocked fp32 sum's rounding, and as much again for
    the rounding its fp32 inputs already carry)."""
    return 2.0 * math.sqrt(n_terms) * 2.0 ** -24 * S


_TR = ["pnp_encoder2.0", "pnp_encoder2.2", "pnp_encoder2.4", "pnp_encoder2.6"]
_DE = ["seq_decoder.0", "seq_decoder.2", "seq_decoder.4", "seq_decoder.6"]


def closed_form_step(params, Ld, x, mask, mask_p, eps, *, reg_type="kl_reg", alpha=0.5, beta=1.0, beta_annealing=False,
                     epoch=1, eps_ml=None, device_gates=None, stats=None):
    """float64 loss and hand-derived gradients of one step (numpy).  mask_p None: vanilla.  eps [P, B, L].
    device_gates {(pass, layer name): bool [B, n]} (optional): the side of the ReLU an fp32 implementation took.  The
    derivative of ReLU at 0 is any value in [0, 1], and a pre-activation inside kink_band() of 0 has no sign that fp32 can
    resolve; for those units - and only those - the gate is the implementation's, everywhere else it is pre > 0 in float64.
    stats (a dict): receives the number of units inside the band and of those gated the other way than float64."""
    P = _np64(params)
    x = np.asarray(x, dtype=np.float64)
    B, d = x.shape
    var = math.exp(X_LOGVAR)
    bw = (epoch / MAX_EPOCH) * beta if beta_annealing else beta
    masks = [np.asarray(mask) != 0] + ([np.asarray(mask_p) != 0] if mask_p is not None else [])
    eps = np.asarray(eps, dtype=np.float64)
    passes = []

    def gate_fn_for(p_):
        if device_gates is None:
            return None

        def fn(name, pre, S):
            amb = np.abs(pre) <= kink_band(P[name + ".weight"].shape[1], S)
            dev = np.asarray(device_gates[(p_, name)], dtype=bool)
            if stats is not None:
                stats["in_band"] = stats.get("in_band", 0) + int(amb.sum())
                stats["taken_from_device"] = stats.get("taken_from_device", 0) + int((amb & (dev != (pre > 0))).sum())
            return np.where(amb, dev, pre > 0)
        return fn
    for p_, m in enumerate(masks):
        agg = front_chunked(x, m, P["type_pars1"], P["type_bias1"], P["pnp_encoder1.0.weight"], P["pnp_encoder1.0.bias"])
        ta, tg = _mlp_fwd(P, _TR, agg, None, gate_fn_for(p_))
        mean, lv = ta[-1][:, :Ld], ta[-1][:, Ld:]
        std = np.exp(lv / 2)
        z = mean + eps[p_] * std
        da, dg = _mlp_fwd(P, _DE, z, "sigmoid", gate_fn_for(p_))
        passes.append(dict(m=m, agg=agg, ta=ta, tg=tg, dg=dg, mean=mean, lv=lv, std=std, z=z, da=da, xhat=da[-1]))

    def nll(w, xhat):  # sum over ALL entries of the reference's masked Normal NLL, and its gradient in xhat
        w = w.astype(np.float64)
        val = (HL + w * (0.5 * X_LOGVAR + (x - xhat) ** 2 / (2 * var))).sum()
        return val, -w * (x - xhat) / var

    kl0 = lambda mean, lv: (0.5 * (np.exp(lv) + mean ** 2 - 1.0 - lv)).sum()
    q = passes[0]
    dxhat = [np.zeros_like(x) for _ in passes]
    dmean = [np.zeros((B, Ld)) for _ in passes]
    dlv = [np.zeros((B, Ld)) for _ in passes]

    def add_nll(c, w, p_):
        v, g = nll(w, passes[p_]["xhat"])
        dxhat[p_] += c * g
        return c * v

    def add_kl0(c, p_):
        pp = passes[p_]
        dmean[p_] += c * pp["mean"]
        dlv[p_] += c * 0.5 * (np.exp(pp["lv"]) - 1.0)
        return c * kl0(pp["mean"], pp["lv"])

    if mask_p is None:
        loss = add_nll(1.0, q["m"], 0) + add_kl0(bw, 0)
    elif reg_type == "kl_reg":
        pp = passes[1]
        loss = add_nll(1.0 - alpha, q["m"], 0) + add_kl0((1.0 - alpha) * bw, 0)
        loss += add_nll(alpha, pp["m"], 1) + add_kl0(alpha * bw, 1)
        loss += add_nll(alpha, q["m"] & ~pp["m"], 0)
        # KL(q || p) = sum 0.5 (lv_p - lv_q) + (var_q + (mq - mp)^2) / (2 var_p) - 0.5
        vq, vp, dm = np.exp(q["lv"]), np.exp(pp["lv"]), q["mean"] - pp["mean"]
        loss += alpha * (0.5 * (pp["lv"] - q["lv"]) + (vq + dm ** 2) / (2 * vp) - 0.5).sum()
        dmean[0] += alpha * dm / vp
        dmean[1] += -alpha * dm / vp
        dlv[0] += alpha * (-0.5 + vq / (2 * vp))
        dlv[1] += alpha * (0.5 - (vq + dm ** 2) / (2 * vp))
    elif reg_type == "ml_reg":
        pp = passes[1]
        loss = add_nll(1.0, q["m"], 0) + add_kl0(bw, 0)
        w = (epoch / MAX_EPOCH) * alpha
        e3 = np.asarray(eps_ml, dtype=np.float64)
        zq = q["mean"] + e3 * q["std"]
        vp = np.exp(pp["lv"])
        r = zq - pp["mean"]
        loss += -w * (-HL - 0.5 * pp["lv"] - r ** 2 / (2 * vp)).sum()
        dzq = w * r / vp
        dmean[0] += dzq
        dlv[0] += dzq * e3 * q["std"] * 0.5
        dmean[1] += -w * r / vp
        dlv[1] += w * (0.5 - r ** 2 / (2 * vp))
    else:
        raise ValueError(reg_type)
    grads = {}
    E, tb, Wp, cp = P["type_pars1"], P["type_bias1"], P["pnp_encoder1.0.weight"], P["pnp_encoder1.0.bias"]
    for p_, pp in enumerate(passes):
        dz = _mlp_bwd(P, _DE, pp["da"], pp["dg"], dxhat[p_] / B, "sigmoid", grads)
        dm = dmean[p_] / B + dz
        dl = dlv[p_] / B + dz * eps[p_] * pp["std"] * 0.5
        dagg = _mlp_bwd(P, _TR, pp["ta"], pp["tg"], np.concatenate([dm, dl], 1), None, grads)
        _, fg = front_chunked(x, pp["m"], E, tb, Wp, cp, dagg)
        for k, v in fg.items():
            grads[k] = grads.get(k, 0.0) + v
    return loss / B, grads


class TorchTrainer:
    """The reference's training sequence on the port: forward, loss, autograd backward, torch.optim.Adam (train.py:21, 87-117)."""

    def __init__(self, params, Ld, reg_type="kl_reg", vanilla=False, lr=1e-3, dtype=torch.float32):
        self.p = {k: params[k].detach().clone().to(dtype).requires_grad_(True) for k in KEYS}
        self.port = EDDIMnistPort(self.p, Ld, reg_type)
        self.port.x_logvar = self.port.x_logvar.to(dtype)
        self.vanilla, self.dtype = vanilla, dtype
        self.opt = torch.optim.Adam([self.p[k] for k in KEYS], lr=lr)

    def step(self, x, mask, mask_p, eps, *, epoch=1, alpha=0.5, beta=1.0, beta_annealing=False):
        port, x, eps = self.port, x.to(self.dtype), eps.to(self.dtype)
        if self.vanilla:
            o = port.vanilla_forward(x, mask, eps[0])
            _, tl = port.vanilla_loss(x, o[2], o[3], o[0], o[1], epoch, mask, beta=beta, beta_annealing=beta_annealing)
        else:
            o = port.reg_forward(x, mask, mask_p, eps[0], eps[1])
            _, tl = port.reg_loss(x, o[2], o[3], o[0], o[1], o[6], o[7], o[4], o[5], mask, mask_p, epoch, beta=beta,
                                  alpha=alpha, beta_annealing=beta_annealing)
        self.opt.zero_grad()
        tl.backward()
        self.opt.step()
        return float(tl.item())
