"""float64 restatement of the MIWAE path (MIWAE src/models/VAE.py:3011-3134, Reg_MIWAE :3137-3301) for the tests:
forward, the Student-t importance-weighted bound with the reference's row / sample pairing or the per-row pairing, the
llh_eval imputation and the closed-form gradients that csrc/vpc_miw.hip implements.

Pairing (module docstring of miwae.py): the likelihood sums are built in (row, sample) order and reshaped to [S, B], the
prior / posterior terms are [B, S].permute(1, 0); slot (i, j) of the bound pairs flat likelihood row i*B + j with the
prior / posterior term of row j, sample i.  "per_row" pairs both terms of row j, sample i.
"""
import math

import torch
import torch.nn.functional as F

KEYS = [f"seq_encoder.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")] + \
       [f"seq_decoder.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")]


def params64(src, prefix="param.", requires_grad=False):
    """The 12 state_dict tensors of a fixture dict as float64 leaves."""
    return {k: torch.as_tensor(src[prefix + k]).double().clone().requires_grad_(requires_grad) for k in KEYS}


def _mlp(p, pre, h):
    h = F.relu(F.linear(h, p[f"{pre}.0.weight"], p[f"{pre}.0.bias"]))
    h = F.relu(F.linear(h, p[f"{pre}.2.weight"], p[f"{pre}.2.bias"]))
    return F.linear(h, p[f"{pre}.4.weight"], p[f"{pre}.4.bias"])


def encode(p, x, mask, eps):
    """-> mean, scale [B, L], z [B, S, L] (eps [B, S, L])."""
    mean, raw = _mlp(p, "seq_encoder", x.double() * mask.double()).chunk(2, dim=1)
    scale = F.softplus(raw)
    return mean, scale, mean[:, None, :] + scale[:, None, :] * eps.double()


def decode(p, z):
    mu, sc, v = _mlp(p, "seq_decoder", z).chunk(3, dim=-1)
    return torch.sigmoid(mu), F.softplus(sc) + 0.001, F.softplus(v) + 3


def student_lp(x, mu, sc, v):
    y = (x - mu) / sc
    return (torch.lgamma((v + 1) / 2) - torch.lgamma(v / 2) - 0.5 * torch.log(v) - 0.5 * math.log(math.pi)
            - torch.log(sc) - (v + 1) / 2 * torch.log1p(y * y / v))


def slot_matrix(x, m, dec, mean, scale, e2, pairing):
    """a [S, B] of one pass: likelihood term + (logpz - logq) of the fresh draw z2 = mean + scale * e2."""
    B, S, d = dec[0].shape
    lp = student_lp(x.double()[:, None, :], *dec)                        # [B, S, d]
    lpo = (lp * m.double()[:, None, :]).sum(-1)                          # [B, S]
    z2 = mean[:, None, :] + scale[:, None, :] * e2.double()
    lpz = (-0.5 * z2 * z2 - 0.5 * math.log(2 * math.pi)).sum(-1)
    lq = (-((z2 - mean[:, None, :]) ** 2) / (2 * scale[:, None, :] ** 2) - torch.log(scale[:, None, :])
          - 0.5 * math.log(2 * math.pi)).sum(-1)
    lw = (lpz - lq).permute(1, 0)                                        # [S, B]
    if pairing == "reference":
        return lpo.reshape(S, B) + lw
    return lpo.permute(1, 0) + lw


def loss(x, mask, mask_p, q, p, eps2, alpha=1.0, pairing="reference"):
    """q / p = (dec (mu, sc, v) [B,S,d] each, mean [B,L], scale [B,L]); eps2 = fresh draws [P][B,S,L].  Returns the loss
    and the q-pass slot matrix."""
    a_q = slot_matrix(x, mask, q[0], q[1], q[2], eps2[0], pairing)
    nb_q = -torch.logsumexp(a_q, 0).mean()
    if p is None:
        return nb_q, a_q
    a_p = slot_matrix(x, mask_p, p[0], p[1], p[2], eps2[1], pairing)
    nb_p = -torch.logsumexp(a_p, 0).mean()
    lp_q = student_lp(x.double()[:, None, :], *q[0])
    reg_like = (lp_q * mask.double()[:, None, :] * (1 - mask_p.double())[:, None, :]).sum(-1).mean()
    vr = (q[2] / p[2]) ** 2
    t1 = ((q[1] - p[1]) / p[2]) ** 2
    kl = (0.5 * (vr + t1 - 1 - torch.log(vr))).mean()  # mean over [B, S, L] = mean over [B, L]
    return nb_q + alpha * (kl - nb_q + nb_p - reg_like), a_q


def impute(a_q, x_mean):
    """llh_eval: softmax over the samples of the slot matrix, applied to the un-mixed x_mean [B, S, d]."""
    w = torch.softmax(a_q, 0)                                            # [S, B]
    return torch.einsum("ki,kij->ij", w, x_mean.permute(1, 0, 2))


def run(p, x, mask, mask_p, eps, alpha=1.0, pairing="reference"):
    """Whole forward + loss from parameters.  eps = [forward q, (forward p,) loss q, (loss p)] [B, S, L] each."""
    reg = mask_p is not None
    P = 2 if reg else 1
    mq, sq, zq = encode(p, x, mask, eps[0])
    q = (decode(p, zq), mq, sq)
    pp = None
    if reg:
        mp, sp, zp = encode(p, x, mask_p, eps[1])
        pp = (decode(p, zp), mp, sp)
    lo, a_q = loss(x, mask, mask_p, q, pp, eps[P:], alpha, pairing)
    return lo, a_q, q, pp


def closed_form_grads(x, mask, mask_p, q, p, eps2, alpha=1.0, pairing="reference"):
    """Closed-form d loss / d (mu, sc, v) [B,S,d] and d loss / d (mean, scale) [B,L] per pass: what vpc_miw_loss writes
    (activated heads, raw = 0)."""
    reg = p is not None
    passes = [q, p] if reg else [q]
    B, S, d = q[0][0].shape
    x = x.double()
    out = []
    for k, (dec, mean, scale) in enumerate(passes):
        m = (mask if k == 0 else mask_p).double()
        a = slot_matrix(x, m, dec, mean, scale, eps2[k], pairing)
        w = torch.softmax(a, 0)                                          # [S, B]
        coef = (-(1 - alpha) if k == 0 else -alpha) / B if reg else -1.0 / B
        gslot = coef * w                                                 # d loss / d a[i, j]
        gpo = gslot.reshape(B, S) if pairing == "reference" else gslot.permute(1, 0)  # on (row, sample)
        glw = gslot.permute(1, 0)                                        # [B, S]
        glp = gpo[:, :, None] * m[:, None, :]
        if k == 0 and reg:
            glp = glp - alpha / (B * S) * (mask.double() * (1 - mask_p.double()))[:, None, :]
        mu, sc, v = dec
        y = (x[:, None, :] - mu) / sc
        t = y * y / v
        u = 1 + t
        gmu = glp * (v + 1) * y / (v * sc * u)
        gsc = glp * (-1 / sc + (v + 1) * t / (sc * u))
        gv = glp * (0.5 * torch.digamma((v + 1) / 2) - 0.5 * torch.digamma(v / 2) - 0.5 / v - 0.5 * torch.log(u)
                    + (v + 1) * t / (2 * v * u))
        e = eps2[k].double()
        z2 = mean[:, None, :] + scale[:, None, :] * e
        gm = (glw[:, :, None] * -z2).sum(1)
        gs = (glw[:, :, None] * (1 / scale[:, None, :] - z2 * e)).sum(1)
        if reg:
            mq, sq, mp_, sp = q[1], q[2], p[1], p[2]
            c = alpha / (B * mean.shape[1])
            if k == 0:
                gm = gm + c * (mq - mp_) / sp ** 2
                gs = gs + c * (sq / sp ** 2 - 1 / sq)
            else:
                gm = gm - c * (mq - mp_) / sp ** 2
                gs = gs + c * (1 / sp - (sq ** 2 + (mq - mp_) ** 2) / sp ** 3)
        out.append((gmu, gsc, gv, gm, gs))
    return out
