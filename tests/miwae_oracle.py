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


KINK_BAND = 1e-5  # of a layer's max |pre-activation|: inside it fp32 and float64 may gate a ReLU unit differently


def new_gate_stats():
    return dict(units=0, in_band=0, taken_from_device=0, mismatch_outside=0)


def _mlp(p, pre, h, gate=None):
    """gate = (device gates {layer index: bool tensor}, or None; stats dict): the two hidden layers count their units
    inside the kink band into stats and, given the device's gates, take those inside the band and their own pre > 0
    everywhere else (a device gate that differs outside the band is counted as a mismatch, never taken)."""
    for i in (0, 2):
        a = F.linear(h, p[f"{pre}.{i}.weight"], p[f"{pre}.{i}.bias"])
        if gate is None:
            h = F.relu(a)
            continue
        dev, stats = gate
        g = a.detach() > 0
        inb = a.detach().abs() <= KINK_BAND * a.detach().abs().max()
        stats["units"] += a.numel()
        stats["in_band"] += int(inb.sum())
        if dev is not None:
            dg = dev[i].reshape(a.shape)
            stats["taken_from_device"] += int((inb & (dg != g)).sum())
            stats["mismatch_outside"] += int((~inb & (dg != g)).sum())
            g = torch.where(inb, dg, g)
        h = a * g
    return F.linear(h, p[f"{pre}.4.weight"], p[f"{pre}.4.bias"])


def encode(p, x, mask, eps, gate=None):
    """-> mean, scale [B, L], z [B, S, L] (eps [B, S, L])."""
    mean, raw = _mlp(p, "seq_encoder", x.double() * mask.double(), gate).chunk(2, dim=1)
    scale = F.softplus(raw)
    return mean, scale, mean[:, None, :] + scale[:, None, :] * eps.double()


def decode(p, z, gate=None):
    mu, sc, v = _mlp(p, "seq_decoder", z, gate).chunk(3, dim=-1)
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


def run(p, x, mask, mask_p, eps, alpha=1.0, pairing="reference", gates=None, stats=None):
    """Whole forward + loss from parameters.  eps = [forward q, (forward p,) loss q, (loss p)] [B, S, L] each.
    stats (new_gate_stats()): count the hidden units inside the kink band; gates {"enc_q" | "dec_q" | "enc_p" | "dec_p":
    {0: bool [rows, H], 2: ..}}: the gates a device step took, used inside the band only (_mlp)."""
    reg = mask_p is not None
    P = 2 if reg else 1
    gt = lambda k: None if stats is None else (None if gates is None else gates[k], stats)
    mq, sq, zq = encode(p, x, mask, eps[0], gt("enc_q"))
    q = (decode(p, zq, gt("dec_q")), mq, sq)
    pp = None
    if reg:
        mp, sp, zp = encode(p, x, mask_p, eps[1], gt("enc_p"))
        pp = (decode(p, zp, gt("dec_p")), mp, sp)
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


def terms(x, mask, mask_p, q, p, eps2, alpha=1.0, pairing="reference"):
    """The eight doubles vpc_miw_loss writes: [loss, nb_q, nb_p, kl, reg_like, sum(lp_q * (1 - mask)) / (B * 5000)
    (VAE.py:3099, a literal 5000), sum_j logsumexp_i a_q, sum_j logsumexp_i a_p]; the p / regulariser entries are 0 for
    MIWAE."""
    B = x.shape[0]
    z = torch.zeros((), dtype=torch.float64)
    a_q = slot_matrix(x, mask, q[0], q[1], q[2], eps2[0], pairing)
    lse_q = torch.logsumexp(a_q, 0).sum()
    lp_q = student_lp(x.double()[:, None, :], *q[0])
    third = (lp_q * (1 - mask.double())[:, None, :]).sum() / (B * 5000)
    if p is None:
        return torch.stack([-lse_q / B, -lse_q / B, z, z, z, third, lse_q, z])
    lse_p = torch.logsumexp(slot_matrix(x, mask_p, p[0], p[1], p[2], eps2[1], pairing), 0).sum()
    reg_like = (lp_q * mask.double()[:, None, :] * (1 - mask_p.double())[:, None, :]).sum(-1).mean()
    vr = (q[2] / p[2]) ** 2
    kl = (0.5 * (vr + ((q[1] - p[1]) / p[2]) ** 2 - 1 - torch.log(vr))).mean()
    nb_q, nb_p = -lse_q / B, -lse_p / B
    return torch.stack([nb_q + alpha * (kl - nb_q + nb_p - reg_like), nb_q, nb_p, kl, reg_like, third, lse_q, lse_p])


# ---- the elementwise kernels (miw_sample, miw_sample_bwd, miw_heads, miw_heads_bwd), in the dtype of their inputs: the
# GPU tests evaluate them in float64 (the reference) and in float32 (the error a correct fp32 evaluation has)
def softplus_d(v):
    """torch's Softplus backward (threshold 20): identity above the threshold, exp(v) / (exp(v) + 1) below."""
    z = torch.exp(torch.clamp(v, max=20.0))
    return torch.where(v > 20, torch.ones_like(v), z / (z + 1))


def sample(heads, eps, S):
    """heads [R, mean L | raw scale L], eps [R, S, L] or None (z = mean) -> z [R, S, L], hact [R, mean L | scale L]."""
    L = heads.shape[1] // 2
    mean, sc = heads[:, :L], F.softplus(heads[:, L:])
    z = mean[:, None, :].expand(-1, S, -1)
    if eps is not None:
        z = z + eps * sc[:, None, :]
    return z, torch.cat([mean, sc], 1)


def sample_bwd(dz, eps, heads, g_hact, S):
    """d / d heads of sample(): dz [R, S, L] and g_hact [R, 2L] are the gradients of its two outputs, either may be None."""
    L = heads.shape[1] // 2
    gm, gs = torch.zeros_like(heads[:, :L]), torch.zeros_like(heads[:, L:])
    if g_hact is not None:
        gm, gs = gm + g_hact[:, :L], gs + g_hact[:, L:]
    if dz is not None:
        gm = gm + dz.sum(1)
        if eps is not None:
            gs = gs + (dz * eps).sum(1)
    return torch.cat([gm, gs * softplus_d(heads[:, L:])], 1)


def heads_act(y):
    """raw decoder heads [M, 3d] -> [sigmoid | softplus + 0.001 | softplus + 3] (VAE.py:3072-3076)."""
    mu, sc, v = y.chunk(3, dim=1)
    return torch.cat([torch.sigmoid(mu), F.softplus(sc) + 0.001, F.softplus(v) + 3], 1)


def heads_bwd(y, g):
    """d / d raw heads of heads_act().  The sigmoid's derivative is z / (1 + z)^2 with z = exp(-|mu|), the kernel's form:
    s (1 - s) loses the digits of 1 - s once s is within rounding of 1."""
    mu, sc, v = y.chunk(3, dim=1)
    z = torch.exp(-mu.abs())
    return g * torch.cat([z / ((1 + z) * (1 + z)), softplus_d(sc), softplus_d(v)], 1)
