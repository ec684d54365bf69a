"""Float64 restatement of the flow path (reference src/models/VAE.py: VAEFlow :1860-1996, REG_VAEFlow :1999-2124, Flow
:1816-1854, PiecewiseLinearCDF :1781-1813, unconstrained_linear_spline / linear_spline :1680-1774) with closed-form
gradients (`step`), and the same mathematics in torch float64 for autograd (`torch_step`).

The flow is restated per pass of B rows: m = [|eps| <= 1]; every layer reads the context c[b, i, j] = t[b, 10 i + j] *
m[b, j] (the reference's in-place multiply); layer 1's input is eps * m; a pass with no inside draw is the identity.

For the kernel-by-kernel parity tests (tests/test_flow_kernels_gpu.py) flow_fwd / flow_bwd return and take the per-element
discrete decisions (the bin of layers 2 / 3, each layer's clamp gate), flow_flags / alternative name and switch the ones
that are a tie in fp32, _torch_flow runs in fp32 on given decisions, and loss_terms restates vpc_flow_loss entry by entry.
"""
import numpy as np
import torch

L = 10
HL = 0.5 * np.log(2 * np.pi)
LOGVAR = -8.0
ENC = [("seq_encoder.0", "elu"), ("seq_encoder.2", "elu"), ("seq_encoder.4", None)]
DEC = [("seq_decoder.0", "elu"), ("seq_decoder.2", "elu"), ("seq_decoder.4", "elu"), ("seq_decoder.6", "elu"),
       ("decoder_mean.0", "sigmoid")]
TRAINABLE = [f"{n}.{w}" for n, _ in ENC + DEC for w in ("weight", "bias")]


def _act(a, kind):
    if kind == "elu":
        return np.where(a > 0, a, np.expm1(np.minimum(a, 0)))
    if kind == "sigmoid":
        return 1 / (1 + np.exp(-a))
    return a


def _act_d(a, y, kind):
    if kind == "elu":
        return np.where(a > 0, 1.0, np.exp(np.minimum(a, 0)))
    if kind == "sigmoid":
        return y * (1 - y)
    return np.ones_like(a)


def mlp(P, layers, x):
    cache = [x]
    pre = []
    for name, kind in layers:
        a = cache[-1] @ P[name + ".weight"].T + P[name + ".bias"]
        pre.append(a)
        cache.append(_act(a, kind))
    return cache, pre


def mlp_bwd(P, layers, cache, pre, dy, grads):
    """dy: gradient w.r.t. the last layer's OUTPUT; returns the gradient w.r.t. the input."""
    g = dy
    for i in range(len(layers) - 1, -1, -1):
        name, kind = layers[i]
        g = g * _act_d(pre[i], cache[i + 1], kind)
        grads[name + ".weight"] = grads.get(name + ".weight", 0) + g.T @ cache[i]
        grads[name + ".bias"] = grads.get(name + ".bias", 0) + g.sum(0)
        g = g @ P[name + ".weight"]
    return g


def bin_of(x):
    """Spline bin of inputs x in [-1, 1], decided in float32 as the reference computes bin_pos (VAE.py:1761-1764): a
    float64 bin position a few ulp below an integer would otherwise select the neighbouring bin."""
    bp = (np.asarray(x, np.float32) + np.float32(1)) / np.float32(2) * np.float32(L)
    return np.minimum(np.floor(bp).astype(np.int64), L - 1)


FLAG_BIN = 1e-5    # a layer-2 / 3 bin position this close to an integer (about ten fp32 ulp at 10) is a tie in fp32
FLAG_GATE = 1e-6   # a layer's o this close to 0 or 1 (ten accumulated ulp at 1) likewise


def flow_fwd(t, eps, decisions=None):
    """t [B, 100], eps [B, 10] of ONE pass -> z, z_log_prob, cache.

    decisions = dict(bins int [3, B, 10], gates bool [3, B, 10]): the per-element discrete decisions, taken as given
    (bins[1:], gates) or, with None, taken here; cache[4] returns them.  bins[0] is never free: layer 1's bin is
    bin_of(eps * m), exact fp32 arithmetic on the given draw.  The gate 0 <= o <= 1 only enters the backward."""
    B = eps.shape[0]
    lp = -eps ** 2 / 2 - HL
    if not np.any(np.abs(eps) <= 1):
        return eps.copy(), lp, None
    m = (np.abs(eps) <= 1).astype(np.float64)
    c = t.reshape(B, L, L) * m[:, None, :]
    e = np.exp(c - c.max(-1, keepdims=True))
    pdf = e / e.sum(-1, keepdims=True)
    cdf = np.cumsum(pdf, -1) - pdf
    x = eps * m
    steps, ld = [], 0
    bins, gates = np.zeros((3, B, L), np.int64), np.zeros((3, B, L), bool)
    bi, li = np.arange(B)[:, None], np.arange(L)[None, :]
    for l in range(3):
        bp = (x + 1) / 2 * L
        b = bin_of(x) if decisions is None or l == 0 else np.asarray(decisions["bins"][l])
        al = bp - b
        pb, cb = pdf[bi, li, b], cdf[bi, li, b]
        o = cb + al * pb
        steps.append((b, al, pb, o))
        bins[l] = b
        gates[l] = (o >= 0) & (o <= 1) if decisions is None else decisions["gates"][l]
        x = np.clip(o, 0, 1) * 2 - 1
        ld = ld + np.log(pb) + np.log(L)
    return x, lp - ld, (m, pdf, cdf, steps, dict(bins=bins, gates=gates))


def flow_bwd(cache, dz, dzlp):
    """d / d t [B, 100] given d / d z and d / d z_log_prob (cache of flow_fwd, its decisions included)."""
    B = dz.shape[0]
    if cache is None:
        return np.zeros((B, L * L))
    m, pdf, cdf, steps, dec = cache
    bi, li = np.arange(B)[:, None], np.arange(L)[None, :]
    du = np.zeros((B, L, L))
    gout = dz.copy()
    glad = -dzlp
    for l in (2, 1, 0):
        b, al, pb, o = steps[l]
        go = np.where(dec["gates"][l], 2 * gout, 0.0)
        cb = cdf[bi, li, b]
        onehot = (np.arange(L)[None, None, :] == b[..., None]).astype(np.float64)
        below = (np.arange(L)[None, None, :] < b[..., None]).astype(np.float64)
        du += go[..., None] * (pdf * (below - cb[..., None]) + (al * pb)[..., None] * (onehot - pdf))
        du += glad[..., None] * (onehot - pdf)
        gout = go * L * 0.5 * pb
    return (du * m[:, None, :]).reshape(B, L * L)


def flow_flags(cache):
    """Which decisions of a flow_fwd cache fp32 may take the other way: dict(bins bool [3, B, 10] (layer 1 never),
    gates bool [3, B, 10]), from the float64 bin positions (FLAG_BIN) and o (FLAG_GATE)."""
    steps = cache[3]
    fb, fg = np.zeros((3,) + steps[0][0].shape, bool), np.zeros((3,) + steps[0][0].shape, bool)
    for l, (b, al, pb, o) in enumerate(steps):
        bp = b + al
        if l:
            fb[l] = np.abs(bp - np.rint(bp)) < FLAG_BIN
        fg[l] = np.minimum(np.abs(o), np.abs(o - 1)) < FLAG_GATE
    return dict(bins=fb, gates=fg)


def flagged(flags):
    """[B, 10]: the elements with any flagged decision."""
    return flags["bins"].any(0) | flags["gates"].any(0)


N_ALTERNATIVES = 32  # two bins and three gates


def alternative(cache, flags, c):
    """The decisions of `cache` with the flagged ones among (bin 2, bin 3, gate 1, gate 2, gate 3) switched where bit
    0 .. 4 of c is set: a flagged bin to the other bin at the knot (the same one at the ends 0 and 10), a flagged gate to
    its negation.  c = 0 is the cache's own decisions."""
    steps, dec = cache[3], cache[4]
    bins, gates = dec["bins"].copy(), dec["gates"].copy()
    for s, l in enumerate((1, 2)):
        if c >> s & 1:
            k = np.rint(steps[l][0] + steps[l][1]).astype(np.int64)  # the knot: the candidates are bins k - 1 and k
            other = np.clip(2 * k - 1 - bins[l], 0, L - 1)
            bins[l] = np.where(flags["bins"][l], other, bins[l])
    for s, l in enumerate((0, 1, 2)):
        if c >> (2 + s) & 1:
            gates[l] = np.where(flags["gates"][l], ~gates[l], gates[l])
    return dict(bins=bins, gates=gates)


def nll(x, xr, w):
    """-Normal(xr * w, exp(-8 w / 2)).log_prob(x * w) elementwise, w in {0, 1}."""
    var = np.exp(LOGVAR * w)
    return (x * w - xr * w) ** 2 / (2 * var) + LOGVAR * w / 2 + HL


def step(P, x, mask, mask_p, eps, alpha=1.0, beta=1.0, stage="train"):
    """One forward + closed-form backward.  mask_p None: VAEFlow, else REG_VAEFlow.  eps [P, B, 10].
    Returns dict(loss = train_loss, print_loss, llh (RE_q / B, RE_q_imputed / B), fwd, grads over TRAINABLE)."""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    x = np.asarray(x, np.float64)
    m = np.asarray(mask, np.float64)
    reg = mask_p is not None
    B = x.shape[0]
    masks = [m] + ([np.asarray(mask_p, np.float64)] if reg else [])
    passes = []
    for k, mk in enumerate(masks):
        ecache, epre = mlp(P, ENC, np.concatenate([x * mk, mk], 1))
        z, zlp, fc = flow_fwd(ecache[-1], np.asarray(eps[k], np.float64))
        dcache, dpre = mlp(P, DEC, z)
        passes.append(dict(ec=ecache, ep=epre, z=z, zlp=zlp, fc=fc, dc=dcache, dp=dpre, xm=dcache[-1]))
    q = passes[0]
    kl = lambda p_: np.sum(p_["zlp"] + p_["z"] ** 2 / 2 + HL)
    RE_q = np.sum(nll(x, q["xm"], m))
    RE_imp = np.sum(nll(x, q["xm"], 1 - m))
    KL_q = kl(q)
    loss_q = RE_q + beta * KL_q
    train = reg and stage == "train"
    if train:
        p = passes[1]
        mp = masks[1]
        RE_p, KL_p = np.sum(nll(x, p["xm"], mp)), kl(p)
        KL_reg = np.sum(np.abs(q["zlp"] - p["zlp"]))
        NLL_r = np.sum(nll(x, q["xm"], m * (1 - mp)))
        loss = loss_q + alpha * (KL_reg - loss_q + RE_p + beta * KL_p + NLL_r)
        c_q, c_p = 1 - alpha, alpha
    else:
        loss = loss_q
        c_q, c_p = 1.0, 0.0
    s = 1.0 / B
    inv_var = np.exp(-LOGVAR)
    grads = {}
    gx_q = (c_q * m + (alpha * m * (1 - masks[1]) if train else 0)) * (q["xm"] - x) * inv_var * s
    sgn = np.sign(q["zlp"] - passes[1]["zlp"]) if train else 0
    seeds = [(gx_q, c_q * beta * q["z"] * s, (c_q * beta + alpha * sgn) * s)]
    if train:
        p = passes[1]
        seeds.append((c_p * masks[1] * (p["xm"] - x) * inv_var * s, c_p * beta * p["z"] * s,
                      (c_p * beta - alpha * sgn) * s))
    for pp, (gx, gz, gzlp) in zip(passes, seeds):
        dz = mlp_bwd(P, DEC, pp["dc"], pp["dp"], gx, grads) + gz
        dt = flow_bwd(pp["fc"], dz, np.broadcast_to(gzlp, dz.shape))
        mlp_bwd(P, ENC, pp["ec"], pp["ep"], dt, grads)
    for k in TRAINABLE:
        grads.setdefault(k, np.zeros_like(P[k]))
    train_loss = loss / B
    fwd = {"z_q": q["z"], "z_log_prob_q": q["zlp"], "x_mean_q": q["xm"]}
    if reg:
        fwd.update(z_p=passes[1]["z"], z_log_prob_p=passes[1]["zlp"], x_mean_p=passes[1]["xm"])
    return dict(loss=train_loss, print_loss=loss if not reg else train_loss, llh=(RE_q / B, RE_imp / B), fwd=fwd,
                grads=grads)


# ------------------------------------------------------------------------------------------------ torch autograd
def _torch_flow(t, eps, decisions=None):
    """In the dtype of t.  decisions (flow_fwd's): the bins of layers 2 / 3 and every clamp gate are taken from them,
    so that an fp32 run differs from the float64 one by rounding only (the gate decides where autograd passes)."""
    B = eps.shape[0]
    lp = -eps ** 2 / 2 - HL
    if not bool(torch.any(eps.abs() <= 1)):
        return eps, lp
    m = (eps.abs() <= 1).to(t.dtype)
    pdf = torch.softmax(t.reshape(B, L, L) * m[:, None, :], -1)
    cdf = torch.nn.functional.pad(torch.cumsum(pdf, -1)[..., :-1], (1, 0))
    x = eps * m
    ld = 0
    for l in range(3):
        bp = (x + 1) / 2 * L
        if decisions is None or l == 0:
            b = torch.from_numpy(bin_of(x.detach().numpy()))
        else:
            b = torch.from_numpy(np.asarray(decisions["bins"][l]))
        al = bp - b.to(t.dtype)
        pb = pdf.gather(-1, b[..., None])[..., 0]
        o = cdf.gather(-1, b[..., None])[..., 0] + al * pb
        oc = torch.clamp(o, 0, 1)
        if decisions is not None:  # the clamped value, the gradient of o where the gate is open
            g = torch.from_numpy(np.asarray(decisions["gates"][l]))
            oc = torch.where(g, o + (oc - o).detach(), oc.detach())
        x = oc * 2 - 1
        ld = ld + torch.log(pb) + np.log(L)
    return x, lp - ld


def loss_terms(x, m, mp, xm, z, zlp, alpha, beta, stage="train", gated=0, gscale=1.0):
    """vpc_flow_loss restated in torch, in the dtype of x (float64: the oracle; fp32: the rounding yardstick).
    xm, z, zlp: (q, p) pairs; mp None: VAEFlow (the p entries are not read).  Returns dict(out8 [8] = loss (unscaled),
    RE_q, RE_p, KL_q, KL_p, KL_reg, NLL of x * mask * ~mask_p, RE_q on ~mask; abs8 [8] = the sum of the absolute values
    of each entry's terms; grads = (gxm_q, gxm_p, gz_q, gz_p, gzlp_q, gzlp_p) of gscale * loss in closed form, the xm
    pair times xm (1 - xm) when gated (the gradient of a Sigmoid's pre-activation), sign(0) = 0 at a z_log_prob tie)."""
    reg = mp is not None
    pp = reg and stage == "train"
    sc = torch.exp(torch.tensor(LOGVAR / 2, dtype=x.dtype))
    var, logs = sc * sc, torch.log(sc)

    def nll_(xr, w):
        return torch.where(w == 0, torch.full_like(x, HL), (x - xr) ** 2 / (2 * var) + logs + HL)

    kl_ = lambda k: zlp[k] - (-(z[k] * z[k]) / 2 - HL)
    zero = torch.zeros_like(x)
    wr = m * (1 - mp) if reg else zero
    terms = [nll_(xm[0], m), nll_(xm[1], mp) if pp else zero, kl_(0), kl_(1) if pp else torch.zeros_like(z[0]),
             (zlp[0] - zlp[1]).abs() if pp else torch.zeros_like(z[0]), nll_(xm[0], wr) if reg else zero,
             nll_(xm[0], 1 - m)]
    s = [u.double().sum() for u in terms]
    a = [u.double().abs().sum() for u in terms]
    loss_q, abs_q = s[0] + beta * s[2], a[0] + beta * a[2]
    loss, abs_l = loss_q, abs_q
    if pp:
        loss = loss_q + alpha * (s[4] - loss_q + (s[1] + beta * s[3]) + s[5])
        abs_l = abs_q + alpha * (a[4] + abs_q + a[1] + beta * a[3] + a[5])
    c_q, c_r, c_p = (1 - alpha, alpha, alpha) if pp else (1.0, 0.0, 0.0)
    gs = gscale / var
    gq = (c_q * m + c_r * wr) * (xm[0] - x) * gs
    gp = c_p * mp * (xm[1] - x) * gs if pp else zero
    if gated:
        gq = gq * (xm[0] * (1 - xm[0]))
        if pp:
            gp = gp * (xm[1] * (1 - xm[1]))
    sgn = torch.sign(zlp[0] - zlp[1]) if pp else torch.zeros_like(z[0])
    grads = (gq, gp, gscale * c_q * beta * z[0], gscale * c_p * beta * z[1] if pp else torch.zeros_like(z[0]),
             gscale * (c_q * beta + alpha * sgn), gscale * (c_p * beta - alpha * sgn) if pp else torch.zeros_like(z[0]))
    return dict(out8=torch.stack([loss] + s), abs8=torch.stack([abs_l] + a), grads=grads)


def torch_step(P, x, mask, mask_p, eps, alpha=1.0, beta=1.0, stage="train"):
    """The same step with torch float64 autograd -> (train_loss, grads over TRAINABLE)."""
    T = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=k in TRAINABLE) for k, v in P.items()}
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    m = torch.as_tensor(np.asarray(mask), dtype=torch.float64)
    reg = mask_p is not None
    masks = [m] + ([torch.as_tensor(np.asarray(mask_p), dtype=torch.float64)] if reg else [])
    actf = {"elu": torch.nn.functional.elu, "sigmoid": torch.sigmoid, None: lambda a: a}

    def run(layers, h):
        for name, kind in layers:
            h = actf[kind](h @ T[name + ".weight"].T + T[name + ".bias"])
        return h

    outs = []
    for k, mk in enumerate(masks):
        t = run(ENC, torch.cat([x * mk, mk], 1))
        z, zlp = _torch_flow(t, torch.as_tensor(np.asarray(eps[k]), dtype=torch.float64))
        outs.append((z, zlp, run(DEC, z)))

    def nll_t(xr, w):
        var = torch.exp(LOGVAR * w)
        return (x * w - xr * w) ** 2 / (2 * var) + LOGVAR * w / 2 + HL

    kl = lambda o: torch.sum(o[1] + o[0] ** 2 / 2 + HL)
    q = outs[0]
    loss_q = nll_t(q[2], m).sum() + beta * kl(q)
    if reg and stage == "train":
        p = outs[1]
        loss_p = nll_t(p[2], masks[1]).sum() + beta * kl(p)
        loss = loss_q + alpha * (torch.sum(torch.abs(q[1] - p[1])) - loss_q + loss_p +
                                 nll_t(q[2], m * (1 - masks[1])).sum())
    else:
        loss = loss_q
    tl = loss / x.shape[0]
    tl.backward()
    return tl.item(), {k: T[k].grad.numpy() for k in TRAINABLE}


def init_params(d, H, seed=0):
    """Reference-shaped parameters (nn.Linear's default init scale), float32."""
    g = np.random.default_rng(seed)
    shapes = {"seq_encoder.0": (H, 2 * d), "seq_encoder.2": (H, H), "seq_encoder.4": (L * L, H),
              "seq_decoder.0": (H, L), "seq_decoder.2": (H, H), "seq_decoder.4": (H, H), "seq_decoder.6": (H, H),
              "decoder_mean.0": (d, H)}
    P = {}
    for n, (o, i) in shapes.items():
        bound = 1 / np.sqrt(i)
        P[n + ".weight"] = g.uniform(-bound, bound, (o, i)).astype(np.float32)
        P[n + ".bias"] = g.uniform(-bound, bound, (o,)).astype(np.float32)
    return P
