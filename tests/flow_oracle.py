"""Float64 restatement of the flow path (reference src/models/VAE.py: VAEFlow :1860-1996, REG_VAEFlow :1999-2124, Flow
:1816-1854, PiecewiseLinearCDF :1781-1813, unconstrained_linear_spline / linear_spline :1680-1774) with closed-form
gradients (`step`), and the same mathematics in torch float64 for autograd (`torch_step`).

The flow is restated per pass of B rows: m = [|eps| <= 1]; every layer reads the context c[b, i, j] = t[b, 10 i + j] *
m[b, j] (the reference's in-place multiply); layer 1's input is eps * m; a pass with no inside draw is the identity.
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


def flow_fwd(t, eps):
    """t [B, 100], eps [B, 10] of ONE pass -> z, z_log_prob, cache."""
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
    bi, li = np.arange(B)[:, None], np.arange(L)[None, :]
    for _ in range(3):
        bp = (x + 1) / 2 * L
        b = bin_of(x)
        al = bp - b
        pb, cb = pdf[bi, li, b], cdf[bi, li, b]
        o = cb + al * pb
        steps.append((b, al, pb, o))
        x = np.clip(o, 0, 1) * 2 - 1
        ld = ld + np.log(pb) + np.log(L)
    return x, lp - ld, (m, pdf, cdf, steps)


def flow_bwd(cache, dz, dzlp):
    """d / d t [B, 100] given d / d z and d / d z_log_prob (cache of flow_fwd)."""
    B = dz.shape[0]
    if cache is None:
        return np.zeros((B, L * L))
    m, pdf, cdf, steps = cache
    bi, li = np.arange(B)[:, None], np.arange(L)[None, :]
    du = np.zeros((B, L, L))
    gout = dz.copy()
    glad = -dzlp
    for b, al, pb, o in steps[::-1]:
        go = np.where((o >= 0) & (o <= 1), 2 * gout, 0.0)
        cb = cdf[bi, li, b]
        onehot = (np.arange(L)[None, None, :] == b[..., None]).astype(np.float64)
        below = (np.arange(L)[None, None, :] < b[..., None]).astype(np.float64)
        du += go[..., None] * (pdf * (below - cb[..., None]) + (al * pb)[..., None] * (onehot - pdf))
        du += glad[..., None] * (onehot - pdf)
        gout = go * L * 0.5 * pb
    return (du * m[:, None, :]).reshape(B, L * L)


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
def _torch_flow(t, eps):
    B = eps.shape[0]
    lp = -eps ** 2 / 2 - HL
    if not bool(torch.any(eps.abs() <= 1)):
        return eps, lp
    m = (eps.abs() <= 1).to(t.dtype)
    pdf = torch.softmax(t.reshape(B, L, L) * m[:, None, :], -1)
    cdf = torch.nn.functional.pad(torch.cumsum(pdf, -1)[..., :-1], (1, 0))
    x = eps * m
    ld = 0
    for _ in range(3):
        bp = (x + 1) / 2 * L
        b = torch.from_numpy(bin_of(x.detach().numpy()))
        al = bp - b.to(t.dtype)
        pb = pdf.gather(-1, b[..., None])[..., 0]
        o = cdf.gather(-1, b[..., None])[..., 0] + al * pb
        x = torch.clamp(o, 0, 1) * 2 - 1
        ld = ld + torch.log(pb) + np.log(L)
    return x, lp - ld


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
