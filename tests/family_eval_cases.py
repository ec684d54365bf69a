"""Shared by tests/test_ensemble_eval_families_{cpu,gpu}.py: models of the mask-augmented and point-net families, their data and
the float64 closed form of their evaluation.

The closed form of one batch is, for the mask family, oracle.vae_oracle.closed_form_pass on the encoder input [x*m | m]
(VAE.py:545-548), and for the point-net family oracle.eddi_oracle.front_closed_form (VAE.py:719-733) followed by the trunk
pnp_encoder2 and the decoder - closed_form_pass again, on the aggregate.  Then the reference's per-batch numbers
(VAE.py:570-580, 757-767, 935-950, 1053-1060; evaluate.py:229-234), the mean over the batches of a pass and the mean over the
passes (evaluate.py:238-245), exactly as oracle_eval of tests/test_ensemble_eval_gpu.py states them for the plain family."""
import numpy as np
import torch

import vpc_amd as vpc
from conftest import load_golden
from oracle import eddi_oracle as EO
from oracle import vae_oracle as O

L = 10
TP = {"batch_size": 64, "patience": 100}
GOLDEN = "family_eval_d14.npz"
GOLDEN_TAGS = {"mask_reg": ("mask", "reg"), "mask_van": ("mask", "van"), "eddi_reg": ("eddi", "reg"), "eddi_van": ("eddi", "van")}
_TRUNK = {f"seq_encoder.{i}.{w}": f"pnp_encoder2.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")}


def build(family, kind, d, K=10, reg_type="kl_reg", params=None, latent=L):
    """A CPU model of `family` ("mask" / "eddi"), kind "reg" / "van"; params: state_dict entries to load."""
    if family == "mask":
        m = vpc.Reg_VAE_mask(d, 500, 10, latent, TP, "e", reg_type) if kind == "reg" else vpc.vanilla_VAE_mask(d, 500, 10, latent, TP, "e")
    else:
        m = vpc.Reg_EDDI(d, 500, K, latent, TP, "e", reg_type) if kind == "reg" else vpc.vanilla_EDDI(d, 500, K, latent, TP, "e")
    if params is not None:
        sd = m.state_dict()
        for k, v in params.items():
            sd[k] = torch.as_tensor(v).clone()
        m.load_state_dict(sd)
    return m


def params_of(m):
    """The trainable tensors of a model by their state_dict names, on the CPU."""
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if "prior" not in k}


def copy_of(family, m, device):
    """A fresh, unstacked model with m's current parameters."""
    kind = "reg" if getattr(m, "reg_type", None) is not None else "van"
    return build(family, kind, m.obs_dim, getattr(m, "emb_dim", 10), getattr(m, "reg_type", None) or "kl_reg",
                 params_of(m)).to(device)


def data(shape, seed, keep=0.7):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g), torch.rand(*shape, generator=g) < keep


def golden_case(tag):
    """-> (family, kind, params, x, mask, eps_q, the reference's (loss, RE_q / B, RE_q_imputed / B)) of one golden model."""
    g = load_golden(GOLDEN)
    pre = tag + ".param."
    params = {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(pre) and "prior" not in k}
    return GOLDEN_TAGS[tag] + (params, g[tag + ".x"], g[tag + ".mask"], g[tag + ".eps_q"], np.asarray(g[tag + ".eval_llh"], np.float64))


def closed_form_batch(family, P, xb, mb, eps, latent=L):
    """float64 forward of one batch -> vae_oracle.PassCache (xhat, mean, logvar are what the evaluation reads)."""
    ones = np.ones_like
    if family == "mask":
        xin = np.concatenate([xb * mb, mb], 1)
        return O.closed_form_pass(P, xin, ones(xin), eps, latent)
    agg = EO.front_closed_form(xb, mb, P["type_pars1"], P["type_bias1"], P["pnp_encoder1.0.weight"], P["pnp_encoder1.0.bias"])
    Q = {k: v for k, v in P.items() if k.startswith("seq_decoder")}
    Q.update({k: P[src] for k, src in _TRUNK.items()})
    return O.closed_form_pass(Q, agg, ones(agg), eps, latent)


def oracle_eval(family, params, x, mask, eps, batches, bw=1.0, latent=L):
    """batches: M lists of (row_lo, row_hi) into x / mask; draw rows count on from batch to batch, pass to pass (eps row r).
    -> ((rmse, elbo, negll, negll_imp) in float64, whether every batch has an unobserved entry)."""
    P = O._np(params)
    x, mk, eps = np.asarray(x, np.float64), np.asarray(mask, np.float64), np.asarray(eps, np.float64)
    s2, every, r, passes = np.exp(O.X_LOGVAR), True, 0, []
    for ranges in batches:
        rows = []
        for lo, hi in ranges:
            xb, mb, n = x[lo:hi], mk[lo:hi], hi - lo
            c = closed_form_batch(family, P, xb, mb, eps[r:r + n], latent)
            r += n
            t = 0.5 * O.X_LOGVAR + (xb - c.xhat) ** 2 / (2 * s2)
            const = O.HALF_LOG_2PI * xb.size
            negll, negll_imp = (np.sum(mb * t) + const) / n, (np.sum((1 - mb) * t) + const) / n
            kl = np.sum(0.5 * (np.exp(c.logvar) + c.mean ** 2 - 1.0 - c.logvar))
            every = every and np.sum(1 - mb) > 0
            rows.append((np.sqrt(np.sum((1 - mb) * (c.xhat - xb) ** 2) / np.sum(1 - mb)), negll + bw * kl / n, negll, negll_imp))
        passes.append(np.mean(np.array(rows), 0))
    return np.mean(np.array(passes), 0), every


def batch_ranges(N, batch_size, M):
    """The layout evaluate(batch_size=...) walks, spelled as explicit ranges."""
    return [[(lo, min(lo + batch_size, N)) for lo in range(0, N, batch_size)]] * M


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))
