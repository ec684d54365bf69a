"""Float64 restatement of the flow models' config 5 reward (reference src/experiment_main/evaluate.py:
R_lindley_chain_ratio_version :637-665, chaini_I_ratio_version :669-684, chaini_II_ratio_version :688-708), built on
tests/flow_oracle.py (`mlp`, `flow_fwd`): the literal four-encoder-calls-per-(candidate, sample) loop on the rows
loc(u) = {n : mask[n, u] == 0}, with the carry-over of the imputed target between samples (temp_x is cloned once per
candidate, :653-658), the per-call torch.any(inside) of the flow (flow_fwd takes it over the rows it is given) and an
empty loc (the column stays -1e4).

Draws are injected as the dense tensor eps [d-1, M, 4, n, 10] (call order Ia, Ib, IIa, IIb; rows outside loc(u) unused).
"""
import numpy as np

import flow_oracle as F

L = F.L


def encoder_zlp(P, x, mask, eps):
    """z_log_prob [rows, 10] of ONE vae.encoder(x, mask) call (VAE.py:1924-1931) and its flow cache."""
    t = F.mlp(P, F.ENC, np.concatenate([x * mask, mask], 1))[0][-1]
    _, zlp, cache = F.flow_fwd(t, eps)
    return zlp, cache


def _edge_distance(cache, rows):
    """Per row: the smallest distance of a layer-2 / layer-3 bin position to an integer (layer 1's input is the draw
    itself and cannot move)."""
    if cache is None:
        return np.full(rows, np.inf)
    steps = cache[3]
    dist = np.full(rows, np.inf)
    for b, al, _, _ in steps[1:]:
        bp = b + al
        dist = np.minimum(dist, np.abs(bp - np.round(bp)).min(1))
    return dist


def reward_matrix(P, x, mask, im, eps, candidates=None):
    """-> dict(R [n, d-1], edge [n, d-1] smallest layer-2/3 bin-position distance to an integer over the evaluations an
    entry sums (inf where none), S = the largest |z_log_prob| met).  candidates: only these columns (timing a subset)."""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    x = np.asarray(x, np.float64)
    mask = (np.asarray(mask) != 0).astype(np.float64)
    im = np.asarray(im, np.float64)
    eps = np.asarray(eps, np.float64)
    n, d = x.shape
    M = im.shape[0]
    R = np.full((n, d - 1), -1e4)
    edge = np.full((n, d - 1), np.inf)
    S = 0.0
    for u in (range(d - 1) if candidates is None else candidates):
        loc = np.where(mask[:, u] == 0)[0]
        if loc.size == 0:
            continue
        tx = x.copy()
        acc = np.zeros(loc.size)
        ed = np.full(loc.size, np.inf)
        for m in range(M):
            tx[loc, u] = im[m, loc, u]
            lps = []
            for call in range(4):
                if call == 2:
                    tx[loc, -1] = im[m, loc, -1]
                tm = mask[loc].copy()
                if call >= 2:
                    tm[:, -1] = 1
                if call & 1:
                    tm[:, u] = 1
                zlp, cache = encoder_zlp(P, tx[loc], tm, eps[u, m, call][loc])
                ed = np.minimum(ed, _edge_distance(cache, loc.size))
                S = max(S, float(np.abs(zlp).max()))
                lps.append(zlp)
            acc += np.abs(lps[0] - lps[1]).sum(1)
            acc -= np.abs(lps[2] - lps[3]).sum(1)
        R[loc, u] = acc / M
        edge[loc, u] = ed
    return dict(R=R, edge=edge, S=S)


# The check every comparison against this oracle or the reference uses (derived in the issue from what the flow forward
# is already held to, 2e-5 of max on z_log_prob): one entry is a mean over m of 2 chains x 10 latents x a difference of 2
# values, so |R - R_ref| <= 2 * 10 * 2 * 2e-5 * S.  An entry may be left out only when a layer-2/3 bin position lies within
# `delta` of an integer (fp32 GEMM rounding can move it across the edge, and logabsdet jumps there); at most 5 % may.
TOL_PER_S = 8e-4
MAX_FLAGGED = 0.05


def compare(R, ref, edge, S, delta):
    """-> (largest error over the unflagged unobserved entries, bound, flagged share).  Asserts nothing."""
    R, ref = np.asarray(R, np.float64), np.asarray(ref, np.float64)
    unobs = ref != -1e4
    flagged = unobs & (edge <= delta)
    keep = unobs & ~flagged
    err = float(np.abs(R - ref)[keep].max()) if keep.any() else 0.0
    return err, TOL_PER_S * S, float(flagged.sum()) / max(1, int(unobs.sum()))
