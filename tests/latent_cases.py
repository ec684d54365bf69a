"""Latent widths of the dense VAE family: the case lists, seeded inputs and comparisons of test_latent_widths_cpu.py and
test_latent_widths_gpu.py.

The register-chained kernels take latent_dim 1 .. 15 (MAX_L in csrc/vpc_layout.h); every kernel body decides per lane, by
`4 * q + j < L` and `4 * q + j == L`, which columns of the 16-wide mean / logvar tiles are latent features, which one is the
constant 1 of the decoder's bias chain and which carry no gradient.  The rest of the suite runs at L = 10 (the bias column in
the middle of quad 2).  The widths here put that boundary everywhere else it can fall:

    L = 1    one live column, two head rows
    L = 3    the bias column is the last of quad 0
    L = 4, 8, 12   the bias column opens the next quad; every earlier quad is fully valid
    L = 15   the bias column is the last column of the tile: no padding column left

16 .. 64 is the range models.py routes to the GEMM-backed wide path.

Nothing here needs a GPU: the GPU module imports the lists, the CPU module checks that every case is sound (float32 torch port
against the float64 closed form, inside the GPU tolerances with room to spare) and counts the lists."""
import functools

import numpy as np
import torch

from oracle import vae_oracle as O

LATENTS = (1, 3, 4, 8, 12, 15)
WIDE_LATENTS = (16, 33, 64)
L_REF = 10  # the width of the rest of the suite: kept where a test compares two forms, so a failure shows as specific to a width
TP = {"batch_size": 64, "patience": 100}

# the project's tolerances for the same comparisons at L = 10 (tests/test_gpu_parity.py, tests/test_bf16.py, tests/test_reward.py)
FWD_ATOL, Z_ATOL = 2e-5, 3e-5
LOSS_RTOL, GRAD_RTOL = 2e-5, 2e-4
TRAJ_LOSS_RTOL, TRAJ_PARAM_RTOL = 3e-5, 1e-4  # test_fused_adam_trajectory_matches_golden
BF16_TOL = {"bf16x3": (1e-4, 5e-3), "bf16": (5e-3, 0.15)}  # test_ragged_and_full_size_vs_f32_path
# the CPU soundness check holds the float32 port to a quarter of a GPU tolerance: the kernel's own summation order gets the rest
ROOM = 4.0

# d = 13: padded columns; 72: in (64, 128], % 4 == 0, both decoder kernels; 128: full width
# B = 5: less than a 16-row tile; 37: ragged 16-row tiles; 130: two 64-row tiles + 2, one 128-row tile + 2
FORWARD_SHAPES = ((13, 5), (128, 37))
API_SHAPES = ((13, 5), (72, 37))
API_FORMS = ("kl_reg", "ml_reg", "vanilla")
STEP_SHAPES = ((13, 5), (72, 37), (128, 130))
# the two-pass losses (ml_reg: a third eps plane and its log-likelihood term, masked per column by L) and the one-pass loss
STEP_KINDS = ("kl_reg", "ml_reg", "vanilla")
# workgroup shapes of FusedTrainer's fp32 step: the N-split kernel (VPC_TILE unset, csrc/vpc_small.hip), the 64-row shape, the
# 128-row shape with the 8-wave decoder (VPC_DEC8=1; below d = 65 the 4-wave one is the only one) and, in (64, 128], with the
# 4-wave / two-tile decoder (VPC_DEC8=0)
STEP_FORMS = ("nsplit", "tile64", "tile128", "tile128_dec4")
STEP_ENV = {"nsplit": {}, "tile64": {"VPC_TILE": "64"}, "tile128": {"VPC_TILE": "128", "VPC_DEC8": "1"},
            "tile128_dec4": {"VPC_TILE": "128", "VPC_DEC8": "0"}}
ADAM_SHAPE = (72, 37)
BF16_LATENTS = (1, 4, 12, 15)
BF16_SHAPES = ((72, 130), (72, 300), (128, 130), (128, 300))
BF16_TILES = ("64", "128")
BF16_PRECS = ("bf16x3", "bf16")
EDGE_LATENTS = (1, 4, 15)  # groups that run a second family of kernels: the three widths with no L = 10 neighbour
AUGM_DIMS = (13, 40, 64)
AUGM_B = 37
AUGM_KINDS = STEP_KINDS
AUGM_PATHS = ("step_small", "decoder_fused")
DRAW_D = 72
EVAL_LATENTS = (1, 8, 15)
EVAL_DIMS = (14, 72)
REWARD_SHAPES = ((13, 5, 17), (100, 6, 7))  # (d, n, M)
REWARD_KINDS = ("plain", "mask", "eddi")
EDDI_SHAPES = ((40, 7, 37), (128, 20, 130))  # (d, K, B)
EDDI_KINDS = STEP_KINDS
ENSEMBLE_FAMILIES = ("plain", "mask", "eddi")
WIDE_CASES = ((14, 16, 37), (129, 33, 70), (40, 64, 33))  # (d, L, B)


def step_forms(d):
    return STEP_FORMS if d > 64 else STEP_FORMS[:3]


FORWARD_CASES = [(L, d, B) for L in LATENTS for d, B in FORWARD_SHAPES]
API_CASES = [(L, d, B, form) for L in LATENTS for d, B in API_SHAPES for form in API_FORMS]
STEP_CASES = [(L, d, B, form, kind) for L in LATENTS for d, B in STEP_SHAPES for form in step_forms(d) for kind in STEP_KINDS]
ADAM_CASES = [(L, kind) for L in LATENTS for kind in ("reg", "vanilla")]
BF16_CASES = [(L, d, B, tile, prec) for L in BF16_LATENTS for d, B in BF16_SHAPES for tile in BF16_TILES for prec in BF16_PRECS]
AUGM_CASES = [(L, d, kind, path) for L in EDGE_LATENTS for d in AUGM_DIMS for kind in AUGM_KINDS for path in AUGM_PATHS]
DRAW_CASES = [(L, rt) for L in EDGE_LATENTS + (L_REF,) for rt in ("kl_reg", None)]
EVAL_CASES = [(L, d, kind) for L in EVAL_LATENTS for d in EVAL_DIMS for kind in ("reg", "vanilla")]
REWARD_CASES = [(L, d, n, M, kind) for L in EDGE_LATENTS for d, n, M in REWARD_SHAPES for kind in REWARD_KINDS]
EDDI_CASES = [(L, d, K, B, kind) for L in EDGE_LATENTS for d, K, B in EDDI_SHAPES for kind in EDDI_KINDS]
ENSEMBLE_CASES = [(L, fam) for L in EDGE_LATENTS for fam in ENSEMBLE_FAMILIES]


def lid(L):
    """The test-id fragment of a latent width: names the boundary it was chosen for."""
    return {1: "L1_one_column", 3: "L3_bias_ends_quad", 4: "L4_bias_opens_quad", 8: "L8_bias_opens_quad",
            12: "L12_bias_opens_quad", 15: "L15_bias_last_column", 10: "L10_suite_width"}.get(L, f"L{L}")


def case_id(case):
    L, rest = case[0], case[1:]
    return lid(L) + "".join("-" + str(r) for r in rest)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def synth(B, d, L, seed=0):
    """x, mask, mask_p, eps_q, eps_p, eps_ml: test_gpu_parity.synth with the latent width passed in (and the ml_reg sample)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, d, generator=g)
    mask = torch.rand(B, d, generator=g) < 0.7
    mask_p = mask & (torch.rand(B, d, generator=g) < 0.7)
    eq = torch.randn(B, L, generator=g)
    ep = torch.randn(B, L, generator=g)
    eml = torch.randn(B, L, generator=g)
    return x, mask, mask_p, eq, ep, eml


def case_seed(L, d, B):
    return 1000 * L + 7 * d + B


def make_model(cls, d, L, params, reg_type="kl_reg", dev="cuda"):
    """test_gpu_parity.make_model with the latent width passed in; `cls` is a class of the package."""
    import vpc_amd as vpc
    extra = [reg_type] if issubclass(cls, vpc.Reg_VAE) else []
    m = cls(d, 500, 10, L, TP, "exp", *extra)
    sd = m.state_dict()
    sd.update({k: v.clone() for k, v in params.items()})
    m.load_state_dict(sd)
    return m.to(dev)


# ---------------------------------------------------------------------------------------------- references, computed once
STEP_KW = {"kl_reg": dict(alpha=0.8, beta=0.9), "ml_reg": dict(alpha=0.8, beta=0.9, epoch=1400), "vanilla": dict(beta=0.9)}


@functools.lru_cache(maxsize=None)
def step_case(form, L, d, B, mask_augm=False):
    """One training step of the dense family at (L, d, B): parameters, inputs and the float32 port's loss and gradients.
    form: "kl_reg" / "ml_reg" (two passes) or "vanilla".  The result is shared between tests: read-only."""
    seed = case_seed(L, d, B)
    params = O.init_params(d, L, seed=seed, mask_augm=mask_augm)
    data = synth(B, d, L, seed=seed + 1)
    x, mask, mask_p, eq, ep, eml = data
    kw = STEP_KW[form]
    aug = {"mask_augm": True} if mask_augm else {}
    if form == "vanilla":
        loss, grads, outs = O.torch_vanilla_step(params, L, x, mask, eq, **kw, **aug)
    else:
        loss, grads, outs = O.torch_reg_step(params, L, x, mask, mask_p, eq, ep, reg_type=form,
                                             eps_ml=eml if form == "ml_reg" else None, **kw, **aug)
    return params, data, loss.item(), {k: v.numpy() for k, v in grads.items()}, outs


def closed_form_step(form, L, d, B):
    """The float64 closed form of step_case(form, L, d, B) -> (loss, grads)."""
    params, (x, mask, mask_p, eq, ep, eml), _, _, _ = step_case(form, L, d, B)
    xn, mn, mpn = x.numpy().astype(np.float64), mask.numpy(), mask_p.numpy()
    kw = STEP_KW[form]
    if form == "vanilla":
        loss, grads, _ = O.closed_form_vanilla_step(params, L, xn, mn, eq.numpy(), **kw)
    else:
        loss, grads, _, _ = O.closed_form_reg_step(params, L, xn, mn, mpn, eq.numpy(), ep.numpy(), reg_type=form,
                                                   eps_ml=eml.numpy() if form == "ml_reg" else None, **kw)
    return loss, grads


def kind_form(kind):
    return "kl_reg" if kind == "reg" else "vanilla"


# ---------------------------------------------------------------------------------------------- comparisons
WORST = {}


def record(group, what, err, tol):
    """Keeps (and prints, for `pytest -rA`) the worst figure of a group next to its tolerance."""
    key = (group, what)
    if key not in WORST or err > WORST[key][0]:
        WORST[key] = (err, tol)
    print(f"LATFIG {group} {what} {err:.3e} tol {tol:.1e}")


def check_loss_grads(group, loss, flat, model, loss_ref, grads_ref, what, loss_tol=LOSS_RTOL, grad_tol=GRAD_RTOL):
    """A loss and a flat gradient (state_dict order) against a reference {key: array}: loss relative, every gradient tensor
    relative to its largest entry.  Every figure is printed before it is asserted."""
    flat = np.asarray(flat)
    assert np.isfinite(loss) and np.all(np.isfinite(flat)), what
    le = abs(loss - loss_ref) / abs(loss_ref)
    record(group, "loss", le, loss_tol)
    errs, off = {}, 0
    for k, p in zip(O.PARAM_KEYS, model.trainable()):
        n = p.numel()
        errs[k] = rel(flat[off:off + n].reshape(tuple(p.shape)), grads_ref[k])
        off += n
    assert off == flat.size, what
    record(group, "grad", max(errs.values()), grad_tol)
    assert le <= loss_tol, (what, loss, loss_ref)
    for k, e in errs.items():
        assert e < grad_tol, (what, k, e)


def flat_grads(model):
    return torch.cat([p.grad.reshape(-1) for p in model.trainable()]).cpu().numpy()
