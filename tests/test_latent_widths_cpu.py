"""Latent widths of the dense VAE family, the part that needs no GPU (tests/latent_cases.py):
  1. the cases of test_latent_widths_gpu.py that are held to the torch port are sound: on their very inputs the float32 port
     agrees with the float64 closed form inside a quarter of the tolerance the GPU test holds the kernels to, so a GPU failure
     is the kernel's (the closed form states the plain encoder: the mask-augmented and point-net cases have no such check);
  2. the packed-image chain of test_layout_cpu.py (index tables, bias chain, gradient gather) at L = 1, 4, 12, 15;
  3. the bf16 image tables and the compact image of the whole-step kernel at L = 1, 4, 15;
  4. the case lists have the size LATENTS x shapes x forms, and the GPU module is parametrised with those very lists: a dropped
     case fails here."""
import ctypes as C

import numpy as np
import pytest

import latent_cases as lc
import vpc_amd as vpc
from oracle import vae_oracle as O
from test_layout_cpu import test_packed_chain_matches_oracle as _packed_chain

# ---------------------------------------------------------------------------------------------- 1. the cases are sound
ORACLE_STEPS = sorted({(form, L, d, B) for L, d, B, form in lc.API_CASES} |
                      {(kind, L, d, B) for L, d, B, _, kind in lc.STEP_CASES} |
                      {(lc.kind_form(kind), L) + lc.ADAM_SHAPE for L, kind in lc.ADAM_CASES})


@pytest.mark.parametrize("form,L,d,B", ORACLE_STEPS, ids=[f"{lc.lid(L)}-{f}-d{d}-B{B}" for f, L, d, B in ORACLE_STEPS])
def test_step_cases_are_sound(form, L, d, B):
    _, _, loss32, grads32, _ = lc.step_case(form, L, d, B)
    loss64, grads64 = lc.closed_form_step(form, L, d, B)
    assert np.isfinite(loss64) and abs(loss32 - loss64) <= lc.LOSS_RTOL / lc.ROOM * abs(loss64), (loss32, loss64)
    for k in O.PARAM_KEYS:
        assert np.max(np.abs(grads64[k])) > 0, k  # a gradient tensor of zeros would make the relative bound empty
        assert lc.rel(grads32[k], grads64[k]) < lc.GRAD_RTOL / lc.ROOM, k


@pytest.mark.parametrize("L,d,B", lc.FORWARD_CASES, ids=[lc.case_id(c) for c in lc.FORWARD_CASES])
def test_forward_cases_are_sound(L, d, B):
    seed = lc.case_seed(L, d, B)
    params = O.init_params(d, L, seed=seed)
    x, mask, _, eq, _, _ = lc.synth(B, d, L, seed=seed + 1)
    port = O.TorchPort(params, L)
    z, mean, lv = port.encoder(x, mask, eq)
    xh, _ = port.decoder(z)
    c = O.closed_form_pass(O._np(params), x.numpy().astype(np.float64), mask.numpy().astype(np.float64),
                           eq.numpy().astype(np.float64), L)
    assert mean.shape == (B, L) and c.mean.shape == (B, L)
    for got, want, tol in ((mean, c.mean, lc.FWD_ATOL), (lv, c.logvar, lc.FWD_ATOL), (z, c.z, lc.Z_ATOL), (xh, c.xhat, lc.FWD_ATOL)):
        assert np.max(np.abs(got.numpy() - want)) <= tol / lc.ROOM


# ---------------------------------------------------------------------------------------------- 2. packed chain
@pytest.mark.parametrize("d,Ld", [(13, 1), (72, 4), (128, 12), (128, 15)])
def test_packed_chain_matches_oracle_at_latent_edges(d, Ld):
    """test_layout_cpu.test_packed_chain_matches_oracle, whose own list is (14, 10), (128, 10), (40, 6), (64, 15)."""
    _packed_chain(d, Ld)


# ---------------------------------------------------------------------------------------------- 3. bf16 tables
@pytest.mark.parametrize("L", [1, 4, 15], ids=lc.lid)
def test_bf16_image_tables(L):
    """test_bf16.test_bf16_image_tables_cpu with the latent width passed in."""
    lay = vpc._lib.layout(128, L)
    l = vpc._lib.lib()
    e, dd = C.c_int(), C.c_int()
    assert l.vpc_layout_sizes_bf16(128, L, 0, C.byref(e), C.byref(dd)) == 0
    assert e.value == lay.enc_img and dd.value == lay.dec_img + 64 * 16
    idx = np.empty(lay.n_params, np.int32)
    tmpl = np.empty(e.value + dd.value, np.float32)
    assert l.vpc_build_indices_bf16(128, L, 0, idx.ctypes.data_as(C.c_void_p), tmpl.ctypes.data_as(C.c_void_p)) == 0
    w = idx[idx >= 0]
    used = np.concatenate([w, w + 8])
    assert len(w) == lay.n_params - 100
    assert len(np.unique(used)) == len(used) and used.max() < 2 * tmpl.size
    b = -(idx[idx < 0] + 1)
    assert len(b) == 100 and len(np.unique(b)) == 100
    u = tmpl.view(np.uint16)
    assert (u == 0x3F80).sum() == 3 + 1
    assert not np.isin(np.flatnonzero(u == 0x3F80), used).any()
    assert np.count_nonzero(u) == 4  # nothing but the four constants
    assert l.vpc_layout_sizes_bf16(128, 16, 0, None, None) == 2


@pytest.mark.parametrize("L", [1, 4, 15], ids=lc.lid)
def test_step_image_tables(L):
    """test_bf16.test_step_image_tables_cpu with the latent width passed in."""
    l = vpc._lib.lib()
    n, lds = C.c_int(), C.c_int()
    assert l.vpc_step_layout_bf16(128, L, C.byref(n), C.byref(lds)) == 0
    assert n.value * 4 == 100864 and lds.value <= 163840
    lay = vpc._lib.layout(128, L)
    idx = np.empty(lay.n_params, np.int32)
    tmpl = np.empty(n.value, np.float32)
    assert l.vpc_step_build_indices_bf16(128, L, idx.ctypes.data_as(C.c_void_p), tmpl.ctypes.data_as(C.c_void_p)) == 0
    w = idx[idx >= 0]
    assert len(w) == lay.n_params - 100
    assert len(np.unique(w)) == len(w) and w.max() < 2 * tmpl.size
    b = -(idx[idx < 0] + 1)
    assert len(b) == 100 and len(np.unique(b)) == 100
    assert not np.isin(w // 2, b).any()
    u = tmpl.view(np.uint16)
    ones = np.flatnonzero(u == 0x3F80)
    assert len(ones) == 3 + 1 and not np.isin(ones, w).any()
    assert np.count_nonzero(u) == 4
    assert l.vpc_step_layout_bf16(128, 16, None, None) == 2 and l.vpc_step_layout_bf16(128, 0, None, None) == 2
    assert l.vpc_step_fused_applicable(130, 128, L, 2) == 1 and l.vpc_step_fused_applicable(130, 128, 16, 2) == 0


# ---------------------------------------------------------------------------------------------- 4. counting
def test_case_lists_are_complete():
    nL, nE = len(lc.LATENTS), len(lc.EDGE_LATENTS)
    assert lc.LATENTS == (1, 3, 4, 8, 12, 15) and lc.WIDE_LATENTS == (16, 33, 64) and lc.EDGE_LATENTS == (1, 4, 15)
    assert len(lc.FORWARD_CASES) == nL * len(lc.FORWARD_SHAPES) == 12
    assert len(lc.API_CASES) == nL * len(lc.API_SHAPES) * len(lc.API_FORMS) == 36
    # d = 13 has three workgroup forms, d = 72 and 128 four (both decoder kernels)
    assert len(lc.STEP_CASES) == nL * (3 + 4 + 4) * len(lc.STEP_KINDS) == 198
    assert len(lc.ADAM_CASES) == nL * 2
    assert len(lc.BF16_CASES) == len(lc.BF16_LATENTS) * len(lc.BF16_SHAPES) * len(lc.BF16_TILES) * len(lc.BF16_PRECS) == 64
    assert len(lc.AUGM_CASES) == nE * len(lc.AUGM_DIMS) * len(lc.AUGM_KINDS) * len(lc.AUGM_PATHS) == 54
    assert len(lc.DRAW_CASES) == (nE + 1) * 2
    assert len(lc.EVAL_CASES) == len(lc.EVAL_LATENTS) * len(lc.EVAL_DIMS) * 2 == 12
    assert len(lc.REWARD_CASES) == nE * len(lc.REWARD_SHAPES) * len(lc.REWARD_KINDS) == 18
    assert len(lc.EDDI_CASES) == nE * len(lc.EDDI_SHAPES) * len(lc.EDDI_KINDS) == 18
    assert len(lc.ENSEMBLE_CASES) == nE * len(lc.ENSEMBLE_FAMILIES) == 9
    assert [L for _, L, _ in lc.WIDE_CASES] == list(lc.WIDE_LATENTS)
    for cases in (lc.FORWARD_CASES, lc.API_CASES, lc.STEP_CASES, lc.ADAM_CASES):
        assert {c[0] for c in cases} == set(lc.LATENTS)
    # every boundary is named in a test id
    assert all(str(L) in lc.lid(L) and lc.lid(L) != f"L{L}" for L in lc.LATENTS)


def test_gpu_module_runs_every_case():
    """The GPU module's parametrisations are these lists, and none of its tests carries a skip or expected-failure mark."""
    import test_latent_widths_gpu as G
    for name, cases in G.CASES_OF.items():
        fn = getattr(G, name)
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        assert len(marks) == 1 and list(marks[0].args[1]) == list(cases), name
        assert len(marks[0].kwargs["ids"]) == len(cases) == len(set(marks[0].kwargs["ids"])), name
    tests = [n for n in dir(G) if n.startswith("test_")]
    assert set(G.CASES_OF) <= set(tests)
    for n in tests:
        assert not [m for m in getattr(getattr(G, n), "pytestmark", []) if m.name in ("skip", "skipif", "xfail")], n
