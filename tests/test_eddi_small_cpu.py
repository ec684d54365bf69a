"""Host arithmetic of the small-batch one-kernel step of the point-net classes (Reg_EDDI / vanilla_EDDI: vpc_step_small_eddi_f32,
vpc_reduce_step_adam_eddi).  No GPU: the routing predicate, the point-net layout against a numpy restatement, the front-end's
chain rule against autograd in float64, the refusals of the C entries."""
import ctypes

import numpy as np
import pytest
import torch

import vpc_amd as vpc
from vpc_amd import eddi, ops
from vpc_amd._lib import HIDDEN_POS1 as POS1, HIDDEN_POS2 as POS2

OK, ERR_ARG, ERR_SHAPE = 0, 1, 2
H1, H2 = 100, 50


# ------------------------------------------------------------------ routing
def test_tiles_per_shape():
    assert ops.small_eddi_tiles(12, 10) == (1, 1) and ops.small_eddi_tiles(12, 16) == (1, 1)
    assert ops.small_eddi_tiles(12, 17) == (2, 1) and ops.small_eddi_tiles(12, 32) == (2, 1)
    assert ops.small_eddi_tiles(17, 20) == (2, 2) and ops.small_eddi_tiles(33, 10) == (1, 4) and ops.small_eddi_tiles(64, 32) == (2, 4)
    assert ops.small_eddi_tiles(65, 20) is None and ops.small_eddi_tiles(128, 20) is None
    assert ops.small_eddi_tiles(12, 33) is None and ops.small_eddi_tiles(12, 0) is None and ops.small_eddi_tiles(0, 10) is None


@pytest.mark.parametrize("d,K,B,world,rows,want", [
    (12, 10, 64, 1, 4096, True), (12, 20, 64, 1, 4096, True), (64, 32, 4096, 1, 4096, True), (14, 10, 1, 1, 4096, True),
    (12, 10, 4097, 1, 4096, False),   # above the row limit
    (12, 10, 64, 1, 0, False),        # VPC_STEP_SMALL=0
    (12, 10, 64, 2, 4096, False),     # data parallel
    (65, 20, 64, 1, 4096, False), (128, 20, 64, 1, 4096, False), (12, 33, 64, 1, 4096, False),   # no instantiation
    (12, 10, 0, 1, 4096, False)])
def test_routing_predicate(d, K, B, world, rows, want):
    assert eddi.small_step_route(d, K, B, world, rows) is want


def test_environment_sets_the_row_limit(monkeypatch):
    monkeypatch.delenv("VPC_TILE", raising=False)
    monkeypatch.setenv("VPC_STEP_SMALL", "0")
    assert ops.step_small_max_rows() == 0 and not eddi.small_step_route(12, 10, 64, 1, ops.step_small_max_rows())
    monkeypatch.setenv("VPC_STEP_SMALL", "64")
    assert eddi.small_step_route(12, 10, 64, 1, ops.step_small_max_rows())
    assert not eddi.small_step_route(12, 10, 65, 1, ops.step_small_max_rows())
    monkeypatch.delenv("VPC_STEP_SMALL")
    assert ops.step_small_max_rows() >= 64 and eddi.small_step_route(12, 10, 64, 1, ops.step_small_max_rows())


# ------------------------------------------------------------------ layout
def swz(col, row, S=64):
    return (((col >> 2) ^ (row & 15 & (S // 4 - 1))) << 2) | (col & 3)


def expected_pack_idx(d, K, L):
    """pack_idx of the twelve tiled tensors, restated from csrc/vpc_layout.h: encoder image [W1: 112 x 64][b1: 128][W2: 64 x 128]
    [W3: 32 x 64] with the trunk's input K wide, then the decoder image [W4: 64 x 16][W5: 112 x 64][W6: 16 DT x 128]."""
    dt = 1 if d <= 16 else 2 if d <= 32 else 4 if d <= 64 else 8
    oW1, ob1 = 0, 112 * 64
    oW2 = ob1 + 128
    oW3 = oW2 + 64 * 128
    DB = oW3 + 32 * 64
    oW4, oW5 = DB, DB + 64 * 16
    oW6 = oW5 + 112 * 64
    idx = []
    idx += [oW1 + POS1[o] * 64 + swz(i, POS1[o]) for o in range(H1) for i in range(K)]
    idx += [ob1 + POS1[o] for o in range(H1)]
    idx += [oW2 + POS2[o] * 128 + swz(POS1[i], POS2[o]) for o in range(H2) for i in range(H1)]
    idx += [oW2 + POS2[o] * 128 + swz(POS1[H1], POS2[o]) for o in range(H2)]
    row3 = lambda o: o if o < L else 16 + (o - L)
    idx += [oW3 + row3(o) * 64 + swz(POS2[i], row3(o)) for o in range(2 * L) for i in range(H2)]
    idx += [oW3 + row3(o) * 64 + swz(POS2[H2], row3(o)) for o in range(2 * L)]
    idx += [oW4 + POS2[o] * 16 + swz(i, POS2[o], 16) for o in range(H2) for i in range(L)]
    idx += [oW4 + POS2[o] * 16 + swz(L, POS2[o], 16) for o in range(H2)]
    idx += [oW5 + POS1[o] * 64 + swz(POS2[i], POS1[o]) for o in range(H1) for i in range(H2)]
    idx += [oW5 + POS1[o] * 64 + swz(POS2[H2], POS1[o]) for o in range(H1)]
    idx += [oW6 + o * 128 + swz(POS1[i], o) for o in range(d) for i in range(H1)]
    idx += [oW6 + o * 128 + swz(POS1[H1], o) for o in range(d)]
    ones = [ob1 + POS1[H1], oW2 + POS2[H2] * 128 + swz(POS1[H1], POS2[H2]), oW4 + POS2[H2] * 16 + swz(L, POS2[H2], 16),
            oW5 + POS1[H1] * 64 + swz(POS2[H2], POS1[H1])]
    return np.array(idx), ones, DB, oW6 + 16 * dt * 128 - DB


@pytest.mark.parametrize("d,K,L", [(12, 10, 10), (12, 20, 10), (14, 16, 10), (40, 20, 6), (64, 32, 15), (128, 1, 1)])
def test_pointnet_layout(d, K, L):
    lay = vpc._lib.pointnet_layout(d, K, L)
    n_trunk = H1 * K + H1 + H2 * H1 + H2 + 2 * L * H2 + 2 * L
    n_dec = H2 * L + H2 + H1 * H2 + H1 + d * H1 + d
    assert (lay.n_enc, lay.n_params, lay.n_front) == (n_trunk, n_trunk + n_dec, d * K + d + K * (2 + K) + K)
    want, ones, enc_img, dec_img = expected_pack_idx(d, K, L)
    assert (lay.enc_img, lay.dec_img) == (enc_img, dec_img)
    assert np.array_equal(lay.pack_idx, want)
    # every parameter has exactly one place in the images, none on a constant of the bias chain; everything else is padding: zero
    assert len(set(lay.pack_idx.tolist())) == lay.n_params and lay.pack_idx.min() >= 0 and lay.pack_idx.max() < enc_img + dec_img
    tmpl = lay.img_template
    assert sorted(np.flatnonzero(tmpl).tolist()) == sorted(ones) and np.all(tmpl[ones] == 1.0)
    assert not set(ones) & set(lay.pack_idx.tolist())
    img = tmpl.copy()
    img[lay.pack_idx] = np.arange(1, lay.n_params + 1)
    rest = np.setdiff1d(np.arange(img.size), np.concatenate([lay.pack_idx, ones]))
    assert np.all(img[rest] == 0.0) and np.count_nonzero(img) == lay.n_params + 4
    # and exactly one place in its partial block
    ge, gd = lay.grad_idx[:lay.n_enc], lay.grad_idx[lay.n_enc:]
    assert len(set(ge.tolist())) == ge.size and ge.min() >= 0 and ge.max() < lay.enc_part
    assert len(set(gd.tolist())) == gd.size and gd.min() >= 0 and gd.max() < lay.dec_part
    # the decoder half is the dense layout's: the model's own decoder image and the step's agree
    dense = vpc._lib.layout(d, L)
    assert np.array_equal(lay.pack_idx[lay.n_enc:] - lay.enc_img, dense.pack_idx[dense.n_enc:] - dense.enc_img)
    assert np.array_equal(gd, dense.grad_idx[dense.n_enc:])


def test_existing_layouts_are_unchanged():
    for d, aug in ((12, False), (12, True), (128, False), (64, True)):
        lay = vpc._lib.Layout(d, 10, aug)
        din = 2 * d if aug else d
        assert lay.n_enc == H1 * din + H1 + H2 * H1 + H2 + 20 * H2 + 20 and lay.K == 0 and lay.n_front == 0
    l = vpc._lib.lib()
    v = ctypes.c_int()
    assert l.vpc_layout_sizes(65, 10, 1, None, None, None, ctypes.byref(v), None, None, None, None) == ERR_SHAPE
    assert l.vpc_layout_sizes_pointnet(12, 33, 10, *([None] * 9)) == ERR_SHAPE
    assert l.vpc_layout_sizes_pointnet(12, 0, 10, *([None] * 9)) == ERR_SHAPE
    assert l.vpc_layout_sizes_pointnet(129, 10, 10, *([None] * 9)) == ERR_SHAPE
    assert l.vpc_build_indices_pointnet(12, 33, 10, None, None, None) == ERR_SHAPE
    assert l.vpc_build_indices_pointnet(12, 10, 10, None, None, None) == ERR_ARG


# ------------------------------------------------------------------ chain rule
def front_chain_rule(dA, dC, E, tb, Wp):
    """The tail's arithmetic (csrc/vpc_misc.hip: front_tail_body; csrc/vpc_eddi.hip: eddi_param_bwd_kernel), term by term: from the
    gradients of A_j = w_x + W_E E_j and C_j = w_t t_j + c, both [K][d], to those of type_pars1 [d][K], type_bias1 [d][1],
    pnp_encoder1.0.weight [K][2+K] = [w_x | W_E | w_t] and pnp_encoder1.0.bias [K]."""
    K, d = dA.shape
    gE, gtb, gWp, gcp = torch.zeros(d, K, dtype=dA.dtype), torch.zeros(d, 1, dtype=dA.dtype), torch.zeros(K, 2 + K, dtype=dA.dtype), \
        torch.zeros(K, dtype=dA.dtype)
    for j in range(d):
        for e in range(K):
            gE[j, e] = sum(Wp[k, 1 + e] * dA[k, j] for k in range(K))      # dE[j][e] = sum_k W_E[k][e] dA[k][j]
        gtb[j, 0] = sum(Wp[k, 1 + K] * dC[k, j] for k in range(K))          # dt[j] = sum_k w_t[k] dC[k][j]
    for k in range(K):
        gWp[k, 0] = dA[k].sum()                                              # dW[k][0] = sum_j dA
        for e in range(K):
            gWp[k, 1 + e] = sum(dA[k, j] * E[j, e] for j in range(d))       # dW[k][1+e] = sum_j dA E[j][e]
        gWp[k, 1 + K] = sum(dC[k, j] * tb[j, 0] for j in range(d))          # dW[k][1+K] = sum_j dC t[j]
        gcp[k] = dC[k].sum()                                                 # dc[k] = sum_j dC[k][j]
    return gE, gtb, gWp, gcp


@pytest.mark.parametrize("d,K", [(12, 10), (14, 20), (5, 32)])
def test_front_chain_rule_against_autograd(d, K):
    """(dA, dC) -> (type_pars1, type_bias1, pnp_encoder1.0.weight, .bias): the arithmetic of the tail, in float64, against autograd
    through the unfolded front-end of the reference (VAE.py:719-733: Linear(2 + K -> K) on [x, x E_j, t_j], ReLU, masked sum)."""
    g = torch.Generator().manual_seed(d * K)
    B = 9
    f64 = dict(dtype=torch.float64, generator=g)
    x, m = torch.rand(B, d, **f64), (torch.rand(B, d, generator=g) < 0.7).double()
    E, tb = torch.randn(d, K, **f64).requires_grad_(), torch.randn(d, 1, **f64).requires_grad_()
    Wp, cp = (0.3 * torch.randn(K, 2 + K, **f64)).requires_grad_(), (0.3 * torch.randn(K, **f64)).requires_grad_()
    dagg = torch.randn(B, K, **f64)
    xf = x.reshape(-1, 1)
    feat = torch.cat([xf, xf * E.repeat(B, 1), tb.repeat(B, 1)], 1)
    h = torch.relu(torch.nn.functional.linear(feat, Wp, cp)).reshape(B, d, K)
    ((m.reshape(B, d, 1) * h).sum(1) * dagg).sum().backward()
    with torch.no_grad():  # the folded form the kernel accumulates: dA[k][j] = sum_r g x, dC[k][j] = sum_r g
        A = Wp[:, :1] + Wp[:, 1:1 + K] @ E.t()                       # [K][d]
        C = Wp[:, 1 + K:] * tb.t() + cp.reshape(-1, 1)
        gate = m.t().unsqueeze(0) * ((x.t().unsqueeze(0) * A.unsqueeze(2) + C.unsqueeze(2)) > 0) * dagg.t().unsqueeze(1)  # [K][d][B]
        dA, dC = (gate * x.t().unsqueeze(0)).sum(2), gate.sum(2)
        got = front_chain_rule(dA, dC, E, tb, Wp)
    for a, p, name in zip(got, (E, tb, Wp, cp), ("type_pars1", "type_bias1", "pnp_encoder1.0.weight", "pnp_encoder1.0.bias")):
        assert a.shape == p.grad.shape, name
        assert float((a - p.grad).abs().max()) <= 1e-12 * max(1.0, float(p.grad.abs().max())), name


# ------------------------------------------------------------------ C entries
def test_c_entries_refuse_before_any_launch():
    """Host buffers and no device: every refusal is returned by the argument checks."""
    l = vpc._lib.lib()
    host = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(host))
    ptrs = (ctypes.c_void_p * 2)(p.value, p.value)
    co = vpc._lib.VpcLossCoef([1.0], [0.0], 1.0)
    nb = ctypes.byref(ctypes.c_int())

    def both(d, d_real, K, x=p, front=p):
        head = (x, p, p, 1, ptrs, None, co, ptrs, None, 1.0, 0.0, p, p, p, nb, 16, d, d_real, 10, K, front, p, p)
        a = l.vpc_step_small_eddi_f32(*head, None)
        b = l.vpc_step_small_eddi_draw_f32(*head, None, 0.7, p, 256, 0, 0, 0, None, 0, 16, 16, 0, 16, None)
        assert a == b
        return a

    assert both(12, 12, 33) == ERR_SHAPE and both(12, 12, 0) == ERR_SHAPE
    assert both(14, 14, 10) == ERR_SHAPE     # d % 4 != 0
    assert both(12, 13, 10) == ERR_SHAPE and both(16, 12, 10) == ERR_SHAPE and both(12, 0, 10) == ERR_SHAPE
    assert both(68, 68, 10) == ERR_SHAPE     # no instantiation past obs_dim 64
    assert both(16, 14, 10, x=ctypes.c_void_p(p.value + 4)) == ERR_ARG
    assert both(16, 14, 10, front=ctypes.c_void_p(p.value + 2)) == ERR_ARG
    assert both(16, 14, 10, front=None) == ERR_ARG
    tail = lambda K, dp, inv=p: l.vpc_reduce_step_adam_eddi(p, 1, 24704, p, 1, 23552, inv, p, 100, p, 1, co, 16, 16, 12, p, p, p, p, p,
                                                            1e-3, 0.9, 0.999, 1e-8, 1, p, p, p, 1, p, K, dp, None)
    assert tail(33, 12) == ERR_SHAPE and tail(10, 8) == ERR_SHAPE and tail(10, 68) == ERR_SHAPE
    assert tail(10, 12, inv=None) == ERR_ARG
