"""The few-row layer ops (csrc/vpc_rows.hip: rows_fwd_kernel<VEC>, rows_bwd_kernel<VN, VK>), driven through vpc_amd.linear
and held to a float64 torch reference of the same operation on the same fp32 operands.  Method and bounds are those of
test_linear_gpu.py, restated here:

  * outputs are pre-filled with NaN, so an element the kernel does not write fails the comparison;
  * fp32 forward 1e-5 and gradients 2e-5 of max(1, |ref|max); forward and data-gradient bounds scaled by
    sqrt(contraction / 128) above 128 (the rounding error of an fp32 sum grows like the square root of its length); the
    weight-gradient bound unscaled (its contraction is at most 128 rows); bias sums 1e-5.

Shapes: M at and around the 16-row MFMA tile and the 64-row workgroup (1, 15, 16, 17, 37, 74, 128); (N, K) = the flow model's
layers at hid_dim 500 (24 -> 500, 500 -> 500, 500 -> 100, 10 -> 500, 500 -> 12) and two that are smaller than one tile."""
import math
from functools import cached_property

import pytest
import torch

from vpc_amd import linear as lin
from vpc_amd._lib import VpcError

pytestmark = pytest.mark.gpu

NAN = float("nan")
NONE, ELU, SIGHT, RELU = lin.ACT_NONE, lin.ACT_ELU, lin.ACT_SIGMOID_HARDTANH, lin.ACT_RELU
ROWS = [1, 15, 16, 17, 37, 74, 128]
LAYERS = [(500, 24), (500, 500), (100, 500), (500, 10), (12, 500), (7, 5), (16, 4)]
LAYER_IDS = [f"n{n}k{k}" for n, k in LAYERS]


# ------------------------------------------------------------------------------------------------ float64 reference
def _act(v, act, split):
    if act == ELU:
        return torch.nn.functional.elu(v)
    if act == SIGHT:
        return torch.cat([torch.sigmoid(v[:, :split]), torch.nn.functional.hardtanh(v[:, split:], -10.0, 0.0)], 1)
    if act == RELU:
        return torch.relu(v)
    return v


def _act_grad(y, act, split):
    """Derivative of the activation through its OUTPUT y, as the kernel forms it."""
    if act == ELU:
        return torch.where(y > 0, torch.ones_like(y), y + 1)
    if act == SIGHT:
        return torch.cat([y[:, :split] * (1 - y[:, :split]), ((y[:, split:] > -10) & (y[:, split:] < 0)).to(y.dtype)], 1)
    if act == RELU:
        return (y > 0).to(y.dtype)
    return torch.ones_like(y)


class _Data:
    """Seeded fp32 operands of one layer on M rows, and its float64 results (each computed once, then shared)."""

    def __init__(self, M, N, K, gate, prev, gsplit):
        self.M, self.N, self.K, self.gate, self.prev, self.gsplit = M, N, K, gate, prev, gsplit
        self._ref = {}

    def _randn(self, tag, *shape):
        g = torch.Generator(device="cuda").manual_seed(1000003 * tag + 7 * self.M + 13 * self.N + self.K)
        return torch.randn(*shape, device="cuda", generator=g)

    @cached_property
    def x(self):  # the layer's input = the previous layer's output
        return _act(self._randn(1, self.M, self.K), self.prev, self.K)

    @cached_property
    def w(self):
        return self._randn(2, self.N, self.K) / self.K ** 0.5

    @cached_property
    def b(self):
        return self._randn(3, self.N)

    @cached_property
    def y(self):  # the layer's output, for the gate on load
        return _act(self._randn(4, self.M, self.N) * 3, self.gate, self.gsplit)

    @cached_property
    def dy(self):
        return self._randn(5, self.M, self.N)

    def fwd_ref(self, act, split, bias=True):
        key = ("fwd", act, split, bias)
        if key not in self._ref:
            pre = self.x.double() @ self.w.double().t()
            self._ref[key] = _act(pre + self.b.double() if bias else pre, act, split)
        return self._ref[key]

    def dpre(self, gated):
        key = ("dpre", gated)
        if key not in self._ref:
            dy = self.dy.double()
            self._ref[key] = dy * _act_grad(self.y.double(), self.gate, self.gsplit) if gated else dy
        return self._ref[key]

    def dx_ref(self, gated, use_prev):
        key = ("dx", gated, use_prev)
        if key not in self._ref:
            dx = self.dpre(gated) @ self.w.double()
            self._ref[key] = dx * _act_grad(self.x.double(), self.prev, self.K) if use_prev else dx
        return self._ref[key]

    def dw_ref(self, gated):
        key = ("dw", gated)
        if key not in self._ref:
            self._ref[key] = (self.dpre(gated).t() @ self.x.double(), self.dpre(gated).sum(0))
        return self._ref[key]


@pytest.fixture(scope="module")
def data():
    cache = {}

    def get(M, N, K, gate=SIGHT, prev=ELU, gsplit=None):
        key = (M, N, K, gate, prev, gsplit)
        if key not in cache:
            cache[key] = _Data(M, N, K, gate, prev, N // 2 if gsplit is None else gsplit)
        return cache[key]

    yield get
    cache.clear()


# ------------------------------------------------------------------------------------------------ bounds
def _check(got, ref, base, length, what):
    assert bool(torch.isfinite(got).all()), f"{what}: unwritten or non-finite elements"
    err, scale = float((got.double() - ref).abs().max()), max(1.0, float(ref.abs().max()))
    bound = base * max(1.0, math.sqrt(length / 128))
    print(f"{what}: err / scale {err / scale:.3e}, bound {bound:.3e}")
    assert err <= bound * scale, f"{what}: max abs err {err:.3e}, scale {scale:.3e}, bound {bound:.3e}"


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _bits(t):
    return t.view(torch.int32)


def _ceil4(n):
    return (n + 3) // 4 * 4


# mode -> (row pitch, offset of the base pointer from a 16-byte boundary, in floats)
_MODES = {None: lambda w: (w, 0), "ld+4": lambda w: (_ceil4(w) + 4, 0), "ld+3": lambda w: (w + 3, 0),
          "off1": lambda w: (_ceil4(w) + 4, 1), "off1dense": lambda w: (w, 1)}


class _Buf:
    """A [rows, width] operand as a view into a larger NaN-filled buffer."""

    def __init__(self, rows, width, mode=None, src=None):
        self.ld, self.off = _MODES[mode](width)
        self.rows, self.width = rows, width
        self.buf = _nan(self.off + rows * self.ld + 4)
        assert self.buf.data_ptr() % 16 == 0
        self.t = self._view(self.buf)
        if src is not None:
            self.t.copy_(src)
        self.before = self.buf.clone()

    def _view(self, buf):
        return buf[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width]

    def assert_unchanged(self, what):
        assert torch.equal(_bits(self.buf), _bits(self.before)), f"{what}: an input buffer was written"

    def assert_padding_untouched(self, what):
        after = self.buf.clone()
        self._view(after).fill_(NAN)
        assert torch.equal(_bits(after), _bits(self.before)), f"{what}: written outside the [rows, width] view"


def _run_fwd(d, lay, act=SIGHT, split=None, bias=True):
    M, N, K = d.M, d.N, d.K
    split = N // 2 if split is None else split
    x, w, y = _Buf(M, K, lay.get("x"), d.x), _Buf(N, K, lay.get("w"), d.w), _Buf(M, N, lay.get("y"))
    lin.rows_fwd(x.t, w.t, d.b if bias else None, y.t, M, N, K, act, split, ldx=x.ld, ldy=y.ld)
    _check(y.t, d.fwd_ref(act, split, bias), 1e-5, K, f"fwd act {act} split {split} {lay}")
    y.assert_padding_untouched("y")
    x.assert_unchanged("x"), w.assert_unchanged("w")
    return y.t


def _run_bwd(d, lay, gated=True, use_prev=True, want_dx=True, want_dw=True, want_db=True, accumulate=False):
    """One rows_bwd call; returns (dx, dw, db) as written."""
    M, N, K = d.M, d.N, d.K
    dy, w, x = _Buf(M, N, lay.get("dy"), d.dy), _Buf(N, K, lay.get("w"), d.w), _Buf(M, K, lay.get("x"), d.x)
    yg = _Buf(M, N, lay.get("y_gate"), d.y) if gated else None
    xo = _Buf(M, K, lay.get("x_out"), d.x) if use_prev else None
    dx = _Buf(M, K, lay.get("dx")) if want_dx else None
    dwb = _Buf(N, K, lay.get("dw")) if want_dw else None
    db = _nan(N) if want_dw and want_db else None
    pre_w = pre_b = None
    if accumulate:
        g = torch.Generator(device="cuda").manual_seed(11)
        pre_w, pre_b = torch.randn(N, K, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g)
        dwb.t.copy_(pre_w), db.copy_(pre_b)
        dwb.before = dwb.buf.clone()
    lin.rows_bwd(dy.t, w.t, x.t, dx.t if want_dx else None, dwb.t if want_dw else None, db, M, N, K,
                 y_gate=yg.t if gated else None, gate=d.gate if gated else NONE, gate_split=d.gsplit,
                 x_out=xo.t if use_prev else None, act_prev=d.prev if use_prev else NONE, accumulate=accumulate, lddy=dy.ld,
                 ldyg=yg.ld if gated else None, ldx=x.ld, ldxo=xo.ld if use_prev else None, lddx=dx.ld if want_dx else None)
    tag = f"gated {gated} prev {use_prev} acc {accumulate} {lay}"
    if want_dx:
        _check(dx.t, d.dx_ref(gated, use_prev), 2e-5, N, f"dx {tag}")
        dx.assert_padding_untouched("dx")
    if want_dw:
        dw_ref, db_ref = d.dw_ref(gated)
        _check(dwb.t, dw_ref + pre_w.double() if accumulate else dw_ref, 2e-5, 128, f"dw {tag}")
        if want_db:
            _check(db, db_ref + pre_b.double() if accumulate else db_ref, 1e-5, 128, f"db {tag}")
    for b in (dy, w, x, yg, xo):
        if b is not None:
            b.assert_unchanged("rows_bwd input")
    return (dx.t if want_dx else None, dwb.t if want_dw else None, db)


# ------------------------------------------------------------------------------------------------ 1. every shape
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N,K", LAYERS, ids=LAYER_IDS)
def test_forward(data, M, N, K):
    """Every activation, Sigmoid | Hardtanh split at 0, N / 2 and N, with and without bias."""
    d = data(M, N, K)
    for act, split in [(NONE, 0), (ELU, 0), (RELU, 0), (SIGHT, 0), (SIGHT, N // 2), (SIGHT, N)]:
        _run_fwd(d, {}, act, split)
    _run_fwd(d, {}, ELU, 0, bias=False)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N,K", LAYERS, ids=LAYER_IDS)
def test_backward(data, M, N, K):
    """With and without y_gate, with and without x_out, dx = None, dw = None, db = None, and accumulate on pre-filled dw / db.
    The two halves of the launch do not depend on each other: dx alone and dw alone are bit-equal to the joint call."""
    d = data(M, N, K)
    dx, dw, db = _run_bwd(d, {})
    _run_bwd(d, {}, gated=False, use_prev=False)
    _run_bwd(d, {}, gated=True, use_prev=False)
    _run_bwd(d, {}, gated=False, use_prev=True)
    dx1, _, _ = _run_bwd(d, {}, want_dw=False)
    _, dw1, db1 = _run_bwd(d, {}, want_dx=False)
    assert torch.equal(dx1, dx) and torch.equal(dw1, dw) and torch.equal(db1, db)
    _, dw2, _ = _run_bwd(d, {}, want_db=False)
    assert torch.equal(dw2, dw)
    _run_bwd(d, {}, accumulate=True)


@pytest.mark.parametrize("gate,prev,where", [(ELU, RELU, None), (RELU, ELU, None), (NONE, NONE, None), (SIGHT, ELU, "0"),
                                             (SIGHT, ELU, "N")])
@pytest.mark.parametrize("M,N,K", [(37, 100, 500), (128, 7, 5)])
def test_backward_gates(data, M, N, K, gate, prev, where):
    """Every activation code as the gate on load and as act_prev; the Sigmoid | Hardtanh gate split at 0 and at N."""
    split = None if where is None else 0 if where == "0" else N
    _run_bwd(data(M, N, K, gate, prev, split), {})


# ------------------------------------------------------------------------------------------------ 2. pitches, alignment
@pytest.mark.parametrize("M,N,K", [(74, 100, 500), (37, 500, 24), (17, 12, 500)])
def test_padded_row_pitches(data, M, N, K):
    """Every operand with a row pitch of ceil4(width) + 4 (the 16-byte path kept) and, again, of width + 3 (lost): padding
    columns of the outputs stay NaN, inputs stay as they were."""
    d = data(M, N, K)
    for mode in ("ld+4", "ld+3"):
        _run_fwd(d, {"x": mode, "y": mode})
        _run_bwd(d, {"dy": mode, "y_gate": mode, "x": mode, "x_out": mode, "dx": mode})


@pytest.mark.parametrize("M,N,K", [(74, 100, 500), (37, 500, 24), (128, 16, 4)])
def test_pointers_offset_by_one_float(data, M, N, K):
    """Every operand starts one float past a 16-byte boundary: the scalar load and store paths (the weights and dw dense,
    the others with a pitch that is a multiple of 4)."""
    d = data(M, N, K)
    _run_fwd(d, {"x": "off1", "w": "off1dense", "y": "off1"})
    _run_bwd(d, {"dy": "off1", "y_gate": "off1", "w": "off1dense", "x": "off1", "x_out": "off1", "dx": "off1",
                 "dw": "off1dense"})
    # one operand at a time: each 16-byte flag off alone
    for name in ("x", "y"):
        _run_fwd(d, {name: "off1"})
    for name in ("dy", "y_gate", "x", "x_out", "dx"):
        _run_bwd(d, {name: "off1"})


# ------------------------------------------------------------------------------------------------ 3. errors
def test_unsupported_shapes_launch_nothing(data):
    d = data(128, 500, 24)
    for M, N in [(129, 500), (128, 1025)]:
        x, w, b = torch.zeros(M, 24, device="cuda"), torch.zeros(N, 24, device="cuda"), torch.zeros(N, device="cuda")
        y, dy = _nan(M, N), torch.zeros(M, N, device="cuda")
        dx, dw, db = _nan(M, 24), _nan(N, 24), _nan(N)
        with pytest.raises(VpcError, match="unsupported shape"):
            lin.rows_fwd(x, w, b, y, M, N, 24)
        with pytest.raises(VpcError, match="unsupported shape"):
            lin.rows_bwd(dy, w, x, dx, dw, db, M, N, 24)
        torch.cuda.synchronize()
        for t in (y, dx, dw, db):
            assert bool(torch.isnan(t).all()), "an output was written by a refused call"
    with pytest.raises(VpcError, match="unsupported shape"):
        lin.rows_fwd(torch.zeros(4, 1025, device="cuda"), torch.zeros(8, 1025, device="cuda"), None, _nan(4, 8), 4, 8, 1025)
    with pytest.raises(VpcError, match="bad argument"):
        lin.rows_fwd(d.x, d.w, d.b, None, 128, 500, 24)
    with pytest.raises(VpcError, match="bad argument"):
        lin.rows_bwd(d.dy, d.w, d.x, None, None, None, 128, 500, 24)
    assert lin.rows_max_rows() == 128


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("M,N,K", [(128, 500, 500), (37, 100, 500), (74, 500, 10)])
def test_two_runs_are_bitwise_equal(data, M, N, K):
    d = data(M, N, K)
    y1, y2 = _run_fwd(d, {}), _run_fwd(d, {})
    assert torch.equal(_bits(y1), _bits(y2))
    a, b = _run_bwd(d, {}), _run_bwd(d, {})
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v))
