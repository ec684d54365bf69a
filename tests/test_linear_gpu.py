"""Every build of the generic GEMM layer ops (csrc/vpc_gemm.hip: linear_kernel<MODE, RAGGED, JT, PREC> and the two
reductions of the wgrad partials), driven through vpc_amd.linear and held to a float64 torch reference of the same
operation on the same fp32 inputs.

Dispatch (T = 2 * num_cus()): forward / dgrad take the wide tiling (JT = 4, 128 batch rows per workgroup) when
ceil(M / 128) * ceil(out_features / 128) >= T and the narrow one (JT = 1) below; wgrad splits the batch S = ceil(T / tiles) ways
(tiles = ceil(N / 128) * ceil(K / 128)), clamped to chunks = ceil(M / 64), each split taking ceil(chunks / S) * 64 rows, so that
with S < chunks the trailing splits hold no rows and must still write zeros.  Shapes that have to land on one side of such a
threshold are derived from vpc_num_cus(), and each test asserts the condition it relies on before the launch.

Outputs and the wgrad scratch are pre-filled with NaN: an element the kernel does not write fails the comparison.

Bounds (the project's, from test_notmiwae_gpu.py / test_bf16.py): fp32 1e-5 forward and 2e-5 gradients of max(1, |ref|max);
bf16x3 1e-5 and bf16 2e-2 of |ref|max; bias sums 1e-5 in every precision.  Those were set at contraction lengths <= 128 for
forward and dgrad; the rounding error of an fp32 sum grows like the square root of its length, so for a longer contraction the
fp32 and bf16x3 bounds of forward and dgrad are scaled by sqrt(len / 128).  The wgrad bound (contraction over the batch) was
set at M = 2560 and is used unscaled: no test here sums more rows than that."""
import math
from functools import cached_property

import pytest
import torch

from vpc_amd import linear as lin
from vpc_amd._lib import VpcError, lib, num_cus

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, BF16X3, BF16 = 0, 1, 2
PRECS = [F32, BF16X3, BF16]
PREC_IDS = ["f32", "bf16x3", "bf16"]
NONE, ELU, SIGHT, RELU = lin.ACT_NONE, lin.ACT_ELU, lin.ACT_SIGMOID_HARDTANH, lin.ACT_RELU


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
    """Derivative of the activation through its OUTPUT y, as the kernel forms it (the formulas of test_notmiwae_gpu.py)."""
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
def _bound(prec, base, length=128):
    if prec == BF16:
        return 2e-2
    return (base if prec == F32 else 1e-5) * max(1.0, math.sqrt(length / 128))


def _check(got, ref, prec, base, length, what):
    assert bool(torch.isfinite(got).all()), f"{what}: unwritten or non-finite elements"
    err, rmax = float((got.double() - ref).abs().max()), float(ref.abs().max())
    scale = max(1.0, rmax) if prec == F32 else rmax + 1e-30
    bound = _bound(prec, base, length)
    print(f"{what}: err / scale {err / scale:.3e}, bound {bound:.3e}")
    assert err <= bound * scale, f"{what}: max abs err {err:.3e}, scale {scale:.3e}, bound {bound:.3e}"


def _check_bias(got, ref, prec, what):
    assert bool(torch.isfinite(got).all()), f"{what}: unwritten or non-finite elements"
    err, rmax = float((got.double() - ref).abs().max()), float(ref.abs().max())
    scale = max(1.0, rmax) if prec == F32 else rmax + 1e-30
    print(f"{what}: err / scale {err / scale:.3e}, bound 1.000e-05")
    assert err <= 1e-5 * scale, f"{what}: max abs err {err:.3e}, scale {scale:.3e}"


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _bits(t):
    return t.view(torch.int32)


def _ceil(a, b):
    return -(-a // b)


def _wide(M, out_features):
    return _ceil(M, 128) * _ceil(out_features, 128) >= 2 * num_cus()


def _wide_rows(out_features, ragged):
    """Smallest batch on the wide side of launch_rows' threshold; ragged: 37 rows short of the last 128-row tile."""
    gy = _ceil(out_features, 128)
    M = 128 * _ceil(2 * num_cus(), gy) - (37 if ragged else 0)
    assert _wide(M, out_features) and not _wide(M - 128, out_features)
    return M


def _narrow_rows(M, out_features):
    Mn = min(4000, M // 2)
    assert not _wide(Mn, out_features)
    return Mn


# ------------------------------------------------------------------------------------------------ 1. wide tiling
@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "full"])
def test_wide_tiling_fwd(data, prec, ragged):
    """JT = 4 forward: gy = ceil(N / 128) = 8, M = 128 * ceil(2 * num_cus() / 8) (- 37) so that ceil(M / 128) * gy >= 2 * num_cus()
    (M = 8192 / 8155 at 256 CUs).  Ragged: N = 1000, K = 70, Sigmoid | Hardtanh split at 333; full: N = 1024, K = 64, ELU.
    fp32 only: the first 4000 rows again through the narrow tiling (32 * gy < 2 * num_cus()), held to the reference and to the wide
    result at the same bound, and bit-equal to it: JT only changes which wave owns which batch rows, every output is the same chain
    of MFMAs over k in either tiling."""
    N, K, act, split = (1000, 70, SIGHT, 333) if ragged else (1024, 64, ELU, 0)
    M = _wide_rows(N, ragged)
    assert ragged == (N % 64 != 0 or K % 64 != 0)
    d = data(M, N, K)
    y = _nan(M, N)
    lin.linear_fwd(d.x, d.w, d.b, y, M, N, K, act, split, precision=prec)
    ref = d.fwd_ref(act, split)
    _check(y, ref, prec, 1e-5, K, "wide fwd")
    if prec == F32:
        Mn = _narrow_rows(M, N)
        yn = _nan(Mn, N)
        lin.linear_fwd(d.x[:Mn], d.w, d.b, yn, Mn, N, K, act, split)
        _check(yn, ref[:Mn], prec, 1e-5, K, "narrow fwd")
        _check(y[:Mn], yn.double(), prec, 1e-5, K, "wide vs narrow fwd")
        assert torch.equal(y[:Mn], yn)


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "full"])
def test_wide_tiling_dgrad(data, prec, ragged):
    """JT = 4 dgrad: out_features = K, gy = ceil(K / 128) = 8, M as in the forward test so that ceil(M / 128) * gy >= 2 * num_cus().
    Ragged: K = 1000, N = 70, dY gated on load through y_gate (Sigmoid | Hardtanh split at 35), act_prev = ELU; full: K = 1024,
    N = 64, ReLU gate, act_prev = ReLU.  fp32 only: the first 4000 rows through the narrow tiling are bit-equal to the wide result, as in the forward test."""
    K, N, gate, prev = (1000, 70, SIGHT, ELU) if ragged else (1024, 64, RELU, RELU)
    M = _wide_rows(K, ragged)
    assert ragged == (N % 64 != 0 or K % 64 != 0)
    d = data(M, N, K, gate, prev)
    dx = _nan(M, K)
    lin.linear_dgrad(d.dy, d.w, dx, M, N, K, y_gate=d.y, gate=gate, gate_split=d.gsplit, x_out=d.x, act_prev=prev,
                     precision=prec)
    ref = d.dx_ref(True, True)
    _check(dx, ref, prec, 2e-5, N, "wide dgrad")
    if prec == F32:
        Mn = _narrow_rows(M, K)
        dxn = _nan(Mn, K)
        lin.linear_dgrad(d.dy[:Mn], d.w, dxn, Mn, N, K, y_gate=d.y[:Mn], gate=gate, gate_split=d.gsplit, x_out=d.x[:Mn],
                         act_prev=prev)
        _check(dxn, ref[:Mn], prec, 2e-5, N, "narrow dgrad")
        _check(dx[:Mn], dxn.double(), prec, 2e-5, N, "wide vs narrow dgrad")
        assert torch.equal(dx[:Mn], dxn)


# ------------------------------------------------------------------------------------------------ 2. empty wgrad splits
@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("N,K", [(500, 784), (512, 768)], ids=["ragged", "full"])
def test_wgrad_empty_trailing_splits(data, prec, gated, N, K):
    """tiles = ceil(N / 128) * ceil(K / 128) = 28 (24), S = ceil(2 * num_cus() / tiles) = 19 (22) at 256 CUs, M = 64 * (S + 1) - 13:
    chunks = S + 1 > S, so every split takes 128 rows and the last S - ceil(chunks / 2) splits are empty (k_begin >= k_end); their
    workgroups must still write zero partials and zero bias partials into the NaN-filled scratch.  K > 128: the bias sum comes
    from the blockIdx.z == 0 workgroups alone."""
    T = 2 * num_cus()
    tiles = _ceil(N, 128) * _ceil(K, 128)
    S = _ceil(T, tiles)
    M = 64 * (S + 1) - 13
    chunks = _ceil(M, 64)
    need = int(lib().vpc_linear_wgrad_scratch(M, N, K))
    assert S < chunks and need == S * (N * K + N)
    rows_per_split = _ceil(chunks, S) * 64
    assert rows_per_split == 128 and (S - 1) * rows_per_split >= M  # at least the last split is empty
    d = data(M, N, K)
    kw = dict(y_gate=d.y, gate=d.gate, gate_split=d.gsplit) if gated else {}
    dw, db, scratch = _nan(N, K), _nan(N), _nan(need)
    lin.linear_wgrad(d.dy, d.x, dw, db, M, N, K, precision=prec, scratch=scratch, **kw)
    dw_ref, db_ref = d.dw_ref(gated)
    _check(dw, dw_ref, prec, 2e-5, 128, "wgrad")
    _check_bias(db, db_ref, prec, "bias grad")
    empty = scratch[:S * N * K].view(S, N * K)[_ceil(M, rows_per_split):]
    assert empty.numel() > 0 and not bool(empty.any()), "an empty split did not write zero partials"
    empty_b = scratch[S * N * K:].view(S, N)[_ceil(M, rows_per_split):]
    assert empty_b.numel() > 0 and not bool(empty_b.any()), "an empty split did not write zero bias partials"
    dw2, db2 = dw.clone(), db.clone()
    scratch.fill_(NAN)
    lin.linear_wgrad(d.dy, d.x, dw2, db2, M, N, K, precision=prec, scratch=scratch, accumulate=True, **kw)
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)


# ------------------------------------------------------------------------------------------------ 3. pitches, alignment
def _ceil4(n):
    return (n + 3) // 4 * 4


# mode -> (row pitch, offset of the base pointer from a 16-byte boundary, in floats)
_MODES = {None: lambda w: (w, 0), "ld+4": lambda w: (w + 4, 0), "ld+3": lambda w: (w + 3, 0),
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


def _run_fwd(d, prec, lay, act=SIGHT, split=None, bias=True):
    M, N, K = d.M, d.N, d.K
    split = N // 2 if split is None else split
    x, w, y = _Buf(M, K, lay.get("x"), d.x), _Buf(N, K, lay.get("w"), d.w), _Buf(M, N, lay.get("y"))
    lin.linear_fwd(x.t, w.t, d.b if bias else None, y.t, M, N, K, act, split, ldx=x.ld, ldy=y.ld, precision=prec)
    _check(y.t, d.fwd_ref(act, split, bias), prec, 1e-5, K, f"fwd {lay}")
    y.assert_padding_untouched("y")
    x.assert_unchanged("x"), w.assert_unchanged("w")


def _run_dgrad(d, prec, lay, gated=True, use_prev=True):
    M, N, K = d.M, d.N, d.K
    dy, w, dx = _Buf(M, N, lay.get("dy"), d.dy), _Buf(N, K, lay.get("w"), d.w), _Buf(M, K, lay.get("dx"))
    yg = _Buf(M, N, lay.get("y_gate"), d.y) if gated else None
    xo = _Buf(M, K, lay.get("x_out"), d.x) if use_prev else None
    lin.linear_dgrad(dy.t, w.t, dx.t, M, N, K, y_gate=yg.t if gated else None, gate=d.gate if gated else NONE,
                     gate_split=d.gsplit, x_out=xo.t if use_prev else None, act_prev=d.prev if use_prev else NONE,
                     lddy=dy.ld, lddx=dx.ld, ldyg=yg.ld if gated else None, ldxo=xo.ld if use_prev else None, precision=prec)
    _check(dx.t, d.dx_ref(gated, use_prev), prec, 2e-5, N, f"dgrad {lay}")
    dx.assert_padding_untouched("dx")
    for b in (dy, w, yg, xo):
        if b is not None:
            b.assert_unchanged("dgrad input")


def _run_wgrad(d, prec, lay, gated=True):
    M, N, K = d.M, d.N, d.K
    dy, x = _Buf(M, N, lay.get("dy"), d.dy), _Buf(M, K, lay.get("x"), d.x)
    yg = _Buf(M, N, lay.get("y_gate"), d.y) if gated else None
    dw, db = _nan(N, K), _nan(N)
    scratch = _nan(int(lib().vpc_linear_wgrad_scratch(M, N, K)))
    lin.linear_wgrad(dy.t, x.t, dw, db, M, N, K, y_gate=yg.t if gated else None, gate=d.gate if gated else NONE,
                     gate_split=d.gsplit, lddy=dy.ld, ldx=x.ld, ldyg=yg.ld if gated else None, precision=prec, scratch=scratch)
    dw_ref, db_ref = d.dw_ref(gated)
    _check(dw, dw_ref, prec, 2e-5, 128, f"wgrad {lay}")
    _check_bias(db, db_ref, prec, f"bias grad {lay}")
    for b in (dy, x, yg):
        if b is not None:
            b.assert_unchanged("wgrad input")


_RUN = {"fwd": _run_fwd, "dgrad": _run_dgrad, "wgrad": _run_wgrad}
_OPERANDS = {"fwd": ["x", "y"], "dgrad": ["dy", "y_gate", "x_out", "dx"], "wgrad": ["dy", "y_gate", "x"]}
_LAYOUTS = [(op, {name: mode}, F32) for op, names in _OPERANDS.items() for name in names for mode in ("ld+4", "ld+3", "off1")]
_LAYOUTS += [(op, {"w": "off1dense"}, F32) for op in ("fwd", "dgrad")]                    # vecA alone off
_LAYOUTS += [("fwd", {"x": "ld+4", "y": "ld+3"}, BF16), ("dgrad", {"dy": "off1", "dx": "ld+4", "x_out": "ld+3"}, BF16),
             ("wgrad", {"dy": "ld+4", "x": "off1", "y_gate": "ld+3"}, BF16)]


@pytest.mark.parametrize("M,N,K", [(300, 28, 130), (300, 30, 132), (256, 128, 64)], ids=["ragged", "ragged-k4", "full"])
@pytest.mark.parametrize("op,lay,prec", _LAYOUTS,
                         ids=[f"{op}-{'-'.join(f'{k}.{v}' for k, v in lay.items())}-{PREC_IDS[p]}" for op, lay, p in _LAYOUTS])
def test_row_pitch_and_alignment(data, M, N, K, op, lay, prec):
    """ceil(300 / 128) * 1 and 2 * 1 workgroups < 2 * num_cus(): the narrow tiling, whose loads and epilogue are the wide one's.
    One operand at a time is a view with a row pitch of width + 4 (16-byte path kept where the width allows it) or width + 3
    (lost), or starts one float past a 16-byte boundary with a pitch that is a multiple of 4: each of vecA (the weights, dense),
    vecB, vecC, vecX is off alone while the others are on.  The padding columns of the output stay NaN, the inputs stay as
    they were.  The gated operations run with y_gate (Sigmoid | Hardtanh) and act_prev = ELU.  At K = 130 no K-wide operand (the
    dense weights included) has a pitch that is a multiple of 4, so there vecA and the K-wide operand's flag are off in every case;
    K = 132 (a multiple of 4, not of 64) and the full shape reach "one flag off, the others on" for them, K = 132 together with
    column tails.  That shape has N = 30, so the forward epilogue's last group of 4 features is cut as well, next to NaN padding."""
    assert not _wide(M, max(N, K))
    _RUN[op](data(M, N, K), prec, lay)


# ------------------------------------------------------------------------------------------------ 4. gated bf16 / bf16x3
@pytest.mark.parametrize("prec", [BF16X3, BF16], ids=PREC_IDS[1:])
@pytest.mark.parametrize("M,N,K,gate,prev", [(37, 20, 128, 0, 1), (300, 28, 128, 2, 1), (2560, 256, 128, 2, 1),
                                             (513, 128, 10, 0, 0), (1000, 130, 70, 1, 3), (64, 128, 128, 1, 1)])
def test_gated_dgrad_wgrad_bf16(data, prec, M, N, K, gate, prev):
    """The shapes of test_notmiwae_gpu.test_linear_dgrad_wgrad in the two bf16 builds: the gate-on-load sweep (y_gate), the
    act_prev epilogue of dgrad and accumulate.  Largest grid 20 * 2 workgroups < 2 * num_cus(): the narrow tiling; S = chunks."""
    assert not _wide(M, max(N, K))
    d = data(M, N, K, gate, prev)
    gated, use_prev = gate != NONE, prev != NONE
    gkw = dict(y_gate=d.y, gate=gate, gate_split=d.gsplit) if gated else {}
    dx = _nan(M, K)
    lin.linear_dgrad(d.dy, d.w, dx, M, N, K, x_out=d.x if use_prev else None, act_prev=prev, precision=prec, **gkw)
    _check(dx, d.dx_ref(gated, use_prev), prec, 2e-5, N, "dgrad")
    dw, db = _nan(N, K), _nan(N)
    scratch = _nan(int(lib().vpc_linear_wgrad_scratch(M, N, K)))
    lin.linear_wgrad(d.dy, d.x, dw, db, M, N, K, precision=prec, scratch=scratch, **gkw)
    dw_ref, db_ref = d.dw_ref(gated)
    _check(dw, dw_ref, prec, 2e-5, 128, "wgrad")
    _check_bias(db, db_ref, prec, "bias grad")
    dw2, db2 = dw.clone(), db.clone()
    lin.linear_wgrad(d.dy, d.x, dw2, db2, M, N, K, precision=prec, accumulate=True, **gkw)
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)


# ------------------------------------------------------------------------------------------------ 5. deferred reduction
# (M, N, K, gated, accumulate, with db)
_DEFERRED = [(37, 20, 128, False, False, True), (300, 128, 14, True, True, True), (None, 500, 784, True, False, True),
             (1000, 130, 70, False, True, True), (129, 5, 3, False, True, False), (1, 128, 128, True, False, True),
             (513, 28, 130, True, False, True), (2560, 256, 64, False, True, True)]


def test_deferred_reduction_is_bit_equal(data):
    """linear_wgrad(dw=None) into a NaN-filled buffer per layer, then ONE wgrad_reduce over eight layers (mixed shapes and
    batch sizes, mixed accumulate flags, one db = None): bit-equal to the per-layer linear_wgrad(dw, db), or to prefill + that
    where accumulate is set; the same bits again through the cached argument arrays.  The (500, 784) layer takes the batch of
    test_wgrad_empty_trailing_splits, S = ceil(2 * num_cus() / 28) < chunks; every other layer has S = chunks."""
    S3 = _ceil(2 * num_cus(), 28)
    specs = [(64 * (S3 + 1) - 13 if M is None else M, N, K, g, a, b) for M, N, K, g, a, b in _DEFERRED]
    assert len(specs) == 8
    layers, want, outs = [], [], []
    gen = torch.Generator(device="cuda").manual_seed(5)
    for M, N, K, gated, acc, with_db in specs:
        d = data(M, N, K)
        kw = dict(y_gate=d.y, gate=d.gate, gate_split=d.gsplit) if gated else {}
        dw1, db1 = _nan(N, K), _nan(N)
        lin.linear_wgrad(d.dy, d.x, dw1, db1, M, N, K, **kw)
        _check(dw1, d.dw_ref(gated)[0], F32, 2e-5, 128, f"wgrad {(M, N, K)}")
        pre_w = torch.randn(N, K, device="cuda", generator=gen) if acc else _nan(N, K)
        pre_b = torch.randn(N, device="cuda", generator=gen) if acc else _nan(N)
        scratch = _nan(int(lib().vpc_linear_wgrad_scratch(M, N, K)))
        lin.linear_wgrad(d.dy, d.x, None, None, M, N, K, scratch=scratch, **kw)
        dw, db = pre_w.clone(), pre_b.clone()
        layers.append((scratch, M, N, K, dw, db if with_db else None, acc))
        want.append((pre_w + dw1 if acc else dw1, (pre_b + db1 if acc else db1) if with_db else pre_b))
        outs.append((dw, db, pre_w, pre_b))

    def compare(tag):
        for (dw, db, _, _), (w_ref, b_ref), spec in zip(outs, want, specs):
            assert torch.equal(_bits(dw), _bits(w_ref)), f"{tag}: dw of layer {spec}"
            assert torch.equal(_bits(db), _bits(b_ref)), f"{tag}: db of layer {spec}"  # db = None: left as it was

    lin.wgrad_reduce(layers)
    compare("one launch")
    cache = {}
    for tag in ("cache built", "cache reused"):
        for dw, db, pre_w, pre_b in outs:
            dw.copy_(pre_w), db.copy_(pre_b)
        lin.wgrad_reduce(layers if tag == "cache built" else None, cache=cache)
        compare(tag)
    assert "args" in cache
    with pytest.raises(VpcError):
        lin.wgrad_reduce(layers + layers[:1])
    with pytest.raises(VpcError):
        lin.wgrad_reduce([])


# ------------------------------------------------------------------------------------------------ 6. small edges (fp32)
@pytest.mark.parametrize("M", [1, 31, 32, 33, 127, 128, 129])
@pytest.mark.parametrize("N,K", [(20, 14), (128, 128)], ids=["ragged", "full"])
def test_rows_at_tile_edges(data, M, N, K):
    """M at and around the 32-row tile of the narrow tiling (1 .. 5 workgroups < 2 * num_cus()) and the 128-row tile size,
    forward, dgrad and wgrad (chunks = 1 .. 3, S = chunks), gated and ungated."""
    assert not _wide(M, max(N, K))
    d = data(M, N, K)
    _run_fwd(d, F32, {})
    _run_fwd(d, F32, {}, act=ELU, bias=False)
    _run_dgrad(d, F32, {})
    _run_dgrad(d, F32, {}, gated=False, use_prev=False)
    _run_wgrad(d, F32, {})
    _run_wgrad(d, F32, {}, gated=False)


@pytest.mark.parametrize("M,N,K", [(77, 28, 50), (129, 128, 64)], ids=["ragged", "full"])
@pytest.mark.parametrize("where", ["0", "N"])
def test_activation_split_at_the_ends(data, where, M, N, K):
    """ACT_SIGMOID_HARDTANH with the split at 0 (all Hardtanh) and at N (all Sigmoid), as output activation and as gate.
    Narrow tiling (<= 2 workgroups < 2 * num_cus())."""
    assert not _wide(M, max(N, K))
    split = 0 if where == "0" else N
    d = data(M, N, K, SIGHT, ELU, split)
    _run_fwd(d, F32, {}, split=split)
    _run_dgrad(d, F32, {})
    _run_wgrad(d, F32, {})


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_image_width_contraction(data, bias):
    """K = 784 (the EDDI-mnist width: 12 full 64-wide chunks and one of 16) with N = 200, M = 300: forward contracts over 784,
    dgrad over 200 - both over 128 and no multiple of 64.  3 * 2 and 3 * 7 workgroups < 2 * num_cus(): the narrow tiling."""
    M, N, K = 300, 200, 784
    assert not _wide(M, max(N, K))
    d = data(M, N, K)
    _run_fwd(d, F32, {}, bias=bias)
    _run_dgrad(d, F32, {}, gated=bias, use_prev=bias)
