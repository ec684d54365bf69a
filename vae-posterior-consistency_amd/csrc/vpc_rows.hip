// Few-row dense layers: the same three operations as vpc_gemm.hip (forward, data gradient, weight gradient of nn.Linear +
// activation: reference src/models/VAE.py:1878-1900 for the flow models' eight layers at hid_dim 500, :2343-2363 in general)
// for M <= 128 rows and N, K <= 1024, fp32, where the 128-feature x 32-row tiling of linear_kernel leaves a 500-wide layer on
// 16 of 256 compute units and the weight gradient goes through sixteen copies of the model.
//
//   rows_fwd_kernel   Y[m][n]  = act( sum_k X[m][k] W[n][k] + b[n] )
//   rows_bwd_kernel   dW[n][k] (+)= sum_m dY~[m][n] X[m][k],  db[n] (+)= sum_m dY~[m][n]      (workgroups [0, wg_blocks))
//                     dX[m][k] = ( sum_n dY~[m][n] W[n][k] ) * act_prev'(Xout[m][k])           (the remaining workgroups)
//   dY~ = dY * gate'(Y) formed on load when y_gate is given.
//   rows_fwd_multi_kernel / rows_bwd_multi_kernel   the same bodies (vpc_rows_{fwd,bwd}_body.h) for G members of an ensemble: a
//                     member axis on the grid, member g's operands = member 0's + g * stride (include/vpc.h, vpc_rows_*_multi)
//
// The split is over output FEATURES.  The MFMA is v_mfma_f32_16x16x4_f32 used "transposed" as everywhere in this library: the
// D tile is [feature 4q+j][row or column c].  No operand goes through LDS: every fragment is read from global memory (L2: the
// whole model is 4.3 MB) in the shape the MFMA takes it, a group of chunks requested ahead of its MFMAs.
//   forward / data gradient   a workgroup owns 16 output features x 32 rows (two 16-row tiles).  Its waves split the
//                     contraction in 16-wide chunks, wave w taking chunks w, w + 8, ..; a chunk's weight fragment is loaded once
//                     and feeds both row tiles.  The waves' partial tiles meet in LDS and are summed in wave order.
//   weight gradient   a wave owns 16 features x 64 columns of dW and runs the whole contraction over the M <= 128 rows itself:
//                     four accumulators, column 64 g + 4 c + e on lane c of accumulator e, so X is read and dW written in
//                     16-byte pieces.  Written (or added) straight to dw / db: no partials, no reduction launch.
// No atomics, no communication between workgroups, one fixed summation order: results are bitwise reproducible.  Rows, features
// and contraction columns outside the matrices are read as zero (address 0 of the array, value replaced) and never stored.
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_act.h"

namespace vpc {

constexpr int ROWS_MAX_M = 128;    // rows (the contraction of the weight gradient lives in 32 registers per lane)
constexpr int ROWS_MAX_F = 1024;   // features on either side of a layer
constexpr int ROWS_RT = 2;         // 16-row tiles of a forward / data-gradient workgroup (32 rows: at most 64 x 4 workgroups)
constexpr int ROWS_WAVES = 8;      // waves that split a slab's contraction
constexpr int ROWS_WG_UNITS = 4;   // weight-gradient units per workgroup: waves 0 .. 3, one per SIMD (a unit is MFMA-bound)
constexpr int ROWS_GROUP = 4;      // chunks of a wave whose fragments are requested together (2 where the gate doubles the loads)
constexpr int ROWS_WG_AHEAD = 4;   // 16-row blocks of X a weight-gradient wave requests ahead of its MFMAs

struct RowsFwdArgs {
    const float* x; long ldx;
    const float* w; const float* bias;
    float* y; long ldy;
    int M, N, K, act, split;
    int vecY;  // 16-byte stores of y
};

struct RowsBwdArgs {
    const float* dy; long lddy;
    const float* yg; long ldyg; int gate, gate_split;
    const float* w;
    const float* x; long ldx;
    const float* xo; long ldxo; int act_prev;
    float* dx; long lddx;
    float* dw; float* db;
    int M, N, K, accumulate;
    int wg_units, wg_blocks;     // weight-gradient units and the workgroups that hold them (0: dw == NULL)
    int vecDw, vecDx, vecXo;     // 16-byte access to dw / dx / x_out
};

// base[off .. off + 3], of which the first nv (<= 0: none) lie inside the matrix.  VEC: base is 16-byte aligned, off and the
// matrix's width are multiples of 4, so the group is inside or outside as a whole.  The load is unconditional (an outside
// element reads element 0 of the array) and its value is and-ed with an opaque mask: hipcc turns `ok ? loaded : 0` into an
// exec-masked branch around the load whose join waits for EVERY load in flight (vpc_device.h: opaque_mask), which made each
// chunk of the first build of these kernels a full memory round trip.
template <bool VEC>
__device__ __forceinline__ f32x4 rows_ld4(const float* __restrict__ base, long off, int nv) {
    f32x4 v;
    if (VEC) {
        const bool ok = nv >= 4;
        v = and4(*reinterpret_cast<const f32x4*>(base + (ok ? off : 0)), opaque_mask(ok));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = j < nv;
            v[j] = __uint_as_float(__float_as_uint(base[ok ? off + j : 0]) & opaque_mask(ok));
        }
    }
    return v;
}
// base[(r0 + j) * ld + col], j = 0 .. 3: one column of four consecutive rows (rows < rlim, col_ok)
__device__ __forceinline__ f32x4 rows_ld4_col(const float* __restrict__ base, long ld, int r0, int rlim, int col, bool col_ok) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool ok = col_ok && r0 + j < rlim;
        v[j] = __uint_as_float(__float_as_uint(base[ok ? (long)(r0 + j) * ld + col : 0]) & opaque_mask(ok));
    }
    return v;
}

typedef f32x4 (*rows_red_t)[ROWS_RT][64];
// the partial tiles of row tile rt, summed in wave order
__device__ __forceinline__ f32x4 rows_sum(rows_red_t red, int nw, int rt, int lane) {
    f32x4 s = red[0][rt][lane];
    for (int w = 1; w < nw; ++w) s += red[w][rt][lane];
    return s;
}

// The contraction of one slab (16 output features x NRT row tiles) over this wave's chunks wave, wave + 8, ..: lda(ch) is
// the chunk's A fragment (weights), ldb(ch, rt) row tile rt's B fragment; a chunk past the end loads zeros.  The chunks go
// in groups of ROWS_GROUP whose fragments are ALL requested before the group's first MFMA, so a 500-wide contraction over 8
// waves is one round of loads; the MFMAs of a k-step alternate between the row tiles' independent accumulators.
template <int NRT, int GROUP, class LoadA, class LoadB>
__device__ __forceinline__ void rows_slab_group(int c0, LoadA lda, LoadB ldb, f32x4 (&acc)[ROWS_RT]) {
    f32x4 af[GROUP], bf[GROUP][NRT];
#pragma unroll
    for (int g = 0; g < GROUP; ++g) {
        af[g] = lda(c0 + ROWS_WAVES * g);
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) bf[g][rt] = ldb(c0 + ROWS_WAVES * g, rt);
    }
    // every request above every MFMA (left alone hipcc interleaves them chunk by chunk to save registers: four round
    // trips); VALU and SALU may cross, so the masking and gating of a fragment wait for that fragment only
    __builtin_amdgcn_sched_barrier(0x0006);
#pragma unroll
    for (int g = 0; g < GROUP; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) acc[rt] = VPC_MFMA(af[g][j], bf[g][rt][j], acc[rt]);
}
template <int NRT, int GROUP, class LoadA, class LoadB>
__device__ __forceinline__ void rows_slab_chunks(int nchunk, int wave, LoadA lda, LoadB ldb, f32x4 (&acc)[ROWS_RT]) {
    int c0 = wave;
    for (; c0 + ROWS_WAVES * (GROUP - 1) < nchunk; c0 += ROWS_WAVES * GROUP) rows_slab_group<NRT, GROUP>(c0, lda, ldb, acc);
    for (; c0 < nchunk; c0 += ROWS_WAVES) rows_slab_group<NRT, 1>(c0, lda, ldb, acc);  // (K = 10, 24: one chunk, not a group of zeros)
}
// (a per-MFMA test on the number of live row tiles became a branch forest with a full wait in front: one loop per count)
template <int GROUP, class LoadA, class LoadB>
__device__ __forceinline__ void rows_slab(int nrt, int nchunk, int wave, LoadA lda, LoadB ldb, f32x4 (&acc)[ROWS_RT]) {
    if (nrt <= 1) rows_slab_chunks<1, GROUP>(nchunk, wave, lda, ldb, acc);
    else rows_slab_chunks<ROWS_RT, GROUP>(nchunk, wave, lda, ldb, acc);
}

template <bool VEC>
__global__ __launch_bounds__(64 * ROWS_WAVES) void rows_fwd_kernel(RowsFwdArgs a) {
#define ROWS_BX blockIdx.x
#define ROWS_BY blockIdx.y
#include "vpc_rows_fwd_body.h"
#undef ROWS_BX
#undef ROWS_BY
}

// The MFMAs of one weight-gradient unit over NMB 16-row blocks of the batch (blocks past M multiply zeros).  The X fragments
// run ROWS_WG_AHEAD blocks ahead of the MFMAs that take them; the sched_barrier keeps hipcc from requesting all 32 at once
// (128 registers on top of the 32 of dY~: the first such build spilled).
template <bool VK, int NMB>
__device__ __forceinline__ void rows_wgrad_mm(const RowsBwdArgs& a, const f32x4 (&af)[ROWS_MAX_M / 16], int col, int q,
                                              f32x4 (&acc)[4]) {
    constexpr int AHEAD = VK ? ROWS_WG_AHEAD : ROWS_WG_AHEAD / 2;  // (the scalar path holds an address and a mask per float)
    f32x4 xf[NMB][4];
    auto load = [&](int mb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = 16 * mb + 4 * q + j;
            xf[mb][j] = rows_ld4<VK>(a.x, (long)m * a.ldx + col, m < a.M ? a.K - col : 0);
        }
    };
#pragma unroll
    for (int mb = 0; mb < AHEAD && mb < NMB; ++mb) load(mb);
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb) {
        if (mb + AHEAD < NMB) load(mb + AHEAD);
        __builtin_amdgcn_sched_barrier(0x0006);  // (VALU / SALU may cross: a fragment's masking waits for that fragment only)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = VPC_MFMA(af[mb][j], xf[mb][j][e], acc[e]);
    }
}

// One weight-gradient unit: dW[16 slab + 4 q + r][64 grp + 4 c + e] = accumulator e, register r of lane (c, q).
// k-step (mb, j) contracts the rows m = 16 mb + 4 q' + j, q' = 0 .. 3: A = dY~[m][16 slab + c], B = X[m][64 grp + 4 c + e].
template <bool VK>
__device__ __forceinline__ void rows_wgrad_unit(const RowsBwdArgs& a, int slab, int grp, int c, int q) {
    const int n = 16 * slab + c;
    const bool n_ok = n < a.N;
    const int nmb = (a.M + 15) / 16;
    f32x4 af[ROWS_MAX_M / 16];
#pragma unroll
    for (int mb = 0; mb < ROWS_MAX_M / 16; ++mb) af[mb] = rows_ld4_col(a.dy, a.lddy, 16 * mb + 4 * q, a.M, n, n_ok);
    act_dispatch(a.gate, [&](auto gc) {
        constexpr int G = decltype(gc)::value;
        if (G == ACT_NONE) return;
#pragma unroll
        for (int mb = 0; mb < ROWS_MAX_M / 16; ++mb) {
            const f32x4 y = rows_ld4_col(a.yg, a.ldyg, 16 * mb + 4 * q, a.M, n, n_ok);
#pragma unroll
            for (int j = 0; j < 4; ++j) af[mb][j] *= act_grad<G>(y[j], n >= a.gate_split);
        }
    });
    if (grp == 0 && a.db) {  // the bias gradient: this lane's rows in order, then the four row quarters as (0 + 1) + (2 + 3)
        float s = 0.f;
#pragma unroll
        for (int mb = 0; mb < ROWS_MAX_M / 16; ++mb)
#pragma unroll
            for (int j = 0; j < 4; ++j) s += af[mb][j];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (q == 0 && n_ok) a.db[n] = a.accumulate ? a.db[n] + s : s;
    }
    const int col = 64 * grp + 4 * c;
    f32x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
    if (nmb <= 2) rows_wgrad_mm<VK, 2>(a, af, col, q, acc);
    else if (nmb <= 4) rows_wgrad_mm<VK, 4>(a, af, col, q, acc);
    else rows_wgrad_mm<VK, ROWS_MAX_M / 16>(a, af, col, q, acc);
    if (col >= a.K) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int f = 16 * slab + 4 * q + r;
        if (f >= a.N) continue;
        float* pw = a.dw + (long)f * a.K + col;
        f32x4 v = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
        if (a.vecDw && col + 3 < a.K) {
            if (a.accumulate) v += *reinterpret_cast<const f32x4*>(pw);
            *reinterpret_cast<f32x4*>(pw) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (col + e < a.K) pw[e] = a.accumulate ? pw[e] + v[e] : v[e];
        }
    }
}

// VN: 16-byte loads of dy / y_gate along N (data gradient).  VK: 16-byte loads of x along K (weight gradient).
template <bool VN, bool VK>
__global__ __launch_bounds__(64 * ROWS_WAVES) void rows_bwd_kernel(RowsBwdArgs a) {
#define ROWS_BX blockIdx.x
#include "vpc_rows_bwd_body.h"
#undef ROWS_BX
}

// ================================================================================================ the ensemble forms
// G members in one launch (include/vpc.h, vpc_rows_fwd_multi / vpc_rows_bwd_multi): base = member 0's arguments, member g's
// arrays lie g * stride floats behind them.  A workgroup runs the stand-alone body on its member's arguments, so a member's
// bits do not depend on G, on the order or on where its workgroups run.
struct RowsFwdMultiArgs {
    RowsFwdArgs base;
    long sx, sw, sy;   // floats between two members' x / (w, bias) / y
    int G, order, nx;  // nx: 16-feature slabs of the layer (order 1 folds (slab, row block) into blockIdx.x)
};
struct RowsBwdMultiArgs {
    RowsBwdArgs base;
    long sdy, syg, sx, sxo, sdx, sw;  // sw: w, dw and db (the parameter and the gradient stack share their row pitch)
    int G, order;
};
// The member of this workgroup and its index `blk` among the member's workgroups.  order 0: the member is the grid's last axis
// (member-major: a member's workgroups are dealt over all 8 XCDs).  order 1: grid.x = 8 x the member's workgroups,
// blk = x / 8, member = 8 y + x % 8 - workgroups go round-robin over the XCDs by their linear id, so all workgroups of a member
// sit on one XCD and its weights are re-read through ONE L2 (false: a surplus workgroup of the last member group).
__device__ __forceinline__ bool rows_block_member(int G, int order, unsigned last_axis, unsigned& blk, unsigned& mem) {
    if (order == 0) {
        blk = blockIdx.x;
        mem = last_axis;
        return true;
    }
    blk = blockIdx.x >> 3;
    mem = 8 * blockIdx.y + (blockIdx.x & 7);
    return mem < (unsigned)G;
}

template <bool VEC>
__global__ __launch_bounds__(64 * ROWS_WAVES) void rows_fwd_multi_kernel(RowsFwdMultiArgs ma) {
    unsigned bx, by = blockIdx.y, mem;
    if (!rows_block_member(ma.G, ma.order, blockIdx.z, bx, mem)) return;
    if (ma.order != 0) {
        by = bx / (unsigned)ma.nx;
        bx -= by * (unsigned)ma.nx;
    }
    RowsFwdArgs a = ma.base;  // (uniform: scalar arithmetic)
    a.x += mem * ma.sx;
    a.w += mem * ma.sw;
    if (a.bias) a.bias += mem * ma.sw;
    a.y += mem * ma.sy;
#define ROWS_BX bx
#define ROWS_BY by
#include "vpc_rows_fwd_body.h"
#undef ROWS_BX
#undef ROWS_BY
}

template <bool VN, bool VK>
__global__ __launch_bounds__(64 * ROWS_WAVES) void rows_bwd_multi_kernel(RowsBwdMultiArgs ma) {
    unsigned bx, mem;
    if (!rows_block_member(ma.G, ma.order, blockIdx.y, bx, mem)) return;
    RowsBwdArgs a = ma.base;
    a.dy += mem * ma.sdy;
    if (a.yg) a.yg += mem * ma.syg;
    if (a.w) a.w += mem * ma.sw;
    if (a.x) a.x += mem * ma.sx;
    if (a.xo) a.xo += mem * ma.sxo;
    if (a.dx) a.dx += mem * ma.sdx;
    if (a.dw) a.dw += mem * ma.sw;
    if (a.db) a.db += mem * ma.sw;
#define ROWS_BX bx
#include "vpc_rows_bwd_body.h"
#undef ROWS_BX
}

static bool rows_vec(const void* p, long ld, int width) { return aligned16(p) && (ld % 4) == 0 && (width % 4) == 0; }

// ---- what the stand-alone entry and the ensemble entry share on the host: argument checks, the kernel's record, the grid of
// ONE member and the 16-byte / scalar choice (taken on member 0's operands)
static int rows_fwd_setup(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, long M, int N, int K,
                          int act, int act_split, RowsFwdArgs& a, dim3& grid, bool& vec) {
    if (!x || !w || !y || M < 1 || N < 1 || K < 1 || ldx < K || ldy < N) return VPC_ERR_ARG;
    if (act < ACT_NONE || act > ACT_RELU) return VPC_ERR_ARG;
    if (M > ROWS_MAX_M || N > ROWS_MAX_F || K > ROWS_MAX_F) return VPC_ERR_SHAPE;
    a = RowsFwdArgs{};
    a.x = x; a.ldx = ldx; a.w = w; a.bias = bias; a.y = y; a.ldy = ldy;
    a.M = (int)M; a.N = N; a.K = K; a.act = act; a.split = act == ACT_SIGMOID_HARDTANH ? act_split : N;
    a.vecY = aligned16(y) && (ldy % 4) == 0;
    grid = dim3((unsigned)((N + 15) / 16), (unsigned)((M + 16 * ROWS_RT - 1) / (16 * ROWS_RT)));
    vec = rows_vec(x, ldx, K) && rows_vec(w, K, K);
    return VPC_OK;
}

static int rows_bwd_setup(const float* dy, long lddy, const float* y_gate, long ldyg, int gate, int gate_split, const float* w,
                          const float* x, long ldx, const float* x_out, long ldxo, int act_prev, float* dx, long lddx,
                          float* dw, float* db, long M, int N, int K, int accumulate, RowsBwdArgs& a, unsigned& blocks,
                          bool& vn, bool& vk) {
    if (!dy || M < 1 || N < 1 || K < 1 || lddy < N || (!dw && !dx)) return VPC_ERR_ARG;
    if ((dw && (!x || ldx < K)) || (dx && (!w || lddx < K))) return VPC_ERR_ARG;
    if ((y_gate && ldyg < N) || (dx && x_out && ldxo < K)) return VPC_ERR_ARG;
    if (gate < ACT_NONE || gate > ACT_RELU || act_prev < ACT_NONE || act_prev > ACT_RELU) return VPC_ERR_ARG;
    if (M > ROWS_MAX_M || N > ROWS_MAX_F || K > ROWS_MAX_F) return VPC_ERR_SHAPE;
    a = RowsBwdArgs{};
    a.dy = dy; a.lddy = lddy; a.yg = y_gate; a.ldyg = ldyg;
    a.gate = y_gate ? gate : ACT_NONE;  // (no outputs to gate with: dy is the pre-activation gradient)
    a.gate_split = gate == ACT_SIGMOID_HARDTANH ? gate_split : N;
    a.w = w; a.x = x; a.ldx = ldx; a.xo = dx ? x_out : nullptr; a.ldxo = ldxo; a.act_prev = act_prev;
    a.dx = dx; a.lddx = lddx; a.dw = dw; a.db = dw ? db : nullptr;
    a.M = (int)M; a.N = N; a.K = K; a.accumulate = accumulate != 0;
    a.wg_units = dw ? ((N + 15) / 16) * ((K + 63) / 64) : 0;
    a.wg_blocks = (a.wg_units + ROWS_WG_UNITS - 1) / ROWS_WG_UNITS;
    a.vecDw = dw && aligned16(dw) && (K % 4) == 0;
    a.vecDx = dx && aligned16(dx) && (lddx % 4) == 0;
    a.vecXo = a.xo && aligned16(a.xo) && (ldxo % 4) == 0;
    const int dg_blocks = dx ? ((K + 15) / 16) * (((int)M + 16 * ROWS_RT - 1) / (16 * ROWS_RT)) : 0;
    vn = rows_vec(dy, lddy, N) && (!y_gate || rows_vec(y_gate, ldyg, N));
    vk = !dw || rows_vec(x, ldx, K);
    blocks = (unsigned)(a.wg_blocks + dg_blocks);
    return VPC_OK;
}

// a member stride of the ensemble entries: at least the member's slice ((rows - 1) ld + width floats) and a multiple of 4
// floats, so that the 16-byte / scalar choice taken on member 0's operands holds for every member
static bool rows_stride_ok(long stride, long rows, long ld, long width) {
    return stride >= (rows - 1) * ld + width && (stride % 4) == 0;
}
static bool rows_multi_ok(int G, int order) { return G >= 1 && G <= VPC_ROWS_MULTI_MAX_MEMBERS && (order == 0 || order == 1); }
// the grid of G members with `per` workgroups each, in the order of rows_block_member; false: past the launch limits
static bool rows_multi_grid(dim3 one, int G, int order, bool member_on_z, dim3& grid) {
    const unsigned long per = (unsigned long)one.x * one.y;
    if (order == 0) grid = member_on_z ? dim3(one.x, one.y, (unsigned)G) : dim3(one.x, (unsigned)G);
    else grid = dim3((unsigned)(8 * per), (unsigned)((G + 7) / 8));
    return 8 * per <= 0x7fffffffUL && grid.y <= 65535u && grid.z <= 65535u;
}

}  // namespace vpc

using namespace vpc;

extern "C" {

int vpc_rows_max_rows(void) { return ROWS_MAX_M; }

int vpc_rows_fwd(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, long M, int N, int K,
                 int act, int act_split, void* stream) {
    RowsFwdArgs a;
    dim3 grid;
    bool vec;
    const int rc = rows_fwd_setup(x, ldx, w, bias, y, ldy, M, N, K, act, act_split, a, grid, vec);
    if (rc != VPC_OK) return rc;
    const dim3 block(64 * ROWS_WAVES);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(rows_fwd_kernel<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(rows_fwd_kernel<false>, grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_rows_bwd(const float* dy, long lddy, const float* y_gate, long ldyg, int gate, int gate_split, const float* w,
                 const float* x, long ldx, const float* x_out, long ldxo, int act_prev, float* dx, long lddx, float* dw,
                 float* db, long M, int N, int K, int accumulate, void* stream) {
    RowsBwdArgs a;
    unsigned blocks;
    bool vn, vk;
    const int rc = rows_bwd_setup(dy, lddy, y_gate, ldyg, gate, gate_split, w, x, ldx, x_out, ldxo, act_prev, dx, lddx, dw, db,
                                  M, N, K, accumulate, a, blocks, vn, vk);
    if (rc != VPC_OK) return rc;
    const dim3 grid(blocks), block(64 * ROWS_WAVES);
    hipStream_t st = (hipStream_t)stream;
    if (vn && vk) hipLaunchKernelGGL((rows_bwd_kernel<true, true>), grid, block, 0, st, a);
    else if (vn) hipLaunchKernelGGL((rows_bwd_kernel<true, false>), grid, block, 0, st, a);
    else if (vk) hipLaunchKernelGGL((rows_bwd_kernel<false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((rows_bwd_kernel<false, false>), grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_rows_fwd_multi(const float* x, long ldx, long x_stride, const float* w, const float* bias, long wb_stride, float* y,
                       long ldy, long y_stride, int G, long M, int N, int K, int act, int act_split, int order, void* stream) {
    RowsFwdMultiArgs ma{};
    dim3 one, grid;
    bool vec;
    const int rc = rows_fwd_setup(x, ldx, w, bias, y, ldy, M, N, K, act, act_split, ma.base, one, vec);
    if (rc != VPC_OK) return rc;
    if (!rows_multi_ok(G, order) || !rows_stride_ok(x_stride, M, ldx, K) || !rows_stride_ok(wb_stride, N, K, K) ||
        !rows_stride_ok(y_stride, M, ldy, N))
        return VPC_ERR_ARG;
    if (!rows_multi_grid(one, G, order, true, grid)) return VPC_ERR_SHAPE;
    ma.sx = x_stride; ma.sw = wb_stride; ma.sy = y_stride; ma.G = G; ma.order = order; ma.nx = (int)one.x;
    const dim3 block(64 * ROWS_WAVES);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(rows_fwd_multi_kernel<true>, grid, block, 0, st, ma);
    else hipLaunchKernelGGL(rows_fwd_multi_kernel<false>, grid, block, 0, st, ma);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_rows_bwd_multi(const float* dy, long lddy, long dy_stride, const float* y_gate, long ldyg, long yg_stride, int gate,
                       int gate_split, const float* w, const float* x, long ldx, long x_stride, const float* x_out, long ldxo,
                       long xo_stride, int act_prev, float* dx, long lddx, long dx_stride, float* dw, float* db, long wb_stride,
                       int G, long M, int N, int K, int accumulate, int order, void* stream) {
    RowsBwdMultiArgs ma{};
    unsigned blocks;
    bool vn, vk;
    const int rc = rows_bwd_setup(dy, lddy, y_gate, ldyg, gate, gate_split, w, x, ldx, x_out, ldxo, act_prev, dx, lddx, dw, db,
                                  M, N, K, accumulate, ma.base, blocks, vn, vk);
    if (rc != VPC_OK) return rc;
    if (!rows_multi_ok(G, order) || !rows_stride_ok(dy_stride, M, lddy, N) || (y_gate && !rows_stride_ok(yg_stride, M, ldyg, N)) ||
        ((dw || dx) && !rows_stride_ok(wb_stride, N, K, K)) || (dw && !rows_stride_ok(x_stride, M, ldx, K)) ||
        (dx && x_out && !rows_stride_ok(xo_stride, M, ldxo, K)) || (dx && !rows_stride_ok(dx_stride, M, lddx, K)))
        return VPC_ERR_ARG;
    dim3 grid;
    if (!rows_multi_grid(dim3(blocks), G, order, false, grid)) return VPC_ERR_SHAPE;
    ma.sdy = dy_stride; ma.syg = yg_stride; ma.sx = x_stride; ma.sxo = xo_stride; ma.sdx = dx_stride; ma.sw = wb_stride;
    ma.G = G; ma.order = order;
    const dim3 block(64 * ROWS_WAVES);
    hipStream_t st = (hipStream_t)stream;
    if (vn && vk) hipLaunchKernelGGL((rows_bwd_multi_kernel<true, true>), grid, block, 0, st, ma);
    else if (vn) hipLaunchKernelGGL((rows_bwd_multi_kernel<true, false>), grid, block, 0, st, ma);
    else if (vk) hipLaunchKernelGGL((rows_bwd_multi_kernel<false, true>), grid, block, 0, st, ma);
    else hipLaunchKernelGGL((rows_bwd_multi_kernel<false, false>), grid, block, 0, st, ma);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
