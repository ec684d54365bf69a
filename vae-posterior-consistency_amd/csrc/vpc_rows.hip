// Few-row dense layers: the same three operations as vpc_gemm.hip (forward, data gradient, weight gradient of nn.Linear +
// activation: reference src/models/VAE.py:1878-1900 for the flow models' eight layers at hid_dim 500, :2343-2363 in general)
// for M <= 128 rows and N, K <= 1024, fp32, where the 128-feature x 32-row tiling of linear_kernel leaves a 500-wide layer on
// 16 of 256 compute units and the weight gradient goes through sixteen copies of the model.
//
//   rows_fwd_kernel   Y[m][n]  = act( sum_k X[m][k] W[n][k] + b[n] )
//   rows_bwd_kernel   dW[n][k] (+)= sum_m dY~[m][n] X[m][k],  db[n] (+)= sum_m dY~[m][n]      (workgroups [0, wg_blocks))
//                     dX[m][k] = ( sum_n dY~[m][n] W[n][k] ) * act_prev'(Xout[m][k])           (the remaining workgroups)
//   dY~ = dY * gate'(Y) formed on load when y_gate is given.
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
    __shared__ f32x4 red[ROWS_WAVES][ROWS_RT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int f0 = blockIdx.x * 16, m0 = blockIdx.y * 16 * ROWS_RT;
    const int nrt = min(ROWS_RT, (a.M - m0 + 15) / 16);
    const int nchunk = (a.K + 15) / 16;
    const int fw = f0 + c;
    const bool fw_ok = fw < a.N;
    f32x4 acc[ROWS_RT];
#pragma unroll
    for (int rt = 0; rt < ROWS_RT; ++rt) acc[rt] = zero4();
    // lane (c, q): A = W[f0 + c][16 ch + 4 q + j], B = X[m0 + 16 rt + c][16 ch + 4 q + j] in k-step j of chunk ch
    rows_slab<ROWS_GROUP>(nrt, nchunk, wave,
              [&](int ch) {
                  const int k = 16 * ch + 4 * q;
                  return rows_ld4<VEC>(a.w, (long)fw * a.K + k, fw_ok ? a.K - k : 0);
              },
              [&](int ch, int rt) {
                  const int k = 16 * ch + 4 * q, row = m0 + 16 * rt + c;
                  return rows_ld4<VEC>(a.x, (long)row * a.ldx + k, row < a.M ? a.K - k : 0);
              }, acc);
#pragma unroll
    for (int rt = 0; rt < ROWS_RT; ++rt) red[wave][rt][lane] = acc[rt];
    __syncthreads();
    // waves 0, 1: the epilogue of row tile `wave`.  s[e] = Y[m0 + 16 wave + c][f0 + 4 q + e] before bias and activation
    if (wave >= nrt) return;
    const f32x4 s = rows_sum(red, min(ROWS_WAVES, nchunk), wave, lane);
    const int f = f0 + 4 * q, row = m0 + 16 * wave + c;
    if (f >= a.N || row >= a.M) return;
    f32x4 bv = zero4();
    if (a.bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (f + e < a.N) bv[e] = a.bias[f + e];
    }
    act_dispatch(a.act, [&](auto actc) {
        constexpr int ACT = decltype(actc)::value;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = act_fwd<ACT>(s[e] + bv[e], f + e >= a.split);
        float* py = a.y + (long)row * a.ldy + f;
        if (a.vecY && f + 3 < a.N) {
            *reinterpret_cast<f32x4*>(py) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (f + e < a.N) py[e] = v[e];
        }
    });
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
    __shared__ f32x4 red[ROWS_WAVES][ROWS_RT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    if ((int)blockIdx.x < a.wg_blocks) {  // ---- weight gradient: unit = (slab of 16 features, group of 64 columns) per wave
        const int unit = ROWS_WG_UNITS * blockIdx.x + wave;
        if (wave >= ROWS_WG_UNITS || unit >= a.wg_units) return;
        const int ng = (a.K + 63) / 64;
        rows_wgrad_unit<VK>(a, unit / ng, unit % ng, c, q);
        return;
    }
    // ---- data gradient: slab of 16 input features x 32 rows, the waves split the contraction over N
    const int b = blockIdx.x - a.wg_blocks, nsk = (a.K + 15) / 16;
    const int kf0 = 16 * (b % nsk), m0 = 16 * ROWS_RT * (b / nsk);
    const int nrt = min(ROWS_RT, (a.M - m0 + 15) / 16);
    const int nchunk = (a.N + 15) / 16;
    const int kf = kf0 + c;
    const bool kf_ok = kf < a.K;
    f32x4 acc[ROWS_RT];
#pragma unroll
    for (int rt = 0; rt < ROWS_RT; ++rt) acc[rt] = zero4();
    // lane (c, q): A = W[16 ch + 4 q + j][kf0 + c], B = dY~[m0 + 16 rt + c][16 ch + 4 q + j] in k-step j of chunk ch
    act_dispatch(a.gate, [&](auto gc) {
        constexpr int G = decltype(gc)::value;
        rows_slab<(G == ACT_NONE ? ROWS_GROUP : ROWS_GROUP / 2)>(nrt, nchunk, wave,
                  [&](int ch) { return rows_ld4_col(a.w, a.K, 16 * ch + 4 * q, a.N, kf, kf_ok); },
                  [&](int ch, int rt) {
                      const int n = 16 * ch + 4 * q, row = m0 + 16 * rt + c;
                      const int nv = row < a.M ? a.N - n : 0;
                      f32x4 d = rows_ld4<VN>(a.dy, (long)row * a.lddy + n, nv);
                      if (G != ACT_NONE) {
                          const f32x4 y = rows_ld4<VN>(a.yg, (long)row * a.ldyg + n, nv);
#pragma unroll
                          for (int j = 0; j < 4; ++j) d[j] *= act_grad<G>(y[j], n + j >= a.gate_split);
                      }
                      return d;
                  }, acc);
    });
#pragma unroll
    for (int rt = 0; rt < ROWS_RT; ++rt) red[wave][rt][lane] = acc[rt];
    __syncthreads();
    // wave rt: s[e] = (dY~ W)[m0 + 16 rt + c][kf0 + 4 q + e]
    if (wave >= nrt) return;
    f32x4 v = rows_sum(red, min(ROWS_WAVES, nchunk), wave, lane);
    const int f = kf0 + 4 * q, row = m0 + 16 * wave + c;
    if (f >= a.K || row >= a.M) return;
    const bool full4 = f + 3 < a.K;
    if (a.xo) {
        const float* px = a.xo + (long)row * a.ldxo + f;
        f32x4 xo = zero4();
        if (a.vecXo && full4) {
            xo = *reinterpret_cast<const f32x4*>(px);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (f + e < a.K) xo[e] = px[e];
        }
        act_dispatch(a.act_prev, [&](auto actc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= act_grad<decltype(actc)::value>(xo[e], false);
        });
    }
    float* pd = a.dx + (long)row * a.lddx + f;
    if (a.vecDx && full4) {
        *reinterpret_cast<f32x4*>(pd) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (f + e < a.K) pd[e] = v[e];
    }
}

static bool rows_vec(const void* p, long ld, int width) { return aligned16(p) && (ld % 4) == 0 && (width % 4) == 0; }

}  // namespace vpc

using namespace vpc;

extern "C" {

int vpc_rows_max_rows(void) { return ROWS_MAX_M; }

int vpc_rows_fwd(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, long M, int N, int K,
                 int act, int act_split, void* stream) {
    if (!x || !w || !y || M < 1 || N < 1 || K < 1 || ldx < K || ldy < N) return VPC_ERR_ARG;
    if (act < ACT_NONE || act > ACT_RELU) return VPC_ERR_ARG;
    if (M > ROWS_MAX_M || N > ROWS_MAX_F || K > ROWS_MAX_F) return VPC_ERR_SHAPE;
    RowsFwdArgs a{};
    a.x = x; a.ldx = ldx; a.w = w; a.bias = bias; a.y = y; a.ldy = ldy;
    a.M = (int)M; a.N = N; a.K = K; a.act = act; a.split = act == ACT_SIGMOID_HARDTANH ? act_split : N;
    a.vecY = aligned16(y) && (ldy % 4) == 0;
    const dim3 grid((unsigned)((N + 15) / 16), (unsigned)((M + 16 * ROWS_RT - 1) / (16 * ROWS_RT)));
    const dim3 block(64 * ROWS_WAVES);
    hipStream_t st = (hipStream_t)stream;
    if (rows_vec(x, ldx, K) && rows_vec(w, K, K)) hipLaunchKernelGGL(rows_fwd_kernel<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(rows_fwd_kernel<false>, grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_rows_bwd(const float* dy, long lddy, const float* y_gate, long ldyg, int gate, int gate_split, const float* w,
                 const float* x, long ldx, const float* x_out, long ldxo, int act_prev, float* dx, long lddx, float* dw,
                 float* db, long M, int N, int K, int accumulate, void* stream) {
    if (!dy || M < 1 || N < 1 || K < 1 || lddy < N || (!dw && !dx)) return VPC_ERR_ARG;
    if ((dw && (!x || ldx < K)) || (dx && (!w || lddx < K))) return VPC_ERR_ARG;
    if ((y_gate && ldyg < N) || (dx && x_out && ldxo < K)) return VPC_ERR_ARG;
    if (gate < ACT_NONE || gate > ACT_RELU || act_prev < ACT_NONE || act_prev > ACT_RELU) return VPC_ERR_ARG;
    if (M > ROWS_MAX_M || N > ROWS_MAX_F || K > ROWS_MAX_F) return VPC_ERR_SHAPE;
    RowsBwdArgs a{};
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
    const bool vn = rows_vec(dy, lddy, N) && (!y_gate || rows_vec(y_gate, ldyg, N));
    const bool vk = !dw || rows_vec(x, ldx, K);
    const dim3 grid((unsigned)(a.wg_blocks + dg_blocks)), block(64 * ROWS_WAVES);
    hipStream_t st = (hipStream_t)stream;
    if (vn && vk) hipLaunchKernelGGL((rows_bwd_kernel<true, true>), grid, block, 0, st, a);
    else if (vn) hipLaunchKernelGGL((rows_bwd_kernel<true, false>), grid, block, 0, st, a);
    else if (vk) hipLaunchKernelGGL((rows_bwd_kernel<false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((rows_bwd_kernel<false, false>), grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
