// Small-batch step of the MIWAE path (MIWAE src/models/VAE.py:3011-3134, Reg_MIWAE :3137-3301, the step of
// src/experiment_main/train.py:102-117), fp32 (gfx950): the GEMM chains of MIWTrainer.step as two kernels in the N-split shape
// of vpc_small.hip - one workgroup of 8 waves, v_mfma_f32_16x16x4_f32, the 8 output tiles of a 128-wide layer one per wave,
// activations handed from layer to layer through LDS as [16 rows][SP] fp32, weights read from the flat parameter buffer in
// global memory (L2-resident, row-major nn.Linear [out][in], state_dict order), requested a stage ahead - and one tail.
//
//   miw_small_fwd_kernel   a workgroup owns RB whole data rows of the stacked passes (row r of [P B]: the q pass first) and
//                          all S samples of each: encoder xin -> h1 -> h2 -> heads once on those rows as one 16-row tile,
//                          hact = (mean | softplus), then per 16-row tile of its RB S decoder rows z = mean + eps * scale,
//                          g1, g2 and the raw heads Y.  Everything is stored to the trainer's workspace buffers.
//   miw_small_bwd_kernel   persistent: workgroup g walks the row blocks g, g + grid, ...  First loop, decoder side: per tile
//                          G (the loss's gradient of the raw heads), g2, g1, z -> dWx, dg2, dWd2, dg1, dWd1, dz, and
//                          sum_s dz (+ the loss's own gh) -> the encoder-head gradient of the row (local: the workgroup owns
//                          every sample of the row).  The decoder's weight blocks are written to the workgroup's partial block,
//                          then the second loop runs the encoder backward on the same row blocks in the same registers.
//   miw_small_tail_kernel  partial blocks summed in workgroup order into the flat gradient, flat Adam.
//
//   miw_small_*_multi_kernel  the three for G members of an ensemble in one launch each (miw_ensemble.MIWEnsembleTrainer): the
//                          kernel bodies are the text fragments vpc_miw_small_fwd_body.h / vpc_miw_small_bwd_body.h, which both
//                          forms include; the head of a multi kernel builds member g's MiwSmallArgs in registers.
//
// The loss between the two (vpc_miw_loss on the raw heads) stays the three launches of vpc_miw.hip: the reference's row /
// sample pairing couples rows across the whole batch.  No float atomics, fixed summation orders: bit-reproducible.
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_small_device.h"
#include "vpc_adam.h"
#include "vpc_miw_device.h"
#include "vpc_miw_chain.h"

#include <cmath>

namespace vpc {

struct MiwSmallArgs {
    const float* prm;    // flat parameters
    const float* xin;    // [R][d]   x * mask of the stacked passes
    const float* eps;    // [R][S][L] the sampling planes
    float *h1, *h2;      // [R][128]
    float *heads, *hact; // [R][2L] raw, (mean | softplus)
    float* z;            // [R S][L]
    float *g1, *g2;      // [R S][128]
    float* Y;            // [R S][3d] raw decoder heads
    const float* G;      // [R S][3d] d loss / d Y            (backward)
    const float* gh;     // [R][2L]  d loss / d hact, the loss's own term
    float* dht;          // [R][2L]  d loss / d heads
    float* part;         // [grid][n_params]
    int R, S, d, L, RB, units;
};

// transposed (dgrad): in-feature tile mt of W[N][K]: a[kt][j] = W[16 kt + 4 q + j][16 mt + m], 0 past N and K
template <int KT>
__device__ __forceinline__ void miw_ldAT(const float* W, int N, int K, int mt, int m, int q, f32x4 (&a)[KT]) {
    const int col = 16 * mt + m;
    const bool cok = col < K;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 16 * kt + 4 * q + j;
            a[kt][j] = (cok && r < N) ? W[(long)r * K + col] : 0.f;
        }
}
// [16][128] rows [row0, row0 + nlive) of a global [..][128] array -> an LDS buffer, dead rows 0: one 16-byte load per thread
__device__ __forceinline__ void miw_stage128(float* buf, const float* g, long row0, int nlive) {
    const int r = threadIdx.x >> 5, f = 4 * (threadIdx.x & 31);
    *reinterpret_cast<f32x4*>(buf + r * SP + f) =
        r < nlive ? *reinterpret_cast<const f32x4*>(g + (row0 + r) * MIW_HID + f) : zero4();
}
// [16][16 T] <- rows [row0, row0 + nlive) of a global [..][W] array, columns past W and dead rows 0
__device__ __forceinline__ void miw_stage(float* buf, const float* g, long row0, int nlive, int W, int T) {
    for (int i = threadIdx.x; i < 256 * T; i += THREADS) {
        const int r = i / (16 * T), f = i - r * 16 * T;
        buf[r * SP + f] = (r < nlive && f < W) ? g[(row0 + r) * W + f] : 0.f;
    }
}
// column sum over the 16 rows of an LDS buffer
__device__ __forceinline__ float miw_colsum(const float* buf, int col) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += buf[r * SP + col];
    return s;
}
// gradient tile (rows 16 ta + 4 q + j, columns 16 tb + c) of dW[N][K] into a partial block
__device__ __forceinline__ void miw_put(float* dW, int N, int K, int ta, int tb, int c, int q, f32x4 acc) {
    const int col = 16 * tb + c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 16 * ta + 4 * q + j;
        if (row < N && col < K) dW[(long)row * K + col] = acc[j];
    }
}

enum { F_X = 0, F_H1, F_H2, F_HD, F_Z, F_G1, F_G2, F_COUNT };
static_assert(F_COUNT * SBUF * 4 <= 65536, "static LDS");

// YT = tiles of the 3 d decoder heads (1 .. 6), LT = tiles of the 2 L encoder heads (1, 2); DT = tiles of d
template <int YT, int LT>
__global__ __launch_bounds__(THREADS) void miw_small_fwd_kernel(MiwSmallArgs a) {
#define MIW_BLK blockIdx.x
#include "vpc_miw_small_fwd_body.h"
#undef MIW_BLK
}

enum { K_DP = 0, K_A2, K_A1, K_Z, K_DA2, K_DA1, K_COUNT };
static_assert(K_COUNT * SBUF * 4 <= 65536, "static LDS");

template <int YT, int LT>
__global__ __launch_bounds__(THREADS) void miw_small_bwd_kernel(MiwSmallArgs a) {
#define MIW_BLK blockIdx.x
#define MIW_NBLK gridDim.x
#include "vpc_miw_small_bwd_body.h"
#undef MIW_BLK
#undef MIW_NBLK
}

// gradient i = the partial blocks' entries i summed in workgroup order, then flat Adam (adam_kernel's update)
__device__ __forceinline__ void miw_small_tail_body(const float* __restrict__ part, int nblk, int n, float* __restrict__ grad,
                                                    const AdamFuse& A) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float g = 0.f;
    int b = 0;
    for (; b + 8 <= nblk; b += 8) {  // eight loads in flight, added in block order
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = part[(long)(b + k) * n + i];
#pragma unroll
        for (int k = 0; k < 8; ++k) g += v[k];
    }
    for (; b < nblk; ++b) g += part[(long)b * n + i];
    grad[i] = g;
    adam_apply(A, i, g);
}
__global__ void miw_small_tail_kernel(const float* __restrict__ part, int nblk, int n, float* __restrict__ grad, AdamFuse A) {
    miw_small_tail_body(part, nblk, n, grad, A);
}

// ================================================================================================ the ensemble forms
// G members in one launch (include/vpc.h, vpc_miw_small_fwd_multi / _bwd_multi / _tail_multi): every workspace is the dense
// [G][rows][width] stack of the stand-alone buffers, so a member's strides follow from (R, S, d, L); only the parameter rows
// and the partial blocks carry a stride of their own.  base = member 0's arguments.
struct MiwSmallMultiArgs {
    MiwSmallArgs base;
    long s_prm, s_part;  // floats between two members' parameter rows / partial blocks
    int G, order, nblk;  // nblk: workgroups per member (fwd: units; bwd: blocks_per_member)
};
// (block, member) of this workgroup, the two orders of vpc_small_member.h: 0 = grid (nblk, G), member-major; 1 = grid
// (8 nblk, ceil(G / 8)), all blocks of a member on ids of one residue mod 8 - one XCD, one L2 for the member's parameters
// (false: a surplus workgroup of the last member group).
__device__ __forceinline__ bool miw_block_member(const MiwSmallMultiArgs& ma, unsigned& blk, unsigned& mem) {
    if (ma.order == 0) {
        mem = blockIdx.y;
        blk = blockIdx.x;
        return true;
    }
    blk = blockIdx.x >> 3;
    mem = 8 * blockIdx.y + (blockIdx.x & 7);
    return mem < (unsigned)ma.G;
}
// member `mem`'s arguments, built in registers from the base record (uniform: scalar arithmetic)
__device__ __forceinline__ MiwSmallArgs miw_member_args(const MiwSmallMultiArgs& ma, const unsigned mem) {
    MiwSmallArgs a = ma.base;
    const long g = mem, R = a.R, RS = R * a.S;
    a.prm += g * ma.s_prm;
    a.xin += g * R * a.d;
    a.eps += g * 2 * RS * a.L;  // [2 P][B][S][L] per member: the sampling planes first
    a.h1 += g * R * MIW_HID; a.h2 += g * R * MIW_HID;
    a.heads += g * R * 2 * a.L; a.hact += g * R * 2 * a.L;
    a.z += g * RS * a.L;
    a.g1 += g * RS * MIW_HID; a.g2 += g * RS * MIW_HID;
    a.Y += g * RS * 3 * a.d;
    if (a.G) a.G += g * RS * 3 * a.d;
    if (a.gh) a.gh += g * R * 2 * a.L;
    if (a.dht) a.dht += g * R * 2 * a.L;
    if (a.part) a.part += g * ma.s_part;
    return a;
}
template <int YT, int LT>
__global__ __launch_bounds__(THREADS) void miw_small_fwd_multi_kernel(MiwSmallMultiArgs ma) {
    unsigned blk, mem;
    if (!miw_block_member(ma, blk, mem)) return;
    const MiwSmallArgs a = miw_member_args(ma, mem);
#define MIW_BLK blk
#include "vpc_miw_small_fwd_body.h"
#undef MIW_BLK
}
template <int YT, int LT>
__global__ __launch_bounds__(THREADS) void miw_small_bwd_multi_kernel(MiwSmallMultiArgs ma) {
    unsigned blk, mem;
    if (!miw_block_member(ma, blk, mem)) return;
    const MiwSmallArgs a = miw_member_args(ma, mem);
    const unsigned nblk = (unsigned)ma.nblk;
#define MIW_BLK blk
#define MIW_NBLK nblk
#include "vpc_miw_small_bwd_body.h"
#undef MIW_BLK
#undef MIW_NBLK
}
// blockIdx.y = member: its partial blocks in block order into its row of the gradient stack, flat Adam with its lr
__global__ void miw_small_tail_multi_kernel(const float* __restrict__ part, int nblk, int n, float* __restrict__ grad,
                                            long s_row, AdamFuse A, const VpcMiwMember* __restrict__ members) {
    const long g = blockIdx.y;
    A.param += g * s_row; A.m += g * s_row; A.v += g * s_row;
    A.lr = members[g].lr;
    miw_small_tail_body(part + g * nblk * n, nblk, n, grad + g * s_row, A);
}

}  // namespace vpc

using namespace vpc;

namespace {

typedef void (*MiwSmallKernel)(MiwSmallArgs);
template <int LT>
MiwSmallKernel miw_small_pick_y(int yt, bool bwd) {
    switch (yt) {
        case 1: return bwd ? miw_small_bwd_kernel<1, LT> : miw_small_fwd_kernel<1, LT>;
        case 2: return bwd ? miw_small_bwd_kernel<2, LT> : miw_small_fwd_kernel<2, LT>;
        case 3: return bwd ? miw_small_bwd_kernel<3, LT> : miw_small_fwd_kernel<3, LT>;
        case 4: return bwd ? miw_small_bwd_kernel<4, LT> : miw_small_fwd_kernel<4, LT>;
        case 5: return bwd ? miw_small_bwd_kernel<5, LT> : miw_small_fwd_kernel<5, LT>;
        default: return bwd ? miw_small_bwd_kernel<6, LT> : miw_small_fwd_kernel<6, LT>;
    }
}
MiwSmallKernel miw_small_pick(int d, int L, bool bwd) {
    const int yt = (3 * d + 15) / 16;
    return 2 * L <= 16 ? miw_small_pick_y<1>(yt, bwd) : miw_small_pick_y<2>(yt, bwd);
}

bool miw_small_shape_ok(long R, int S, int d, int L, int RB) {
    return R > 0 && S > 0 && d > 0 && d <= MIW_SMALL_MAX_D && L > 0 && L <= MIW_SMALL_MAX_L && RB >= 1 &&
           RB <= MIW_SMALL_MAX_RB && R * S <= (1L << 24);
}
typedef void (*MiwSmallMultiKernel)(MiwSmallMultiArgs);
template <int LT>
MiwSmallMultiKernel miw_small_pick_multi_y(int yt, bool bwd) {
    switch (yt) {
        case 1: return bwd ? miw_small_bwd_multi_kernel<1, LT> : miw_small_fwd_multi_kernel<1, LT>;
        case 2: return bwd ? miw_small_bwd_multi_kernel<2, LT> : miw_small_fwd_multi_kernel<2, LT>;
        case 3: return bwd ? miw_small_bwd_multi_kernel<3, LT> : miw_small_fwd_multi_kernel<3, LT>;
        case 4: return bwd ? miw_small_bwd_multi_kernel<4, LT> : miw_small_fwd_multi_kernel<4, LT>;
        case 5: return bwd ? miw_small_bwd_multi_kernel<5, LT> : miw_small_fwd_multi_kernel<5, LT>;
        default: return bwd ? miw_small_bwd_multi_kernel<6, LT> : miw_small_fwd_multi_kernel<6, LT>;
    }
}
MiwSmallMultiKernel miw_small_pick_multi(int d, int L, bool bwd) {
    const int yt = (3 * d + 15) / 16;
    return 2 * L <= 16 ? miw_small_pick_multi_y<1>(yt, bwd) : miw_small_pick_multi_y<2>(yt, bwd);
}
bool miw_multi_width_ok(int d, int L) { return d > 0 && d <= MIW_SMALL_MAX_D && L > 0 && L <= MIW_SMALL_MAX_L; }
// member count, workgroup order and a row stride that holds a member's flat parameters
bool miw_multi_ok(int G, int order, long row_stride, int d, int L) {
    return G >= 1 && G <= VPC_MIW_MULTI_MAX_MEMBERS && (order == 0 || order == 1) && miw_multi_width_ok(d, L) &&
           row_stride >= MiwOff(d, L).n;
}
// nblk workgroups for each of G members in the order of miw_block_member (nblk * G <= VPC_MIW_MULTI_MAX_BLOCKS: checked)
dim3 miw_multi_grid(long nblk, int G, int order) {
    return order == 0 ? dim3((unsigned)nblk, (unsigned)G) : dim3((unsigned)(8 * nblk), (unsigned)((G + 7) / 8));
}

long miw_small_units(long R, int RB) { return (R + RB - 1) / RB; }
long miw_small_grid(long R, int RB) {
    const long u = miw_small_units(R, RB), m = num_cus();  // (a workgroup fills a CU: 8 waves at two per SIMD)
    return u < m ? u : m;
}

}  // namespace

extern "C" {

long vpc_miw_small_workspace(int d, int L) {
    if (d <= 0 || d > MIW_SMALL_MAX_D || L <= 0 || L > MIW_SMALL_MAX_L) return 0;
    return (long)num_cus() * MiwOff(d, L).n;
}

int vpc_miw_small_fwd(const float* params, const float* xin, const float* eps, float* h1, float* h2, float* heads,
                      float* hact, float* z, float* g1, float* g2, float* Y, long R, int S, int d, int L, int RB,
                      void* stream) {
    if (!miw_small_shape_ok(R, S, d, L, RB)) return VPC_ERR_ARG;
    if (!params || !xin || !eps || !h1 || !h2 || !heads || !hact || !z || !g1 || !g2 || !Y) return VPC_ERR_ARG;
    if (!aligned16(h1) || !aligned16(h2) || !aligned16(g1) || !aligned16(g2)) return VPC_ERR_ARG;
    MiwSmallArgs a{};
    a.prm = params; a.xin = xin; a.eps = eps; a.h1 = h1; a.h2 = h2; a.heads = heads; a.hact = hact; a.z = z; a.g1 = g1;
    a.g2 = g2; a.Y = Y;
    a.R = (int)R; a.S = S; a.d = d; a.L = L; a.RB = RB; a.units = (int)miw_small_units(R, RB);
    hipLaunchKernelGGL(miw_small_pick(d, L, false), dim3((unsigned)a.units), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_small_bwd(const float* params, const float* xin, const float* eps, const float* h1, const float* h2,
                      const float* heads, const float* z, const float* g1, const float* g2, const float* G,
                      const float* gh, float* dht, float* part, long part_floats, long R, int S, int d, int L, int RB,
                      void* stream) {
    if (!miw_small_shape_ok(R, S, d, L, RB)) return VPC_ERR_ARG;
    if (!params || !xin || !eps || !h1 || !h2 || !heads || !z || !g1 || !g2 || !G || !gh || !dht || !part) return VPC_ERR_ARG;
    if (!aligned16(h1) || !aligned16(h2) || !aligned16(g1) || !aligned16(g2)) return VPC_ERR_ARG;
    const long grid = miw_small_grid(R, RB);
    if (part_floats < grid * MiwOff(d, L).n) return VPC_ERR_ARG;
    MiwSmallArgs a{};
    a.prm = params; a.xin = xin; a.eps = eps; a.h1 = const_cast<float*>(h1); a.h2 = const_cast<float*>(h2);
    a.heads = const_cast<float*>(heads); a.z = const_cast<float*>(z); a.g1 = const_cast<float*>(g1);
    a.g2 = const_cast<float*>(g2); a.G = G; a.gh = gh; a.dht = dht; a.part = part;
    a.R = (int)R; a.S = S; a.d = d; a.L = L; a.RB = RB; a.units = (int)miw_small_units(R, RB);
    hipLaunchKernelGGL(miw_small_pick(d, L, true), dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_small_tail(const float* part, long part_floats, long R, int RB, int d, int L, float* grad, float* params,
                       float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps, long step,
                       void* stream) {
    if (!miw_small_shape_ok(R, 1, d, L, RB) || !part || !grad || !params || !exp_avg || !exp_avg_sq || step < 1)
        return VPC_ERR_ARG;
    const long grid = miw_small_grid(R, RB);
    const int n = MiwOff(d, L).n;
    if (part_floats < grid * n) return VPC_ERR_ARG;
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    const AdamFuse A{params, exp_avg, exp_avg_sq, nullptr, nullptr, lr, beta1, beta2, eps, (float)bc1, (float)std::sqrt(bc2), 0};
    hipLaunchKernelGGL(miw_small_tail_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, (int)grid, n,
                       grad, A);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------- the ensemble entries
long vpc_miw_multi_workspace(int G, int blocks_per_member, int d, int L) {
    if (G < 1 || G > VPC_MIW_MULTI_MAX_MEMBERS || blocks_per_member < 1 || !miw_multi_width_ok(d, L)) return 0;
    return (long)G * blocks_per_member * MiwOff(d, L).n;
}

int vpc_miw_small_fwd_multi(const float* params, long param_stride, const float* xin, const float* eps, float* h1, float* h2,
                            float* heads, float* hact, float* z, float* g1, float* g2, float* Y, int G, long R, int S, int d,
                            int L, int RB, int order, void* stream) {
    if (!miw_small_shape_ok(R, S, d, L, RB) || !miw_multi_ok(G, order, param_stride, d, L)) return VPC_ERR_ARG;
    if (!params || !xin || !eps || !h1 || !h2 || !heads || !hact || !z || !g1 || !g2 || !Y) return VPC_ERR_ARG;
    if (!aligned16(h1) || !aligned16(h2) || !aligned16(g1) || !aligned16(g2)) return VPC_ERR_ARG;
    const long units = miw_small_units(R, RB);
    if (units * G > VPC_MIW_MULTI_MAX_BLOCKS) return VPC_ERR_ARG;
    MiwSmallMultiArgs ma{};
    MiwSmallArgs& a = ma.base;
    a.prm = params; a.xin = xin; a.eps = eps; a.h1 = h1; a.h2 = h2; a.heads = heads; a.hact = hact; a.z = z; a.g1 = g1;
    a.g2 = g2; a.Y = Y;
    a.R = (int)R; a.S = S; a.d = d; a.L = L; a.RB = RB; a.units = (int)units;
    ma.s_prm = param_stride; ma.G = G; ma.order = order; ma.nblk = (int)units;
    hipLaunchKernelGGL(miw_small_pick_multi(d, L, false), miw_multi_grid(units, G, order), dim3(THREADS), 0, (hipStream_t)stream,
                       ma);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_small_bwd_multi(const float* params, long param_stride, const float* xin, const float* eps, const float* h1,
                            const float* h2, const float* heads, const float* z, const float* g1, const float* g2,
                            const float* Gy, const float* gh, float* dht, float* part, long part_floats, int G,
                            int blocks_per_member, long R, int S, int d, int L, int RB, int order, void* stream) {
    if (!miw_small_shape_ok(R, S, d, L, RB) || !miw_multi_ok(G, order, param_stride, d, L)) return VPC_ERR_ARG;
    if (!params || !xin || !eps || !h1 || !h2 || !heads || !z || !g1 || !g2 || !Gy || !gh || !dht || !part) return VPC_ERR_ARG;
    if (!aligned16(h1) || !aligned16(h2) || !aligned16(g1) || !aligned16(g2)) return VPC_ERR_ARG;
    const long units = miw_small_units(R, RB), n = MiwOff(d, L).n;
    if (blocks_per_member < 1 || blocks_per_member > units || blocks_per_member > num_cus()) return VPC_ERR_ARG;
    if ((long)blocks_per_member * G > VPC_MIW_MULTI_MAX_BLOCKS || part_floats < (long)G * blocks_per_member * n) return VPC_ERR_ARG;
    MiwSmallMultiArgs ma{};
    MiwSmallArgs& a = ma.base;
    a.prm = params; a.xin = xin; a.eps = eps; a.h1 = const_cast<float*>(h1); a.h2 = const_cast<float*>(h2);
    a.heads = const_cast<float*>(heads); a.z = const_cast<float*>(z); a.g1 = const_cast<float*>(g1);
    a.g2 = const_cast<float*>(g2); a.G = Gy; a.gh = gh; a.dht = dht; a.part = part;
    a.R = (int)R; a.S = S; a.d = d; a.L = L; a.RB = RB; a.units = (int)units;
    ma.s_prm = param_stride; ma.s_part = blocks_per_member * n; ma.G = G; ma.order = order; ma.nblk = blocks_per_member;
    hipLaunchKernelGGL(miw_small_pick_multi(d, L, true), miw_multi_grid(blocks_per_member, G, order), dim3(THREADS), 0,
                       (hipStream_t)stream, ma);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_small_tail_multi(const float* part, long part_floats, int G, int blocks_per_member, int d, int L, float* grad,
                             float* params, float* exp_avg, float* exp_avg_sq, long row_stride, const VpcMiwMember* members,
                             float beta1, float beta2, float eps, long step, void* stream) {
    if (!miw_multi_ok(G, 0, row_stride, d, L) || !part || !grad || !params || !exp_avg || !exp_avg_sq || !members || step < 1)
        return VPC_ERR_ARG;
    const int n = MiwOff(d, L).n;
    if (blocks_per_member < 1 || blocks_per_member > num_cus() || part_floats < (long)G * blocks_per_member * n) return VPC_ERR_ARG;
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    const AdamFuse A{params, exp_avg, exp_avg_sq, nullptr, nullptr, 0.f, beta1, beta2, eps, (float)bc1, (float)std::sqrt(bc2), 0};
    hipLaunchKernelGGL(miw_small_tail_multi_kernel, dim3((n + 255) / 256, G), dim3(256), 0, (hipStream_t)stream, part,
                       blocks_per_member, n, grad, row_stride, A, members);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
