// The row-major GEMM chain of the MIWAE path's N-split kernels (vpc_miw_small.hip: the small-batch step; vpc_miw_impute.hip:
// the streaming imputation): the layout of the flat parameter buffer, the range-checked weight-fragment request straight from
// it, the bias tile and the fragment x LDS-activation product.  One definition, included by both - and by vpc_nm_impute.hip,
// the streaming imputation of the MNAR models, which has the same hidden width and its own buffer layout (NmOff).
#pragma once
#include "vpc_device.h"
#include "vpc_small_device.h"

namespace vpc {

constexpr int MIW_HID = 128;   // VAE.py:3027-3042 / :3153-3168
constexpr int MIW_SMALL_MAX_D = 32, MIW_SMALL_MAX_L = 16, MIW_SMALL_MAX_RB = 4;

// offsets of the twelve tensors in the flat parameter buffer (state_dict order) = in a partial block = in the gradient
struct MiwOff {
    int We1, be1, We2, be2, Wh, bh, Wd1, bd1, Wd2, bd2, Wx, bx, n;
    __host__ __device__ MiwOff(int d, int L) {
        int o = 0;
        We1 = o; o += MIW_HID * d;
        be1 = o; o += MIW_HID;
        We2 = o; o += MIW_HID * MIW_HID;
        be2 = o; o += MIW_HID;
        Wh = o; o += 2 * L * MIW_HID;
        bh = o; o += 2 * L;
        Wd1 = o; o += MIW_HID * L;
        bd1 = o; o += MIW_HID;
        Wd2 = o; o += MIW_HID * MIW_HID;
        bd2 = o; o += MIW_HID;
        Wx = o; o += 3 * d * MIW_HID;
        bx = o; o += 3 * d;
        n = o;
    }
};

// A fragments of out tile mt of the row-major W[N][K]: a[kt][j] = W[16 mt + m][16 kt + 4 q + j], 0 past N and K
template <int KT>
__device__ __forceinline__ void miw_ldA(const float* W, int N, int K, int mt, int m, int q, f32x4 (&a)[KT]) {
    const int row = 16 * mt + m;
    const bool rok = row < N;
    const float* p = W + (long)(rok ? row : 0) * K;
    if ((K & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15u) == 0) {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            const int f = 16 * kt + 4 * q;
            a[kt] = (rok && f < K) ? *reinterpret_cast<const f32x4*>(p + f) : zero4();
        }
    } else {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = 16 * kt + 4 * q + j;
                a[kt][j] = (rok && f < K) ? p[f] : 0.f;
            }
    }
}
// bias of out tile mt in the C layout (lane (c, q): features 16 mt + 4 q + j of row c)
__device__ __forceinline__ f32x4 miw_bias(const float* b, int N, int mt, int q) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (16 * mt + 4 * q + j < N) ? b[16 * mt + 4 * q + j] : 0.f;
    return v;
}
template <int KT>
__device__ __forceinline__ f32x4 miw_mm(const f32x4 (&a)[KT], const float* in, int c, int q, f32x4 acc) {
    f32x4 b[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) b[t] = ld_act(in, t, c, q);
    return mmW<KT>(a, b, acc);
}

}  // namespace vpc
