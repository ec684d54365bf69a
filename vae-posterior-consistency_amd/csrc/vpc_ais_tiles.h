// Single-chain tile products of the AIS kernel (vpc_ais.hip): the two templates of vpc_dec8.hip (tile_fwd_p2 / tile_T_p2)
// under names of their own, so that the decoder kernel's translation unit stays as it is.  Same swizzled image reads, same
// 2-deep fragment pipeline: two waves share a SIMD and hide each other's LDS latency, so only two A fragments are in flight.
#pragma once
#include "vpc_device.h"

namespace vpc {

// out tile mt of  W[out][in] * in   (A fragment: one ds_read_b128 per 4 MFMAs)
template <int KT, int S, int NK = 4 * KT>  // NK: k-steps to run (the rest multiply padding zeros)
__device__ __forceinline__ f32x4 ais_tile_fwd(const float* W, int mt, const f32x4 (&in)[KT], int m, int q) {
    constexpr int MASK = (S / 4 - 1) & 15;
    const float* rowp = W + (16 * mt + m) * S;
    f32x4 acc = zero4();
    f32x4 fa = *reinterpret_cast<const f32x4*>(rowp + 4 * ((0 + q) ^ (m & MASK)));
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        const int kn = kt + 1 < KT ? kt + 1 : kt;
        const f32x4 fn = *reinterpret_cast<const f32x4*>(rowp + 4 * ((4 * kn + q) ^ (m & MASK)));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * kt + j < NK) acc = VPC_MFMA(fa[j], in[kt][j], acc);
        fa = fn;
    }
    return acc;
}
// out tile mt of  W^T[in][out] * in  where `in` has KT tiles over W's ROW index (A fragment: 4 x ds_read_b32)
template <int KT, int S, int NK = 4 * KT>
__device__ __forceinline__ f32x4 ais_tile_T(const float* W, int mt, const f32x4 (&in)[KT], int m, int q) {
    constexpr int MASK = (S / 4 - 1) & 15;
    const int col = 16 * mt + m;
    const int cs = col >> 2, cl = col & 3;
    auto rd = [&](int kt) {
        f32x4 f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 4 * q + j;
            f[j] = (4 * kt + j < NK) ? W[(16 * kt + r) * S + (((cs ^ (r & MASK)) << 2) | cl)] : 0.f;
        }
        return f;
    };
    f32x4 acc = zero4();
    f32x4 fa = rd(0);
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        const f32x4 fn = rd(kt + 1 < KT ? kt + 1 : kt);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * kt + j < NK) acc = VPC_MFMA(fa[j], in[kt][j], acc);
        fa = fn;
    }
    return acc;
}

}  // namespace vpc
