// Device helpers of the N-split 16-row-tile kernels (one workgroup of 8 waves per tile, the feature tiles of a layer split
// over the waves, activations handed from layer to layer through LDS): the LDS activation-buffer geometry, the C-layout
// tile <-> buffer accessors, the 16-row weight-gradient tile and the weight-fragment request / use pair.  Shared by vpc_small.hip
// (the training step and its ensemble form), vpc_evalsmall.hip (the evaluate-stage forward) and vpc_miw_small.hip (the MIWAE
// path's small-batch step, which reads its fragments from row-major weights instead): one definition, included by all.
#pragma once
#include "vpc_device.h"

namespace vpc {

constexpr int SP = 144;             // row pitch of the LDS activation buffers (dwords)
constexpr int SBUF = 16 * SP;       // one buffer: 16 rows

// C-layout tile <-> [row][feature] buffer
__device__ __forceinline__ f32x4 ld_act(const float* buf, int t, int c, int q) {
    return *reinterpret_cast<const f32x4*>(buf + c * SP + 16 * t + 4 * q);
}
__device__ __forceinline__ void st_act(float* buf, int t, int c, int q, f32x4 v) {
    *reinterpret_cast<f32x4*>(buf + c * SP + 16 * t + 4 * q) = v;
}

// gradient tile (out tile of A-buffer `da`, in tile of B-buffer `xb`) over the 16 rows: acc[m][n] += sum_row da[row][16 ta + m] * xb[row][16 tb + n]
__device__ __forceinline__ f32x4 wgrad16(const float* da, int ta, const float* xb, int tb, f32x4 acc, int m, int kq) {
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = VPC_MFMA(da[(4 * s + kq) * SP + 16 * ta + m], xb[(4 * s + kq) * SP + 16 * tb + m], acc);
    return acc;
}

// Weight fragments straight from the fp32 image in global memory (the layout of vpc_layout.h: row pitch S dwords, 16-byte slot
// XOR-swizzled with the row) - REQUESTED one stage ahead of their use (ldW / ldWT), consumed by mmW.  Forward: rows 16 mt + m,
// one 16-byte load per k-tile; transposed (dgrad): column 16 mt + m, four dword loads per k-tile (tile_fwd / tile_T of
// vpc_device.h, split into request and use).
template <int KT, int S>
__device__ __forceinline__ void ldW(const float* W, int mt, int m, int q, f32x4 (&a)[KT]) {
    constexpr int MASK = (S / 4 - 1) & 15;
    const float* rowp = W + (16 * mt + m) * S;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) a[kt] = *reinterpret_cast<const f32x4*>(rowp + 4 * ((4 * kt + q) ^ (m & MASK)));
}
template <int KT, int S, int NK = 4 * KT>
__device__ __forceinline__ void ldWT(const float* W, int mt, int m, int q, f32x4 (&a)[KT]) {
    constexpr int MASK = (S / 4 - 1) & 15;
    const int col = 16 * mt + m, cs = col >> 2, cl = col & 3;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 4 * q + j;
            a[kt][j] = (4 * kt + j < NK) ? W[(16 * kt + r) * S + (((cs ^ (r & MASK)) << 2) | cl)] : 0.f;
        }
}
template <int KT, int NK = 4 * KT>
__device__ __forceinline__ f32x4 mmW(const f32x4 (&a)[KT], const f32x4 (&in)[KT], f32x4 acc) {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * kt + j < NK) acc = VPC_MFMA(a[kt][j], in[kt][j], acc);
    return acc;
}

}  // namespace vpc
