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
    constexpr int DT = YT <= 3 ? 1 : 2;
    __shared__ __attribute__((aligned(16))) float lds[F_COUNT * SBUF];
    auto buf = [&](int b) { return lds + b * SBUF; };
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int d = a.d, L = a.L, S = a.S;
    const MiwOff o(d, L);
    const float* P = a.prm;
    const long r0 = (long)blockIdx.x * a.RB;
    const int nr = a.R - r0 < a.RB ? (int)(a.R - r0) : a.RB;
    int cc = c, qq = q;
    // ================================================================ encoder: one tile, rows past nr dead
    f32x4 fW1[DT], fW2[8], fW3[8];
    miw_ldA<DT>(P + o.We1, MIW_HID, d, w, cc, qq, fW1);
    miw_stage(buf(F_X), a.xin, r0, nr, d, DT);
    miw_ldA<8>(P + o.We2, MIW_HID, MIW_HID, w, cc, qq, fW2);
    lds_barrier();
    launder(cc, qq);
    {
        const f32x4 v = relu4(miw_mm<DT>(fW1, buf(F_X), cc, qq, miw_bias(P + o.be1, MIW_HID, w, qq)));
        st_act(buf(F_H1), w, cc, qq, v);
        if (cc < nr) *reinterpret_cast<f32x4*>(a.h1 + (r0 + cc) * MIW_HID + 16 * w + 4 * qq) = v;
    }
    if (w < LT) miw_ldA<8>(P + o.Wh, 2 * L, MIW_HID, w, cc, qq, fW3);
    lds_barrier();
    launder(cc, qq);
    {
        const f32x4 v = relu4(miw_mm<8>(fW2, buf(F_H1), cc, qq, miw_bias(P + o.be2, MIW_HID, w, qq)));
        st_act(buf(F_H2), w, cc, qq, v);
        if (cc < nr) *reinterpret_cast<f32x4*>(a.h2 + (r0 + cc) * MIW_HID + 16 * w + 4 * qq) = v;
    }
    // the decoder's fragments do not change from tile to tile: requested once, here
    f32x4 fW4[1], fW5[8], fW6[8];
    miw_ldA<1>(P + o.Wd1, MIW_HID, L, w, cc, qq, fW4);
    miw_ldA<8>(P + o.Wd2, MIW_HID, MIW_HID, w, cc, qq, fW5);
    if (w < YT) miw_ldA<8>(P + o.Wx, 3 * d, MIW_HID, w, cc, qq, fW6);
    const f32x4 bias4 = miw_bias(P + o.bd1, MIW_HID, w, qq), bias5 = miw_bias(P + o.bd2, MIW_HID, w, qq);
    const f32x4 bias6 = miw_bias(P + o.bx, 3 * d, w < YT ? w : 0, qq);
    lds_barrier();
    launder(cc, qq);
    if (w < LT) {  // heads: raw to the workspace, (mean | softplus(raw)) to the workspace and to LDS for the sampler
        const f32x4 v = miw_mm<8>(fW3, buf(F_H2), cc, qq, miw_bias(P + o.bh, 2 * L, w, qq));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = 16 * w + 4 * qq + j;
            const float act = f < L ? v[j] : miw_softplus(v[j]);
            buf(F_HD)[cc * SP + f] = act;
            if (cc < nr && f < 2 * L) {
                a.heads[(r0 + cc) * 2 * L + f] = v[j];
                a.hact[(r0 + cc) * 2 * L + f] = act;
            }
        }
    }
    lds_barrier();
    launder(cc, qq);
    // ================================================================ decoder: the nr S rows r0 S .. in tiles of 16
    const int nrows = nr * S;
    const long drow0 = r0 * S;
    const int zr = threadIdx.x >> 4, zl = threadIdx.x & 15;
    auto eps_of = [&](int t0) {  // this thread's draw of the tile at t0: requested one tile ahead
        return (threadIdx.x < 256 && t0 + zr < nrows && zl < L) ? a.eps[(drow0 + t0 + zr) * L + zl] : 0.f;
    };
    float e_next = eps_of(0);
    for (int t0 = 0; t0 < nrows; t0 += 16) {
        if (threadIdx.x < 256) {  // z = mean + eps * scale (miw_sample_kernel), columns past L and dead rows 0
            const int row = t0 + zr;
            float zv = 0.f;
            if (row < nrows && zl < L) {
                const int b = row / S;
                const float mu = buf(F_HD)[b * SP + zl], sc = buf(F_HD)[b * SP + L + zl];
                zv = mu + e_next * sc;
                a.z[(drow0 + row) * L + zl] = zv;
            }
            buf(F_Z)[zr * SP + zl] = zv;
        }
        lds_barrier();
        launder(cc, qq);
        e_next = eps_of(t0 + 16);
        const bool live = t0 + cc < nrows;
        const long grow = drow0 + t0 + cc;
        {
            const f32x4 v = relu4(miw_mm<1>(fW4, buf(F_Z), cc, qq, bias4));
            st_act(buf(F_G1), w, cc, qq, v);
            if (live) *reinterpret_cast<f32x4*>(a.g1 + grow * MIW_HID + 16 * w + 4 * qq) = v;
        }
        lds_barrier();
        launder(cc, qq);
        {
            const f32x4 v = relu4(miw_mm<8>(fW5, buf(F_G1), cc, qq, bias5));
            st_act(buf(F_G2), w, cc, qq, v);
            if (live) *reinterpret_cast<f32x4*>(a.g2 + grow * MIW_HID + 16 * w + 4 * qq) = v;
        }
        lds_barrier();
        launder(cc, qq);
        if (w < YT) {
            const f32x4 v = miw_mm<8>(fW6, buf(F_G2), cc, qq, bias6);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = 16 * w + 4 * qq + j;
                if (live && f < 3 * d) a.Y[grow * 3 * d + f] = v[j];
            }
        }
        // (no barrier: the next tile's first write to a buffer lies behind a barrier every reader of this tile has passed)
    }
}

enum { K_DP = 0, K_A2, K_A1, K_Z, K_DA2, K_DA1, K_COUNT };
static_assert(K_COUNT * SBUF * 4 <= 65536, "static LDS");

template <int YT, int LT>
__global__ __launch_bounds__(THREADS) void miw_small_bwd_kernel(MiwSmallArgs a) {
    constexpr int DT = YT <= 3 ? 1 : 2;
    __shared__ __attribute__((aligned(16))) float lds[K_COUNT * SBUF];
    auto buf = [&](int b) { return lds + b * SBUF; };
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int tid = threadIdx.x;
    const int d = a.d, L = a.L, S = a.S;
    const MiwOff o(d, L);
    const float* P = a.prm;
    float* part = a.part + (long)blockIdx.x * o.n;
    int cc = c, qq = q;
    // ================================================================ first loop: decoder side
    // wave w: dWx in-tile w x YT out tiles, dWd2 in-tile w x 8 out tiles, dWd1 out tile w; thread t: one bias column
    // (t < 128: bd2, 128 <= t < 256: bd1, 256 <= t < 256 + 3 d: bx)
    {
        f32x4 accX[YT], acc2[8], acc1 = zero4();
#pragma unroll
        for (int t = 0; t < YT; ++t) accX[t] = zero4();
#pragma unroll
        for (int t = 0; t < 8; ++t) acc2[t] = zero4();
        float db = 0.f;
        for (int u = blockIdx.x; u < a.units; u += gridDim.x) {
            const long r0 = (long)u * a.RB;
            const int nr = a.R - r0 < a.RB ? (int)(a.R - r0) : a.RB;
            const int nrows = nr * S;
            const long drow0 = r0 * S;
            // thread (rb, l) of wave 0: the row's encoder-head gradient, from the loss's own term on (miw_sample_bwd_kernel)
            const int rb = tid >> 4, hl = tid & 15;
            const bool hown = rb < nr && hl < L;
            float gm = hown ? a.gh[(r0 + rb) * 2 * L + hl] : 0.f;
            float gs = hown ? a.gh[(r0 + rb) * 2 * L + L + hl] : 0.f;
            // the operands of a tile are requested one tile ahead (registers pG / p2 / p1 / pz / pe) and written to LDS at the top
            // of their tile: G [16][16 YT], g2, g1 [16][128]; z and the sampling eps as tiles 0 and 3 of K_Z (dz is tile 2)
            constexpr int NG = (256 * YT + THREADS - 1) / THREADS;
            float pG[NG], pz = 0.f, pe = 0.f;
            f32x4 p2 = zero4(), p1 = zero4();
            const int sr = tid >> 5, sf = 4 * (tid & 31), zr = tid >> 4;
            auto fetch = [&](int t0) {
                const int nl = nrows - t0 < 16 ? nrows - t0 : 16;
                const long row0 = drow0 + t0;
#pragma unroll
                for (int k = 0; k < NG; ++k) {
                    const int i = tid + k * THREADS, r = i / (16 * YT), f = i - r * 16 * YT;
                    pG[k] = (i < 256 * YT && r < nl && f < 3 * d) ? a.G[(row0 + r) * 3 * d + f] : 0.f;
                }
                p2 = sr < nl ? *reinterpret_cast<const f32x4*>(a.g2 + (row0 + sr) * MIW_HID + sf) : zero4();
                p1 = sr < nl ? *reinterpret_cast<const f32x4*>(a.g1 + (row0 + sr) * MIW_HID + sf) : zero4();
                const bool zok = tid < 256 && zr < nl && hl < L;
                pz = zok ? a.z[(row0 + zr) * L + hl] : 0.f;
                pe = zok ? a.eps[(row0 + zr) * L + hl] : 0.f;
            };
            auto commit = [&]() {
#pragma unroll
                for (int k = 0; k < NG; ++k) {
                    const int i = tid + k * THREADS, r = i / (16 * YT), f = i - r * 16 * YT;
                    if (i < 256 * YT) buf(K_DP)[r * SP + f] = pG[k];
                }
                *reinterpret_cast<f32x4*>(buf(K_A2) + sr * SP + sf) = p2;
                *reinterpret_cast<f32x4*>(buf(K_A1) + sr * SP + sf) = p1;
                if (tid < 256) {
                    buf(K_Z)[zr * SP + hl] = pz;
                    buf(K_Z)[zr * SP + 48 + hl] = pe;
                }
            };
            fetch(0);
            f32x4 fT6[YT];  // (the first stage's fragments: requested behind their last use, for the next tile)
            miw_ldAT<YT>(P + o.Wx, 3 * d, MIW_HID, w, cc, qq, fT6);
            for (int t0 = 0; t0 < nrows; t0 += 16) {
                const int nl = nrows - t0 < 16 ? nrows - t0 : 16;
                f32x4 fT5[8], fT4[8];
                commit();
                lds_barrier();
                launder(cc, qq);
                if (t0 + 16 < nrows) fetch(t0 + 16);
                // ---- dWx | dg2 = relu'(g2) (Wx^T G) | bx
                miw_ldAT<8>(P + o.Wd2, MIW_HID, MIW_HID, w, cc, qq, fT5);
#pragma unroll
                for (int mt = 0; mt < YT; ++mt) accX[mt] = wgrad16(buf(K_DP), mt, buf(K_A2), w, accX[mt], cc, qq);
                st_act(buf(K_DA2), w, cc, qq, gate4(miw_mm<YT>(fT6, buf(K_DP), cc, qq, zero4()), ld_act(buf(K_A2), w, cc, qq)));
                if (tid >= 256 && tid < 256 + 3 * d) db += miw_colsum(buf(K_DP), tid - 256);
                lds_barrier();
                launder(cc, qq);
                // ---- dWd2 | dg1 | bd2
                if (w == 0) miw_ldAT<8>(P + o.Wd1, MIW_HID, L, 0, cc, qq, fT4);
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) acc2[mt] = wgrad16(buf(K_DA2), mt, buf(K_A1), w, acc2[mt], cc, qq);
                st_act(buf(K_DA1), w, cc, qq, gate4(miw_mm<8>(fT5, buf(K_DA2), cc, qq, zero4()), ld_act(buf(K_A1), w, cc, qq)));
                if (tid < 128) db += miw_colsum(buf(K_DA2), tid);
                lds_barrier();
                launder(cc, qq);
                // ---- dWd1 | dz (wave 0, into tile 2 of K_Z) | bd1
                if (t0 + 16 < nrows) miw_ldAT<YT>(P + o.Wx, 3 * d, MIW_HID, w, cc, qq, fT6);
                acc1 = wgrad16(buf(K_DA1), w, buf(K_Z), 0, acc1, cc, qq);
                if (w == 0) st_act(buf(K_Z), 2, cc, qq, miw_mm<8>(fT4, buf(K_DA1), cc, qq, zero4()));
                if (tid >= 128 && tid < 256) db += miw_colsum(buf(K_DA1), tid - 128);
                lds_barrier();
                launder(cc, qq);
                // ---- sum over the row's samples, in sample order: rows [lo, hi) of the tile are samples of data row rb
                if (hown) {
                    const int lo = rb * S - t0 > 0 ? rb * S - t0 : 0, hi = (rb + 1) * S - t0 < nl ? (rb + 1) * S - t0 : nl;
                    for (int r = lo; r < hi; ++r) {
                        const float dzv = buf(K_Z)[r * SP + 32 + hl];
                        gm += dzv;
                        gs += dzv * buf(K_Z)[r * SP + 48 + hl];
                    }
                }
                lds_barrier();  // the next tile's operands overwrite what this stage and the last one read
                launder(cc, qq);
            }
            if (hown) {
                a.dht[(r0 + rb) * 2 * L + hl] = gm;
                a.dht[(r0 + rb) * 2 * L + L + hl] = gs * miw_softplus_d(a.heads[(r0 + rb) * 2 * L + L + hl]);
            }
        }
#pragma unroll
        for (int mt = 0; mt < YT; ++mt) miw_put(part + o.Wx, 3 * d, MIW_HID, mt, w, c, q, accX[mt]);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) miw_put(part + o.Wd2, MIW_HID, MIW_HID, mt, w, c, q, acc2[mt]);
        miw_put(part + o.Wd1, MIW_HID, L, w, 0, c, q, acc1);
        if (tid < 128) part[o.bd2 + tid] = db;
        else if (tid < 256) part[o.bd1 + tid - 128] = db;
        else if (tid < 256 + 3 * d) part[o.bx + tid - 256] = db;
    }
    __syncthreads();  // dht of this workgroup's rows is in memory; every LDS buffer is free
    launder(cc, qq);
    // ================================================================ second loop: encoder side, the same row blocks
    // wave w: dWh in-tile w x LT out tiles, dWe2 in-tile w x 8 out tiles, dWe1 out tile w x DT in tiles; thread t: one bias
    // column (t < 128: be2, 128 <= t < 256: be1, 256 <= t < 256 + 2 L: bh)
    {
        f32x4 accH[LT], acc2[8], acc1[DT];
#pragma unroll
        for (int t = 0; t < LT; ++t) accH[t] = zero4();
#pragma unroll
        for (int t = 0; t < 8; ++t) acc2[t] = zero4();
#pragma unroll
        for (int t = 0; t < DT; ++t) acc1[t] = zero4();
        float db = 0.f;
        for (int u = blockIdx.x; u < a.units; u += gridDim.x) {
            const long r0 = (long)u * a.RB;
            const int nr = a.R - r0 < a.RB ? (int)(a.R - r0) : a.RB;
            f32x4 fT3[LT], fT2[8];
            miw_ldAT<LT>(P + o.Wh, 2 * L, MIW_HID, w, cc, qq, fT3);
            miw_stage(buf(K_DP), a.dht, r0, nr, 2 * L, LT);
            miw_stage128(buf(K_A2), a.h2, r0, nr);
            miw_stage128(buf(K_A1), a.h1, r0, nr);
            miw_stage(buf(K_Z), a.xin, r0, nr, d, DT);
            lds_barrier();
            launder(cc, qq);
            // ---- dWh | dh2 | bh
            miw_ldAT<8>(P + o.We2, MIW_HID, MIW_HID, w, cc, qq, fT2);
#pragma unroll
            for (int mt = 0; mt < LT; ++mt) accH[mt] = wgrad16(buf(K_DP), mt, buf(K_A2), w, accH[mt], cc, qq);
            st_act(buf(K_DA2), w, cc, qq, gate4(miw_mm<LT>(fT3, buf(K_DP), cc, qq, zero4()), ld_act(buf(K_A2), w, cc, qq)));
            if (tid >= 256 && tid < 256 + 2 * L) db += miw_colsum(buf(K_DP), tid - 256);
            lds_barrier();
            launder(cc, qq);
            // ---- dWe2 | dh1 | be2
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) acc2[mt] = wgrad16(buf(K_DA2), mt, buf(K_A1), w, acc2[mt], cc, qq);
            st_act(buf(K_DA1), w, cc, qq, gate4(miw_mm<8>(fT2, buf(K_DA2), cc, qq, zero4()), ld_act(buf(K_A1), w, cc, qq)));
            if (tid < 128) db += miw_colsum(buf(K_DA2), tid);
            lds_barrier();
            launder(cc, qq);
            // ---- dWe1 | be1
#pragma unroll
            for (int t = 0; t < DT; ++t) acc1[t] = wgrad16(buf(K_DA1), w, buf(K_Z), t, acc1[t], cc, qq);
            if (tid >= 128 && tid < 256) db += miw_colsum(buf(K_DA1), tid - 128);
            lds_barrier();  // the next row block stages into the buffers read above
            launder(cc, qq);
        }
#pragma unroll
        for (int mt = 0; mt < LT; ++mt) miw_put(part + o.Wh, 2 * L, MIW_HID, mt, w, c, q, accH[mt]);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) miw_put(part + o.We2, MIW_HID, MIW_HID, mt, w, c, q, acc2[mt]);
#pragma unroll
        for (int t = 0; t < DT; ++t) miw_put(part + o.We1, MIW_HID, d, w, t, c, q, acc1[t]);
        if (tid < 128) part[o.be2 + tid] = db;
        else if (tid < 256) part[o.be1 + tid - 128] = db;
        else if (tid < 256 + 2 * L) part[o.bh + tid - 256] = db;
    }
}

// gradient i = the partial blocks' entries i summed in workgroup order, then flat Adam (adam_kernel's update)
__global__ void miw_small_tail_kernel(const float* __restrict__ part, int nblk, int n, float* __restrict__ grad, AdamFuse A) {
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

}  // extern "C"
