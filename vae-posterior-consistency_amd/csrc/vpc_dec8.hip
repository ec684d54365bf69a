// Fused decoder kernel, 8-wave variant: TWO waves per SIMD, ONE 16-row batch tile per wave.
//
// Same mathematics, LDS images, staging buffers and partial-block layout as dec_kernel<.., MODE_FUSED> in vpc_dec.hip
// (4 waves x 2 batch tiles, one wave per SIMD); what changes is who hides latency.  In the 4-wave kernel everything a
// wave waits for (LDS fragment reads, the VALU of the loss behind the MFMAs of an output tile) is exposed unless the
// compiler interleaves it inside that one wave, and hipcc can only do that by keeping both tiles' state live, which
// spills.  Here the second wave of the SIMD fills those gaps in hardware; the price is one MFMA chain per wave
// (dependent-issue latency) and half the registers per wave (256), which the smaller per-wave state fits:
//   wgrad accumulators 48 (dW6 tile w x 7, dW5 tile w < 7 x 4, dW4 tile w < 4), g1 16, g2 28, dpre 32, latent 16.
// wgrad staging keeps the 64-column buffers: two rounds per phase, waves 4r..4r+3 stage their tile in round r and all
// 8 waves multiply.  Partial blocks are written in the 4-wave layout (out tile mt of dW6 lives at wave mt & 3,
// registers 28 (mt >> 2) + ...), so the host-side index tables and the reduction do not change.
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_bf16.h"
#include "vpc_dec_args.h"
#include "vpc_rng.h"

namespace vpc {

constexpr int DEC8_WAVES = 8, DEC8_THREADS = 512;

// fp32 engine: LDS fragment addresses as lane bases + immediates (vpc_device.h, frag_bases / fragT_bases); 0 builds the
// form that computes every address at its read (for A/B measurements)
#ifndef VPC_LANE_BASES
#define VPC_LANE_BASES 1
#endif

#ifdef VPC_ABLATE
#define ABL(bit) VPC_DBG(bit)   // timing experiments (diagnostic build): 1 no staging writes, 2 no barriers, 4 no wgrad MFMAs
#else
#define ABL(bit) false
#endif

// PREC != PREC_F32: the bf16 engine of vpc_bf16.h on the bf16 decoder image (DecImgBf: W4 rows are 32 dwords).
// DRAW (fp32 only): eps is not read but drawn by the lane that forms z[row][4 q .. 4 q + 3] - vpc_draw_step's counter
// (vpc_rng.h, eps_lane_counter), eps_normal4 - and stored, all 16 floats of the padded row, to dr.eps_w[p].  The pass end re-reads it
// from there with the other statistics (nothing of the draw stays live over the decoder), and eps_buf holds what the separate
// draw launch would have written.
template <int DT, bool VEC, int PREC = PREC_F32>
__global__ __launch_bounds__(DEC8_THREADS) void dec8_kernel(DecArgs a) {
    constexpr bool DRAW = false;
    const DecDraw dr{};
#include "vpc_dec8_body.h"
}
// the fp32 kernel with the eps draw inside (vpc_decoder_fused_draw_f32)
template <int DT>
__global__ __launch_bounds__(DEC8_THREADS) void dec8_draw_kernel(DecArgs a, DecDraw dr) {
    constexpr bool VEC = true, DRAW = true;
    constexpr int PREC = PREC_F32;
#include "vpc_dec8_body.h"
}

size_t dec8_lds(int DT, int prec) {
    const DecImg im(DT, prec == PREC_F32 ? S4 : 32);
    const int na = 16 * DT > H1P ? 16 * DT : H1P;
    return sizeof(float) * (im.total + na * DEC_CH + H1P * DEC_CH + (prec == PREC_F32 ? DEC8_WAVES * LOSS_TERMS : 0));
}

// FUSED mode through the 8-wave kernel; returns VPC_ERR_SHAPE when this variant does not cover the shape
int dec8_dispatch(const DecArgs& a, bool vec, int grid, int prec, hipStream_t s) {
    const int DT = dt_for(a.d);
    const size_t lds = dec8_lds(DT, prec);
    // vector layout (d % 4 == 0, 16-byte aligned rows) only: the scalar-load instantiation of this kernel spilled 468 B
    // per lane at 256 registers; such shapes run the 4-wave kernel of vpc_dec.hip, which has 512 (the caller falls back)
    if (!vec) return VPC_ERR_SHAPE;
#define VPC_CASE8(T)                                                                                         \
    case T: {                                                                                                \
        auto kern = prec == PREC_BF16X3 ? dec8_kernel<T, true, PREC_BF16X3>                                   \
                    : prec == PREC_BF16 ? dec8_kernel<T, true, PREC_BF16>                                     \
                                        : dec8_kernel<T, true, PREC_F32>;                                     \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), lds)) return VPC_ERR_HIP;                    \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(DEC8_THREADS), lds, s, a);                                 \
        return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;                                       \
    }
    switch (DT) { VPC_CASE8(8) }
#undef VPC_CASE8
    return VPC_ERR_SHAPE;
}

int dec8_draw_dispatch(const DecArgs& a, const DecDraw& dr, int grid, hipStream_t s) {
    if (dt_for(a.d) != 8) return VPC_ERR_SHAPE;
    const size_t lds = dec8_lds(8, PREC_F32);
    auto kern = dec8_draw_kernel<8>;
    if (!lds_attr_done(reinterpret_cast<const void*>(kern), lds)) return VPC_ERR_HIP;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(DEC8_THREADS), lds, s, a, dr);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // namespace vpc
