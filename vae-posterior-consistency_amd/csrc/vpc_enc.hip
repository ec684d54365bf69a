// Encoder kernels (gfx950): q(z|x) MLP  d -> 100 -> 50 -> (mean | logvar), forward and backward.
//
// Reference semantics: Reg_VAE.encoder / vanilla_VAE.encoder, src/models/VAE.py:387-395, 1155-1163
//   h = relu(W1 (x*mask) + b1); h = relu(W2 h + b2); mean, logvar = chunk(W3 h + b3); z = mean + eps*exp(logvar/2)
// and its autograd (src/experiment_main/train.py:115).  See vpc_device.h for the register-chained design.
#include "vpc_device.h"
#include "vpc_bf16.h"
#include "vpc_abi_internal.h"
#include "vpc_enc_args.h"
#include "vpc_rng.h"
#include <atomic>
#include <cstdlib>

namespace vpc {

// layer-1 input tile t of one row in C layout.  AUG = mask-augmented encoder input [x*mask | mask] of width 2d
// (Reg_VAE_mask / vanilla_VAE_mask, src/models/VAE.py:545-548): element f < d is x_f * m_f, d <= f < 2d is m_{f-d}.
template <bool VEC, bool AUG>
__device__ __forceinline__ f32x4 ld_input(const float* x, const uint8_t* mask, long row, int d, int t, int q, bool ok) {
    if (!AUG) {
        const f32x4 xv = ld_tile<VEC>(x, row, d, 16 * t + 4 * q, d, ok);
        const f32x4 mk = ld_mask<VEC>(mask, row, d, 16 * t + 4 * q, d, ok);
        return xv * mk;  // x.float() * mask  (VAE.py:388)
    }
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int f = 16 * t + 4 * q + j;
        const bool isx = ok && f < d, ism = ok && f >= d && f < 2 * d;
        const long ix = isx ? row * d + f : 0, im = (isx || ism) ? row * d + (isx ? f : f - d) : 0;
        const float m = mask[im] ? 1.f : 0.f;
        v[j] = isx ? x[ix] * m : (ism ? m : 0.f);
    }
    return v;
}

// NW = waves per workgroup = 16-row batch tiles per workgroup iteration.  8 (two waves per SIMD, 128-row tiles): the
// throughput shape.  4 (one wave per SIMD, 64-row tiles, passes spread over blockIdx.y): the small-batch shape - a batch
// of 8 192 rows then occupies 256 workgroups x 4 waves = every SIMD of the chip with ONE tile-pass each, instead of 64
// workgroups that each run two passes with two waves per SIMD (the step is latency-bound there, profiles/r01_notes.md).
// PREC (vpc_bf16.h): PREC_F32 = v_mfma_f32_16x16x4_f32 on the fp32 image; PREC_BF16X3 / PREC_BF16 = v_mfma_f32_16x16x32_bf16
// on the bf16 image (same geometry: same row pitches, b1 stays fp32), activations converted tile pair by tile pair.
// DRAW (the 8-wave fp32 PIPE form, two passes in one workgroup): pass 1's mask is not fetched but drawn - the mask words of
// pass 0 stay in their registers (where the prefetched words of pass 1 would sit), and at the head of pass 1 the wave draws
// the keep bits of exactly those bytes (counter rule of draw_mask_body, lane mapping of vpc_rng.h: mask_lane_group /
// mask_lane_call_tile), ANDs them in and stores the mask_p bytes for the decoder and the backward kernel.  Per lane and tile
// FOUR Philox calls: lanes q and q ^ 1 hold the two halves of every group, each makes the call of one tile of a tile pair
// and the two words the other needs cross with a 16-lane swap (ds_swizzle, no LDS memory).
template <int DT, bool VEC, bool AUG, int NW, int PREC = PREC_F32>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void enc_fwd_kernel(EncFwdArgs a) {
    constexpr bool DRAW = false;
    const EncDraw dr{};
#include "vpc_enc_fwd_body.h"
}
// the 8-wave fp32 kernel with the mask_p draw inside (vpc_encoder_fwd_draw_f32)
template <int DT>
__global__ __launch_bounds__(512, 2) void enc_fwd_draw_kernel(EncFwdArgs a, EncDraw dr) {
    constexpr bool VEC = true, AUG = false, DRAW = true;
    constexpr int NW = 8, PREC = PREC_F32;
#include "vpc_enc_fwd_body.h"
}
// Both passes of a tile in ONE sweep over the weight image (vpc_enc_sweep_body.h): the 8-wave fp32 vector kernel for two passes
// in one workgroup and d in (64, 128], with (vpc_encoder_fwd_draw_f32) and without (vpc_encoder_fwd) the mask_p draw.  Same
// arguments, same bytes in every workspace as the pass loop above.
template <int DT, bool DRAW>
__global__ __launch_bounds__(512, 2) void enc_fwd_sweep_kernel(EncFwdArgs a, EncDraw dr) {
#include "vpc_enc_sweep_body.h"
}

// NW as in enc_fwd_kernel.  Every wave owns OWN = 8 / NW slices of each wgrad (the 8-wave kernel: one): in tiles
// w + NW i of dW1 / dW2 and tiles w + NW i of dW3, written to the partial block in the slots of the 8-wave layout
// (vpc_layout.h), so the gradient reduction does not care which shape ran.
template <int DT, bool VEC, bool AUG, int NW, int PREC = PREC_F32>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void enc_bwd_kernel(EncBwdArgs a) {
#include "vpc_enc_bwd_body.h"
}

size_t enc_fwd_lds(int DT) { return sizeof(float) * EncImg(DT).total; }
// Where the sweep kernel is eligible (fp32, vector layout, plain encoder, d in (64, 128], two passes in one workgroup):
// VPC_ENC_SWEEP=0 in the environment keeps the pass-loop kernels, =1 takes the sweep in both forms (A/B runs, tests).  Unset:
// the drawing form sweeps (encoder_fwd 68.7 -> 62.9 us at B = 65 536, profiles/enc_fwd_sweep_notes.md), the non-drawing form
// keeps the pass loop (62.8 against 62.2 us: inside the run-to-run spread, so the default did not move).
static bool enc_sweep_on(bool draw) {
    const char* e = getenv("VPC_ENC_SWEEP");
    return e ? atoi(e) != 0 : draw;
}
// which form the last encoder forward of this process launched (vpc_encoder_fwd_last_form)
static std::atomic<int> enc_fwd_form{-1};
void enc_fwd_set_form(int form) { enc_fwd_form.store(form, std::memory_order_relaxed); }
size_t enc_bwd_lds(int DT, int nw) {
    const EncImg im(DT);
    return sizeof(float) * ((im.total - im.oW2) + 2 * H1P * 16 * nw + nw * 128);
}

template <typename K, typename A>
static int launch(K kern, const A& args, int grid_x, int grid_y, int nw, size_t lds, hipStream_t stream) {
    if (!lds_attr_done(reinterpret_cast<const void*>(kern), lds)) return VPC_ERR_HIP;
    hipLaunchKernelGGL(kern, dim3(grid_x, grid_y), dim3(64 * nw), lds, stream, args);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

// the sweep kernels: (EncFwdArgs, EncDraw), 512 threads, one grid row
template <typename K>
static int launch(K kern, const EncFwdArgs& args, const EncDraw& dr, int grid_x, size_t lds, hipStream_t stream) {
    if (!lds_attr_done(reinterpret_cast<const void*>(kern), lds)) return VPC_ERR_HIP;
    hipLaunchKernelGGL(kern, dim3(grid_x), dim3(512), lds, stream, args, dr);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // namespace vpc

using namespace vpc;

extern "C" int vpc_encoder_fwd(const float* x, const float* enc_img, int npass, const uint8_t* const* mask,
                               const float* const* eps, float* const* h1, float* const* h2, float* const* mean,
                               float* const* logvar, float* const* z, int lat_pitch, int mask_augm, int precision,
                               long B, int d, int L, void* stream) {
    if (!x || !enc_img || !mask || !h1 || !h2 || !mean || !logvar) return VPC_ERR_ARG;
    if (npass < 1 || npass > 2 || B <= 0 || precision < 0 || precision > 2) return VPC_ERR_ARG;
    if (d < 1 || (mask_augm ? 2 * d : d) > MAX_D || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (lat_pitch != L && lat_pitch != 16) return VPC_ERR_ARG;
    if (lat_pitch != L && z) return VPC_ERR_ARG;  // z is only produced in the dense [B][L] layout
    EncFwdArgs a{};
    a.x = x; a.img = enc_img; a.B = B; a.d = d; a.L = L; a.npass = npass; a.lp = lat_pitch;
    const TileShape ts = tile_shape(B, npass);
    a.ntiles = ts.ntiles; a.psplit = ts.small;
    bool vec = (d % 4 == 0) && aligned16(x);
    for (int p = 0; p < npass; ++p) {
        if (!mask[p] || !h1[p] || !h2[p] || !mean[p] || !logvar[p]) return VPC_ERR_ARG;
        a.mask[p] = mask[p]; a.eps[p] = eps ? eps[p] : nullptr; a.h1[p] = h1[p]; a.h2[p] = h2[p];
        a.mean[p] = mean[p]; a.logvar[p] = logvar[p]; a.z[p] = z ? z[p] : nullptr;
        vec = vec && ((uintptr_t)mask[p] % 4 == 0);
        if (!aligned16(h1[p]) || !aligned16(h2[p])) return VPC_ERR_ARG;
    }
    const int DT = dt_for(mask_augm ? 2 * d : d);
    const size_t lds = enc_fwd_lds(DT);
    hipStream_t s = (hipStream_t)stream;
    const bool sweep = precision == PREC_F32 && vec && !mask_augm && DT == 8 && npass == 2 && !ts.small && enc_sweep_on(false);
    enc_fwd_form.store(sweep ? VPC_ENC_FWD_SWEEP : VPC_ENC_FWD_PASSES, std::memory_order_relaxed);
    if (sweep) return launch(enc_fwd_sweep_kernel<8, false>, a, EncDraw{}, ts.grid_x, lds, s);
    if (precision != PREC_F32) {  // bf16 variants: throughput shape, vector layout (d % 4 == 0), plain encoder input
        if (!vec || mask_augm) return VPC_ERR_SHAPE;
#define VPC_CASE(T)                                                                                                    \
    case T:                                                                                                            \
        if (ts.small)                                                                                                  \
            return precision == PREC_BF16X3                                                                            \
                       ? launch(enc_fwd_kernel<T, true, false, 4, PREC_BF16X3>, a, ts.grid_x, ts.grid_y, 4, lds, s)    \
                       : launch(enc_fwd_kernel<T, true, false, 4, PREC_BF16>, a, ts.grid_x, ts.grid_y, 4, lds, s);     \
        return precision == PREC_BF16X3                                                                                \
                   ? launch(enc_fwd_kernel<T, true, false, 8, PREC_BF16X3>, a, ts.grid_x, ts.grid_y, 8, lds, s)        \
                   : launch(enc_fwd_kernel<T, true, false, 8, PREC_BF16>, a, ts.grid_x, ts.grid_y, 8, lds, s);
        switch (DT) { VPC_CASE(1) VPC_CASE(2) VPC_CASE(4) VPC_CASE(8) }
#undef VPC_CASE
        return VPC_ERR_SHAPE;
    }
#define VPC_LAUNCH(T, NW)                                                                                   \
    (mask_augm ? launch(enc_fwd_kernel<T, false, true, NW>, a, ts.grid_x, ts.grid_y, NW, lds, s)            \
     : vec     ? launch(enc_fwd_kernel<T, true, false, NW>, a, ts.grid_x, ts.grid_y, NW, lds, s)            \
               : launch(enc_fwd_kernel<T, false, false, NW>, a, ts.grid_x, ts.grid_y, NW, lds, s))
#define VPC_CASE(T) \
    case T: return ts.small ? VPC_LAUNCH(T, 4) : VPC_LAUNCH(T, 8);
    switch (DT) { VPC_CASE(1) VPC_CASE(2) VPC_CASE(4) VPC_CASE(8) }
#undef VPC_CASE
#undef VPC_LAUNCH
    return VPC_ERR_SHAPE;
}

namespace vpc {
int enc_fwd_draw_prepare(const float* x, const float* enc_img, const uint8_t* mask_in, uint8_t* mask_p_out, float* const* h1,
                         float* const* h2, float* const* mean, float* const* logvar, long B, int d, int L, float keep_prob,
                         unsigned long long seed, unsigned long long offset_mask, const long long* state, long mask_elem_lo,
                         EncFwdArgs& a, EncDraw& dr, TileShape& ts) {
    if (!x || !enc_img || !mask_in || !mask_p_out || !h1 || !h2 || !mean || !logvar || B <= 0 || mask_elem_lo < 0) return VPC_ERR_ARG;
    if (d < 1 || d > MAX_D || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    // a Philox group is 8 consecutive bytes: the lanes' mapping needs rows and the shard to start on a group boundary, and
    // the kernel exists for the 16-byte-vector layout with 8 column tiles
    if (d % 8 != 0 || mask_elem_lo % 8 != 0 || dt_for(d) != 8 || !aligned16(x) || (uintptr_t)mask_in % 4 || (uintptr_t)mask_p_out % 4)
        return VPC_ERR_SHAPE;
    a = EncFwdArgs{};
    a.x = x; a.img = enc_img; a.B = B; a.d = d; a.L = L; a.npass = 2; a.lp = 16;
    ts = tile_shape(B, 2, true);  // the drawing kernel exists in the throughput shape only
    a.ntiles = ts.ntiles; a.psplit = 0;
    for (int p = 0; p < 2; ++p) {
        if (!h1[p] || !h2[p] || !mean[p] || !logvar[p] || !aligned16(h1[p]) || !aligned16(h2[p])) return VPC_ERR_ARG;
        a.h1[p] = h1[p]; a.h2[p] = h2[p]; a.mean[p] = mean[p]; a.logvar[p] = logvar[p];
    }
    a.mask[0] = mask_in; a.mask[1] = mask_p_out;
    dr = EncDraw{mask_p_out, keep_prob, seed, offset_mask, state, mask_elem_lo};
    return VPC_OK;
}
}  // namespace vpc

// vpc_draw_mask + vpc_encoder_fwd (two passes, fp32, 8-wave row-tiled kernel, padded latent workspaces) in ONE launch: see
// include/vpc.h
extern "C" int vpc_encoder_fwd_draw_f32(const float* x, const float* enc_img, const uint8_t* mask_in, uint8_t* mask_p_out,
                                        float* const* h1, float* const* h2, float* const* mean, float* const* logvar, long B,
                                        int d, int L, float keep_prob, unsigned long long seed, unsigned long long offset_mask,
                                        const long long* state, long mask_elem_lo, void* stream) {
    EncFwdArgs a;
    EncDraw dr;
    TileShape ts;
    if (int e = enc_fwd_draw_prepare(x, enc_img, mask_in, mask_p_out, h1, h2, mean, logvar, B, d, L, keep_prob, seed, offset_mask,
                                     state, mask_elem_lo, a, dr, ts))
        return e;
    const bool sweep = enc_sweep_on(true);
    enc_fwd_form.store(sweep ? VPC_ENC_FWD_SWEEP_DRAW : VPC_ENC_FWD_PASSES_DRAW, std::memory_order_relaxed);
    if (sweep) return launch(enc_fwd_sweep_kernel<8, true>, a, dr, ts.grid_x, enc_fwd_lds(8), (hipStream_t)stream);
    auto kern = enc_fwd_draw_kernel<8>;
    const size_t lds = enc_fwd_lds(8);
    if (!lds_attr_done(reinterpret_cast<const void*>(kern), lds)) return VPC_ERR_HIP;
    hipLaunchKernelGGL(kern, dim3(ts.grid_x), dim3(512), lds, (hipStream_t)stream, a, dr);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

extern "C" int vpc_encoder_fwd_last_form(void) { return enc_fwd_form.load(std::memory_order_relaxed); }

namespace vpc {
int enc_bwd_prepare(const float* x, const float* enc_img, int npass, const uint8_t* const* mask, const float* const* h1,
                    const float* const* h2, const float* const* dmean, const float* const* dlogvar, int lat_pitch, int mask_augm,
                    int precision, float* partials, long B, int d, int L, bool force_big, EncBwdArgs& a, bool& vec, TileShape& ts) {
    if (!x || !enc_img || !mask || !h1 || !h2 || !dmean || !dlogvar || !partials) return VPC_ERR_ARG;
    if (npass < 1 || npass > 2 || B <= 0 || precision < 0 || precision > 2) return VPC_ERR_ARG;
    if (d < 1 || (mask_augm ? 2 * d : d) > MAX_D || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (lat_pitch != L && lat_pitch != 16) return VPC_ERR_ARG;
    a = EncBwdArgs{};
    a.x = x; a.img = enc_img; a.part = partials; a.B = B; a.d = d; a.L = L; a.npass = npass; a.lp = lat_pitch;
#ifdef VPC_ABLATE
    if (const char* e = getenv("VPC_DEBUG_ENC")) a.dbg = atoi(e);
#endif
    ts = tile_shape(B, npass, force_big);
    a.ntiles = ts.ntiles; a.psplit = ts.small;
    vec = (d % 4 == 0) && aligned16(x);
    for (int p = 0; p < npass; ++p) {
        if (!mask[p] || !h1[p] || !h2[p] || !dmean[p] || !dlogvar[p]) return VPC_ERR_ARG;
        a.mask[p] = mask[p]; a.h1[p] = h1[p]; a.h2[p] = h2[p]; a.dmean[p] = dmean[p]; a.dlogvar[p] = dlogvar[p];
        vec = vec && ((uintptr_t)mask[p] % 4 == 0);
        if (!aligned16(h1[p]) || !aligned16(h2[p])) return VPC_ERR_ARG;
    }
    return VPC_OK;
}
}  // namespace vpc

extern "C" int vpc_encoder_bwd(const float* x, const float* enc_img, int npass, const uint8_t* const* mask,
                               const float* const* h1, const float* const* h2, const float* const* dmean,
                               const float* const* dlogvar, int lat_pitch, int mask_augm, int precision,
                               float* partials, int* nblocks_out, long B, int d, int L, void* stream) {
    EncBwdArgs a;
    bool vec;
    TileShape ts;
    if (int e = enc_bwd_prepare(x, enc_img, npass, mask, h1, h2, dmean, dlogvar, lat_pitch, mask_augm, precision, partials, B, d,
                                L, false, a, vec, ts))
        return e;
    if (nblocks_out) *nblocks_out = ts.nblocks;
    const int DT = dt_for(mask_augm ? 2 * d : d);
    hipStream_t s = (hipStream_t)stream;
    if (precision != PREC_F32) {
        if (!vec || mask_augm) return VPC_ERR_SHAPE;
#define VPC_CASE(T)                                                                                                              \
    case T:                                                                                                                      \
        if (ts.small)                                                                                                            \
            return precision == PREC_BF16X3                                                                                      \
                       ? launch(enc_bwd_kernel<T, true, false, 4, PREC_BF16X3>, a, ts.grid_x, ts.grid_y, 4, enc_bwd_lds(T, 4), s) \
                       : launch(enc_bwd_kernel<T, true, false, 4, PREC_BF16>, a, ts.grid_x, ts.grid_y, 4, enc_bwd_lds(T, 4), s); \
        return precision == PREC_BF16X3                                                                                          \
                   ? launch(enc_bwd_kernel<T, true, false, 8, PREC_BF16X3>, a, ts.grid_x, ts.grid_y, 8, enc_bwd_lds(T, 8), s)    \
                   : launch(enc_bwd_kernel<T, true, false, 8, PREC_BF16>, a, ts.grid_x, ts.grid_y, 8, enc_bwd_lds(T, 8), s);
        switch (DT) { VPC_CASE(1) VPC_CASE(2) VPC_CASE(4) VPC_CASE(8) }
#undef VPC_CASE
        return VPC_ERR_SHAPE;
    }
#define VPC_LAUNCH(T, NW)                                                                                                  \
    (mask_augm ? launch(enc_bwd_kernel<T, false, true, NW>, a, ts.grid_x, ts.grid_y, NW, enc_bwd_lds(T, NW), s)            \
     : vec     ? launch(enc_bwd_kernel<T, true, false, NW>, a, ts.grid_x, ts.grid_y, NW, enc_bwd_lds(T, NW), s)            \
               : launch(enc_bwd_kernel<T, false, false, NW>, a, ts.grid_x, ts.grid_y, NW, enc_bwd_lds(T, NW), s))
#define VPC_CASE(T) \
    case T: return ts.small ? VPC_LAUNCH(T, 4) : VPC_LAUNCH(T, 8);
    switch (DT) { VPC_CASE(1) VPC_CASE(2) VPC_CASE(4) VPC_CASE(8) }
#undef VPC_CASE
#undef VPC_LAUNCH
    return VPC_ERR_SHAPE;
}
