// Argument blocks of the encoder kernels (vpc_enc.hip) and what the one-launch fp32 step (vpc_step_f32.hip), which includes
// their bodies as phases, shares with them.
#pragma once
#include <cstdint>
#include "vpc_abi_internal.h"

namespace vpc {

struct EncFwdArgs {
    const float* x;
    const float* img;
    const uint8_t* mask[2];
    const float* eps[2];
    float* h1[2];
    float* h2[2];
    float* mean[2];
    float* logvar[2];
    float* z[2];
    long B;
    int d, L, npass, ntiles, lp;
    int psplit;  // 1: the passes are spread over blockIdx.y (small batches), 0: every workgroup loops over them
};
// In-kernel mask_p draw, the second argument of enc_fwd_draw_kernel (a record of its own: EncFwdArgs keeps its size, and with
// it the kernel-argument offsets in every other instantiation): pass 1 runs on mask[0] & keep, drawn with vpc_draw_step's
// counters, and stores those bytes to mask_out (= mask[1], which is not read)
struct EncDraw {
    uint8_t* mask_out;
    float keep_prob;
    unsigned long long seed, off_mask;
    const long long* state;  // graph replay: state[1] is added to off_mask
    long elem_lo;            // index of this shard's first mask element in the global array (row_lo * d)
};

struct EncBwdArgs {
    const float* x;
    const float* img;
    const uint8_t* mask[2];
    const float* h1[2];
    const float* h2[2];
    const float* dmean[2];
    const float* dlogvar[2];
    float* part;
    long B;
    int d, L, npass, ntiles, lp, dbg;
    int psplit;  // as EncFwdArgs
};

// 8-wave fp32 backward kernel: LDS fragment addresses as lane bases + immediates (vpc_device.h, frag_bases / fragT_bases);
// 0 builds the form that computes every address at its read (for A/B measurements)
#ifndef VPC_LANE_BASES
#define VPC_LANE_BASES 1
#endif

#ifdef VPC_ABLATE
#define ABLE(bit) ((a.dbg & (bit)) != 0)  // timing experiments (diagnostic build): 1 no staging writes, 2 no barriers, 4 no wgrad 1/2 MFMAs
#else
#define ABLE(bit) false
#endif

// Host side of the three launches of the row-tiled fp32 step, shared with vpc_step_f32: each checks its entry point's
// arguments, fills the kernel's argument block and says which workgroup shape the kernel runs (VPC_OK or the entry's error).
int enc_fwd_draw_prepare(const float* x, const float* enc_img, const uint8_t* mask_in, uint8_t* mask_p_out, float* const* h1,
                         float* const* h2, float* const* mean, float* const* logvar, long B, int d, int L, float keep_prob,
                         unsigned long long seed, unsigned long long offset_mask, const long long* state, long mask_elem_lo,
                         EncFwdArgs& a, EncDraw& dr, TileShape& ts);
// force_big: the throughput shape at every B (as the two drawing kernels run)
int enc_bwd_prepare(const float* x, const float* enc_img, int npass, const uint8_t* const* mask, const float* const* h1,
                    const float* const* h2, const float* const* dmean, const float* const* dlogvar, int lat_pitch, int mask_augm,
                    int precision, float* partials, long B, int d, int L, bool force_big, EncBwdArgs& a, bool& vec, TileShape& ts);
size_t enc_fwd_lds(int DT);
size_t enc_bwd_lds(int DT, int nw);
void enc_fwd_set_form(int form);  // what vpc_encoder_fwd_last_form reports

}  // namespace vpc
