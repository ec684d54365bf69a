// Encoder kernels (gfx950): q(z|x) MLP  d -> 100 -> 50 -> (mean | logvar), forward and backward.
//
// Reference semantics: Reg_VAE.encoder / vanilla_VAE.encoder, src/models/VAE.py:387-395, 1155-1163
//   h = relu(W1 (x*mask) + b1); h = relu(W2 h + b2); mean, logvar = chunk(W3 h + b3); z = mean + eps*exp(logvar/2)
// and its autograd (src/experiment_main/train.py:115).  See vpc_device.h for the register-chained design.
#include "vpc_device.h"
#include "vpc_bf16.h"
#include "vpc_abi_internal.h"
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

// NW as in enc_fwd_kernel.  Every wave owns OWN = 8 / NW slices of each wgrad (the 8-wave kernel: one): in tiles
// w + NW i of dW1 / dW2 and tiles w + NW i of dW3, written to the partial block in the slots of the 8-wave layout
// (vpc_layout.h), so the gradient reduction does not care which shape ran.
template <int DT, bool VEC, bool AUG, int NW, int PREC = PREC_F32>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void enc_bwd_kernel(EncBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
#ifdef VPC_ABLATE
    unsigned long long T[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tlast = __builtin_amdgcn_s_memtime();
#endif
    // Staging is full width (all batch rows of the workgroup tile at once): ONE write + barrier + read round per
    // wgrad round (two rounds: layer 2, then layers 1 + 3 together), 4 barriers per pass instead of 12 (barriers were 16 %
    // of this kernel, `profiles/r01_notes.md`).  That
    // fits in LDS because the B operand of the layer-1 wgrad - x * mask, the only use of x in this kernel - never
    // goes through LDS: a B fragment wants batch rows along the register index and features along the lanes, which
    // is how row-major x lies in memory, so the tile's owner wave reads it from global memory directly.
    constexpr int TILE_ROWS = 16 * NW, CH = TILE_ROWS, NTHR = 64 * NW, OWN = 8 / NW;
    constexpr bool PIPE = VEC && !AUG;
    const EncImg im(DT);
    const int nW = im.total - im.oW2;  // only W2, W3 are needed (layer 1 has no dgrad)
    float* W2 = lds;
    float* W3 = lds + (im.oW3 - im.oW2);
    float* stA = lds + nW;             // [112][CH]  dY operands (dml, dh2, dh1)
    float* stB = stA + H1P * CH;       // [112][CH]  activations (h2, h1)
    float* db1s = stB + H1P * CH;      // [NW][128]: per-wave bias-gradient sums (no atomics across waves: bit-reproducible)
    // bf16 engine: the same buffers hold the operands as bf16, row-major [batch row][7 tile slots], hi plane + lo plane
    // (vpc_bf16.h, bf_stage_*): written once by the owner of the row, read back with the transposing LDS read
    constexpr bool BF = PREC != PREC_F32;
    constexpr int SKB = CH / 32;
    constexpr bool LB = !BF && NW == 8 && VPC_LANE_BASES;
    constexpr int OFF_B = H1P * CH * 4;  // stB behind stA, bytes (too far for an immediate: the B buffer has bases of its own)
    static_assert(frag_imm(128, H1T - 1, 7) < 65536, "ds_read immediates are 16 bits");
    float* sAh = stA;
    float* sAl = stA + 56 * CH;
    float* sBh = stB;
    float* sBl = stB + 56 * CH;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    // the wave index as a scalar for the ownership tests (threadIdx.x >> 6 is divergent to hipcc: exec-masked regions
    // around the wgrad loops); addresses keep the vector value
    const int ws = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p_lo = a.psplit ? (int)blockIdx.y : 0, p_hi = a.psplit ? p_lo + 1 : a.npass;
    // row-layout operands of one (tile, pass) through range-checked buffer descriptors: rows past B read 0 - zero seeds make
    // dh2, dh1 and every wgrad contribution of such a row exactly zero.  (hipcc turns `ok ? load : 0` into an exec-masked
    // branch with a vmcnt(0) wait at the join.)  The first (tile, pass) of the workgroup is requested before the weight
    // image: in the small-batch shape there is only one, and the two latencies otherwise add up.
    // plain bf16: h1 / h2 arrive as the packed operands enc_fwd stored (4 + 2 k-blocks of 8 bf16 per lane)
    constexpr bool HPK = PREC == PREC_BF16;
    struct RowIn { f32x4 dml[2], h2[HPK ? 1 : H2T], h1[HPK ? 1 : H1T]; BfOp h2p[HPK ? 2 : 1], h1p[HPK ? 4 : 1]; };
    auto fetch_rows = [&](int tile, int p, RowIn& R) {
        const long row0 = (long)tile * TILE_ROWS;
        const int lrow = w * 16 + c;
        if (a.lp == 16) {
            R.dml[0] = ld_rows(rows_rsrc(a.dmean[p], row0, a.B, 16), lrow, 16, 4 * q);
            R.dml[1] = ld_rows(rows_rsrc(a.dlogvar[p], row0, a.B, 16), lrow, 16, 4 * q);
        } else {
            const long row = row0 + lrow;
            R.dml[0] = ld_tile<false>(a.dmean[p], row, a.L, 4 * q, a.L, row < a.B);
            R.dml[1] = ld_tile<false>(a.dlogvar[p], row, a.L, 4 * q, a.L, row < a.B);
        }
        if (HPK) {
            const __amdgpu_buffer_rsrc_t rp2 = rows_rsrc(a.h2[p], row0, a.B, 32), rp1 = rows_rsrc(a.h1[p], row0, a.B, 64);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                R.h2p[kb].hi = __builtin_bit_cast(bf16x8, ld_rows(rp2, lrow, 32, 16 * kb + 4 * q));
                R.h2p[kb].lo = R.h2p[kb].hi;
            }
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                R.h1p[kb].hi = __builtin_bit_cast(bf16x8, ld_rows(rp1, lrow, 64, 16 * kb + 4 * q));
                R.h1p[kb].lo = R.h1p[kb].hi;
            }
            return;
        }
        const __amdgpu_buffer_rsrc_t rh2 = rows_rsrc(a.h2[p], row0, a.B, H2P), rh1 = rows_rsrc(a.h1[p], row0, a.B, H1P);
#pragma unroll
        for (int t = 0; t < H2T; ++t) R.h2[t] = ld_rows(rh2, lrow, H2P, 16 * t + 4 * q);
#pragma unroll
        for (int t = 0; t < H1T; ++t) R.h1[t] = ld_rows(rh1, lrow, H1P, 16 * t + 4 * q);
    };
    // (small-batch shape only: the 8-wave kernel sits at its 256-register limit and would spill the extra copy)
    constexpr bool HOIST = NW == 4;
    RowIn Rpre;
    bool have_pre = false;
    if (HOIST && (int)blockIdx.x < a.ntiles) {
        fetch_rows(blockIdx.x, p_lo, Rpre);
        have_pre = true;
    }
    load_image<(NW == 8 ? 5 : 10)>(lds, a.img + im.oW2, nW);
    for (int i = threadIdx.x; i < NW * 128; i += NTHR) db1s[i] = 0.f;
    __syncthreads();
    int sb[4];  // per-lane element offsets of the staging writes (tile 0); tiles add a compile-time constant
    stage_bases<CH>(sb, 16 * w, c, q);

    f32x4 acc1[OWN][H1T], acc2[OWN][H2T], acc3[OWN], dbacc[H1T];
#pragma unroll
    for (int i = 0; i < H1T; ++i) dbacc[i] = zero4();
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
        acc3[o] = zero4();
#pragma unroll
        for (int i = 0; i < H1T; ++i) acc1[o][i] = zero4();
#pragma unroll
        for (int i = 0; i < H2T; ++i) acc2[o][i] = zero4();
    }

    // layer-1 input features of this lane as B-fragment columns (owned in tiles w + NW o)
    const int din = AUG ? 2 * a.d : a.d;
    bool fx[OWN], fm[OWN];
    int colB[OWN];
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
        const int fB = 16 * (w + NW * o) + c;
        fx[o] = fB < a.d; fm[o] = AUG && fB >= a.d && fB < din;  // x * mask column / appended mask column
        colB[o] = fx[o] ? fB : (fm[o] ? fB - a.d : 0);
    }

    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long row0 = (long)tile * TILE_ROWS;
        for (int p = p_lo; p < p_hi; ++p) {
            int cc = c, qq = q;
            launder(cc, qq);
            VPC_STAMP(0);
            // B fragments of slice s (batch rows row0 + 16 s + 4 q + j): raw x and mask bytes; rows past B read row 0
            // (their dh1 is exactly zero), columns past the input width are cleared when the fragment is formed
            // range-checked buffer loads relative to the tile's first row: a row past B is out of range and reads 0 (x and
            // mask byte), so no clamp; per load one 32-bit add of the slice offset to a per-lane base (the range check
            // covers voffset only, so the slice offset must not go into soffset).  Formed from the laundered lane id:
            // hipcc otherwise precomputes all 32 addresses per tile and spills them.
            const __amdgpu_buffer_rsrc_t rx = rows_rsrc(a.x, row0, a.B, a.d);
            const long mrem = (a.B - row0) * (long)a.d;
            const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t*>(a.mask[p]) + row0 * a.d, 0, mrem > 0xffffffffL ? 0xffffffffu : (uint32_t)mrem, 0x00020000);
            auto ld_xb = [&](int o, int sl, f32x4& xv, uint32_t& mb) {
                const int vo0 = 4 * qq * a.d + colB[o];  // element offset of (row 4 q, this lane's column)
                mb = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int off = vo0 + (16 * sl + j) * a.d;
                    xv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, 4 * off, 0, 0));
                    mb |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rm, off, 0, 0) << (8 * j);
                }
            };
            // fp32 engine: the four mask bytes stay in their own registers until the fragment is formed.  Packing them into
            // one word where they are requested (ld_xb) is VALU on the loaded values in front of the MFMAs the loads are
            // meant to run under (hipcc waits for every slice's mask bytes right behind their request), and five
            // instructions per slice where the unpacked form needs four.
            auto ld_xr = [&](int o, int sl, f32x4& xv, uint32_t (&mr)[4]) {
                const int vo0 = 4 * qq * a.d + colB[o];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int off = vo0 + (16 * sl + j) * a.d;
                    xv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, 4 * off, 0, 0));
                    mr[j] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rm, off, 0, 0);
                }
            };
            auto mk_fr = [&](int o, const f32x4& xv, const uint32_t (&mr)[4]) -> f32x4 {
                const uint32_t k = (AUG || fx[o]) ? 0xffu : 0u;  // columns past the input width: mask 0
                const f32x4 m = {(float)(mr[0] & k), (float)(mr[1] & k), (float)(mr[2] & k), (float)(mr[3] & k)};
                if (!AUG) return xv * m;
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fx[o] ? xv[j] * m[j] : (fm[o] ? m[j] : 0.f);
                return v;
            };
            auto mk_fb = [&](int o, const f32x4& xv, uint32_t mb) -> f32x4 {
                if (!AUG) return xv * mask_to_f32(mb & (fx[o] ? 0xffffffffu : 0u));  // columns past the input width: mask 0
                const f32x4 m = mask_to_f32(mb);
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fx[o] ? xv[j] * m[j] : (fm[o] ? m[j] : 0.f);
                return v;
            };
            RowIn R;
            if (HOIST && have_pre) R = Rpre; else fetch_rows(tile, p, R);
            have_pre = false;
            f32x4 (&dml)[2] = R.dml;
            auto& h2 = R.h2;
            auto& h1 = R.h1;
            // ReLU gate of tile mt from the fp32 tile or, packed form, from the bf16 halves of its operand (relu output >= +0:
            // positive <=> the 16 bits are not zero)
            auto gate_h2 = [&](int mt, f32x4 acc) { return HPK ? bf_gate(acc, R.h2p[HPK ? mt >> 1 : 0], mt & 1) : gate4(acc, h2[HPK ? 0 : mt]); };
            auto gate_h1 = [&](int mt, f32x4 acc) { return HPK ? bf_gate(acc, R.h1p[HPK ? mt >> 1 : 0], mt & 1) : gate4(acc, h1[HPK ? 0 : mt]); };
            // (dW3~ += dml * h2^T is staged and computed together with the layer-1 wgrad below: the B staging buffer is
            // free in that round because x never goes through LDS - 4 instead of 6 barriers per pass)
            VPC_STAMP(1);
            // ---- dh2 = relu'(h2) * (W3~^T dml)
            launder(cc, qq);
            f32x4 dh2[H2T];
            BfOp dmlb[1], dh2b[2];  // bf16 engine: packed once, used by the dgrad MFMAs AND the wgrad staging writes
            if (BF) dmlb[0] = bf_pack<PREC>(dml[0], dml[1]);
            uint32_t tj[4], tv[4];
            if (LB) fragT_bases<64>(tj, tv, W3, cc, qq);
#pragma unroll
            for (int mt = 0; mt < H2T; ++mt) {
                if (LB) dh2[mt] = gate4(tile_T_b<2, 64>(tj, tv, mt, dml, zero4()), h2[mt]);
                else if (PREC == PREC_F32) dh2[mt] = gate4(tile_T<2, 64>(W3, mt, dml, zero4(), cc, qq), h2[mt]);
                else dh2[mt] = gate_h2(mt, bf_tile_T<PREC, 1, 64>(W3, mt, dmlb, zero4(), 16 * qq + cc));
            }
            if (BF) bf_acts<PREC, H2T>(dh2, dh2b);
            VPC_STAMP(2);
            // ---- dW2~ += dh2 * h1^T   (owner: wave w -> in tiles w + NW o < 7, all 4 out tiles)
            launder(cc, qq);
            // staging fragments: bases of tile 0 of the A buffer and of this wave's own tile of the B buffer
            uint32_t sf[4], sfw[4];
            if (LB) {
                frag_bases<CH>(sf, stA, cc, qq);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    sfw[v] = sf[v] + (uint32_t)(OFF_B + ws * frag_imm(CH, 1, 0));
                    asm volatile("" : "+v"(sfw[v]));
                }
            }
            if (!ABLE(2)) lds_barrier();
            if (BF && !ABLE(1)) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) bf_stage_write_op<PREC, 7, H2T>(sAh, sAl, 16 * w + cc, kb, qq, dh2b[kb]);
                if (HPK) {
#pragma unroll
                    for (int kb = 0; kb < 4; ++kb) bf_stage_write_op<PREC, 7, H1T>(sBh, sBl, 16 * w + cc, kb, qq, R.h1p[kb]);
                } else {
#pragma unroll
                    for (int t = 0; t < H1T; ++t) bf_stage_write<PREC, 7>(sBh, sBl, 16 * w + cc, t, qq, h1[HPK ? 0 : t]);
                }
            } else if (!ABLE(1)) {
#pragma unroll
                for (int t = 0; t < H2T; ++t) stage_write_b<CH>(stA, t, dh2[t], sb);
#pragma unroll
                for (int t = 0; t < H1T; ++t) stage_write_b<CH>(stB, t, h1[t], sb);
            }
            if (!ABLE(2)) lds_barrier();
#pragma unroll
            for (int o = 0; o < OWN; ++o) {
                if (PREC != PREC_F32) {
                    if (ws + NW * o < H1T && !ABLE(4)) {
#pragma unroll
                        for (int kb = 0; kb < SKB; ++kb) {
                            asm volatile("" ::: "memory");
                            const BfOp fb = bf_stage_frag<PREC, 7>(sBh, sBl, w + NW * o, kb, 16 * qq + cc);
#pragma unroll
                            for (int mt = 0; mt < H2T; ++mt) {
                                const BfOp fa = bf_stage_frag<PREC, 7>(sAh, sAl, mt, kb, 16 * qq + cc);
                                acc2[o][mt] = bf_mma<PREC>(fa, fb, acc2[o][mt]);
                            }
                        }
                    }
                } else if (ws + NW * o < H1T && !ABLE(4)) {
#pragma unroll
                    for (int s = 0; s < CH / 16; ++s) {
                        asm volatile("" ::: "memory");
                        const f32x4 fb = LB ? frag_ld<CH>(sfw, 0, s) : stage_frag<CH>(stB, w + NW * o, s, cc, qq);
                        // A fragments double-buffered by hand (hipcc sinks each LDS read to its first use: one exposed
                        // LDS latency per 4 MFMAs); the sched_barrier pins the read of mt+1 above the MFMAs of mt
                        f32x4 fa = LB ? frag_ld<CH>(sf, 0, s) : stage_frag<CH>(stA, 0, s, cc, qq);
#pragma unroll
                        for (int mt = 0; mt < H2T; ++mt) {
                            const f32x4 fn = LB ? frag_ld<CH>(sf, mt + 1 < H2T ? mt + 1 : mt, s)
                                                : stage_frag<CH>(stA, mt + 1 < H2T ? mt + 1 : mt, s, cc, qq);
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc2[o][mt] = VPC_MFMA(fa[j], fb[j], acc2[o][mt]);
                            fa = fn;
                        }
                    }
                }
            }
            VPC_STAMP(3);
            // the first two B slices of the layer-1 wgrad come in under the dh1 MFMAs
            constexpr int NS = CH / 16;
            f32x4 xb[OWN][3];  // rotating: slices s, s + 1, s + 2
            uint32_t mbb[OWN][3];
            uint32_t mrr[OWN][3][4];  // fp32 engine: unpacked
#pragma unroll
            for (int o = 0; o < OWN; ++o)
                if (NW * (o + 1) <= DT || ws + NW * o < DT) {
                    if (PREC == PREC_F32) {
                        ld_xr(o, 0, xb[o][0], mrr[o][0]);
                        ld_xr(o, 1, xb[o][1], mrr[o][1]);
                    } else {
                        ld_xb(o, 0, xb[o][0], mbb[o][0]);
                        ld_xb(o, 1, xb[o][1], mbb[o][1]);
                        ld_xb(o, 2, xb[o][2], mbb[o][2]);  // bf16: slices are consumed in pairs
                    }
                }
            // ---- dh1 = relu'(h1) * (W2~^T dh2);  db1 += dh1
            launder(cc, qq);
            f32x4 dh1[H1T];
            // db1: per-lane running sums over all tile-passes; the cross-lane reduction happens ONCE, after the
            // loops (it used to be 4 DPP adds + a predicated ds_add per value and pass: ~170 VALU and 28 exec-masked
            // basic blocks in the middle of the dgrad MFMA stream)
            if (BF) {
                bf_layer_T<PREC, 2, 128, H1T, 4, 2>(W2, dh2b, 16 * qq + cc, [&](int mt, f32x4 acc) {
                    dh1[mt] = gate_h1(mt, acc);
                    dbacc[mt] += dh1[mt];
                });
            } else {
                // (not on lane bases: this phase is the kernel's register peak, and the 4 + 4 bases spill 116 B / lane)
#pragma unroll
                for (int mt = 0; mt < H1T; ++mt) {
                    dh1[mt] = gate4(tile_T<H2T, 128, NK2>(W2, mt, dh2, zero4(), cc, qq), h1[mt]);
                    dbacc[mt] += dh1[mt];
                }
            }
            VPC_STAMP(4);
            // ---- dW1 += dh1 * (x*mask)^T   (owner: wave w -> in tiles w + NW o < DT, all 7 out tiles; B straight from global)
            launder(cc, qq);
            // bases of tile 0 of the A buffer (dW1) and of this wave's two operand tiles of dW3 in the B buffer
            uint32_t s1[4], s3a[4], s3b[4];
            if (LB) {
                frag_bases<CH>(s1, stA, cc, qq);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    s3a[v] = s1[v] + (uint32_t)(OFF_B + (H2T + (ws >> 2)) * frag_imm(CH, 1, 0));
                    s3b[v] = s1[v] + (uint32_t)(OFF_B + (ws & 3) * frag_imm(CH, 1, 0));
                    asm volatile("" : "+v"(s3a[v]), "+v"(s3b[v]));
                }
            }
            if (!ABLE(2)) lds_barrier();
            if (BF && !ABLE(1)) {
#pragma unroll
                for (int t = 0; t < H1T; ++t) bf_stage_write<PREC, 7>(sAh, sAl, 16 * w + cc, t, qq, dh1[t]);
                if (HPK) {
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) bf_stage_write_op<PREC, 7, H2T>(sBh, sBl, 16 * w + cc, kb, qq, R.h2p[kb]);
                } else {
#pragma unroll
                    for (int t = 0; t < H2T; ++t) bf_stage_write<PREC, 7>(sBh, sBl, 16 * w + cc, t, qq, h2[HPK ? 0 : t]);
                }
                bf_stage_write_op<PREC, 7, 6>(sBh, sBl, 16 * w + cc, H2T / 2, qq, dmlb[0]);  // tiles 4, 5
            } else if (!ABLE(1)) {
#pragma unroll
                for (int t = 0; t < H1T; ++t) stage_write_b<CH>(stA, t, dh1[t], sb);
                // operands of dW3~ (tile t8 = w + NW o -> out tile t8 >> 2, in tile t8 & 3): h2 -> stB tiles 0..3, dml -> stB tiles 4, 5
#pragma unroll
                for (int t = 0; t < H2T; ++t) stage_write_b<CH>(stB, t, h2[t], sb);
                stage_write_b<CH>(stB, H2T, dml[0], sb);
                stage_write_b<CH>(stB, H2T + 1, dml[1], sb);
            }
            if (!ABLE(2)) lds_barrier();
#pragma unroll
            for (int o = 0; o < OWN; ++o) {
                const int t8 = w + NW * o;
                if (PREC == PREC_F32) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const f32x4 fa = LB ? frag_ld<CH>(s3a, 0, s) : stage_frag<CH>(stB, H2T + (t8 >> 2), s, cc, qq);
                        const f32x4 fb = LB ? frag_ld<CH>(s3b, 0, s) : stage_frag<CH>(stB, t8 & 3, s, cc, qq);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc3[o] = VPC_MFMA(fa[j], fb[j], acc3[o]);
                    }
                } else {
#pragma unroll
                    for (int kb = 0; kb < SKB; ++kb) {
                        const BfOp fa = bf_stage_frag<PREC, 7>(sBh, sBl, H2T + (t8 >> 2), kb, 16 * qq + cc);
                        const BfOp fb = bf_stage_frag<PREC, 7>(sBh, sBl, t8 & 3, kb, 16 * qq + cc);
                        acc3[o] = bf_mma<PREC>(fa, fb, acc3[o]);
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < OWN; ++o) {
                if (PREC != PREC_F32) {
                    if (NW * (o + 1) <= DT || ws + NW * o < DT) {
                        // slices in pairs (one 32-row k-block per MFMA); ring of 4 slices: block sb2 + 1 in flight
                        f32x4 xq[4] = {xb[o][0], xb[o][1], xb[o][2], zero4()};
                        uint32_t mq[4] = {mbb[o][0], mbb[o][1], mbb[o][2], 0u};
                        if (3 < NS) ld_xb(o, 3, xq[3], mq[3]);
#pragma unroll
                        for (int sb2 = 0; sb2 < NS / 2; ++sb2) {
                            asm volatile("" ::: "memory");
                            const BfOp fb = bf_pack<PREC>(mk_fb(o, xq[(2 * sb2) & 3], mq[(2 * sb2) & 3]),
                                                          mk_fb(o, xq[(2 * sb2 + 1) & 3], mq[(2 * sb2 + 1) & 3]));
                            if (2 * sb2 + 4 < NS) ld_xb(o, 2 * sb2 + 4, xq[(2 * sb2) & 3], mq[(2 * sb2) & 3]);
                            if (2 * sb2 + 5 < NS) ld_xb(o, 2 * sb2 + 5, xq[(2 * sb2 + 1) & 3], mq[(2 * sb2 + 1) & 3]);
#pragma unroll
                            for (int mt = 0; mt < H1T; ++mt) {
                                const BfOp fa = bf_stage_frag<PREC, 7>(sAh, sAl, mt, sb2, 16 * qq + cc);
                                acc1[o][mt] = bf_mma<PREC>(fa, fb, acc1[o][mt]);
                            }
                        }
                    }
                } else if ((NW * (o + 1) <= DT || ws + NW * o < DT) && !ABLE(4)) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        asm volatile("" ::: "memory");  // keep each slice's loads in its slice (hipcc hoists all 8 otherwise)
                        if (s + 2 < NS) ld_xr(o, s + 2, xb[o][(s + 2) % 3], mrr[o][(s + 2) % 3]);
                        const f32x4 fb = mk_fr(o, xb[o][s % 3], mrr[o][s % 3]);
                        f32x4 fa = LB ? frag_ld<CH>(s1, 0, s) : stage_frag<CH>(stA, 0, s, cc, qq);
#pragma unroll
                        for (int mt = 0; mt < H1T; ++mt) {
                            const f32x4 fn = LB ? frag_ld<CH>(s1, mt + 1 < H1T ? mt + 1 : mt, s)
                                                : stage_frag<CH>(stA, mt + 1 < H1T ? mt + 1 : mt, s, cc, qq);
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc1[o][mt] = VPC_MFMA(fa[j], fb[j], acc1[o][mt]);
                            fa = fn;
                        }
                    }
                }
            }
            VPC_STAMP(5);
        }
    }
    // ---- db1 = sum of dh1 over this wave's 16 rows (lanes c): DPP butterfly inside each 16-lane row, then the c == 0
    // lanes own one (wave, feature) slot each - plain stores, fixed order, bit-reproducible
#pragma unroll
    for (int mt = 0; mt < H1T; ++mt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = dbacc[mt][j];
            v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
            v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
            v += dpp_mov<0x141>(v);  // row_half_mirror
            v += dpp_mov<0x140>(v);  // row_mirror: every lane of the 16-lane row holds the row sum
            if (c == 0) db1s[w * 128 + 16 * mt + 4 * q + j] = v;
        }
    // ---- write this workgroup's gradient partial block (8-wave slot layout: owned slice o is "wave" w + NW o)
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
        float* part = a.part + blk * ENC_PART + (long)(w + NW * o) * GREGS * 64 + lane;
#pragma unroll
        for (int mt = 0; mt < H1T; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[(4 * mt + j) * 64] = acc1[o][mt][j];
#pragma unroll
        for (int mt = 0; mt < H2T; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[(28 + 4 * mt + j) * 64] = acc2[o][mt][j];
#pragma unroll
        for (int j = 0; j < 4; ++j) part[(44 + j) * 64] = acc3[o][j];
    }
    __syncthreads();  // every wave's db1s row is complete
    if (threadIdx.x < 128) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < NW; ++k) t += db1s[k * 128 + threadIdx.x];
        a.part[blk * ENC_PART + WAVES * GREGS * 64 + threadIdx.x] = t;
    }
#ifdef VPC_ABLATE
    VPC_STAMP(6);
    if (ABLE(64) && blockIdx.x == 100 && (threadIdx.x & 63) == 0 && (threadIdx.x >> 6) % 3 == 0)
        printf("enc_bwd blk %d wave %d cycles: top %llu loads %llu dh2 %llu dW2 %llu dh1 %llu dW1+dW3 %llu epilogue %llu\n",
               blockIdx.x, (int)(threadIdx.x >> 6), T[0], T[1], T[2], T[3], T[4], T[5], T[6]);
#endif
}

static size_t enc_fwd_lds(int DT) { return sizeof(float) * EncImg(DT).total; }
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
static size_t enc_bwd_lds(int DT, int nw) {
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

// vpc_draw_mask + vpc_encoder_fwd (two passes, fp32, 8-wave row-tiled kernel, padded latent workspaces) in ONE launch: see
// include/vpc.h
extern "C" int vpc_encoder_fwd_draw_f32(const float* x, const float* enc_img, const uint8_t* mask_in, uint8_t* mask_p_out,
                                        float* const* h1, float* const* h2, float* const* mean, float* const* logvar, long B,
                                        int d, int L, float keep_prob, unsigned long long seed, unsigned long long offset_mask,
                                        const long long* state, long mask_elem_lo, void* stream) {
    if (!x || !enc_img || !mask_in || !mask_p_out || !h1 || !h2 || !mean || !logvar || B <= 0 || mask_elem_lo < 0) return VPC_ERR_ARG;
    if (d < 1 || d > MAX_D || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    // a Philox group is 8 consecutive bytes: the lanes' mapping needs rows and the shard to start on a group boundary, and
    // the kernel exists for the 16-byte-vector layout with 8 column tiles
    if (d % 8 != 0 || mask_elem_lo % 8 != 0 || dt_for(d) != 8 || !aligned16(x) || (uintptr_t)mask_in % 4 || (uintptr_t)mask_p_out % 4)
        return VPC_ERR_SHAPE;
    EncFwdArgs a{};
    a.x = x; a.img = enc_img; a.B = B; a.d = d; a.L = L; a.npass = 2; a.lp = 16;
    const TileShape ts = tile_shape(B, 2, true);  // the drawing kernel exists in the throughput shape only
    a.ntiles = ts.ntiles; a.psplit = 0;
    for (int p = 0; p < 2; ++p) {
        if (!h1[p] || !h2[p] || !mean[p] || !logvar[p] || !aligned16(h1[p]) || !aligned16(h2[p])) return VPC_ERR_ARG;
        a.h1[p] = h1[p]; a.h2[p] = h2[p]; a.mean[p] = mean[p]; a.logvar[p] = logvar[p];
    }
    a.mask[0] = mask_in; a.mask[1] = mask_p_out;
    const EncDraw dr{mask_p_out, keep_prob, seed, offset_mask, state, mask_elem_lo};
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

extern "C" int vpc_encoder_bwd(const float* x, const float* enc_img, int npass, const uint8_t* const* mask,
                               const float* const* h1, const float* const* h2, const float* const* dmean,
                               const float* const* dlogvar, int lat_pitch, int mask_augm, int precision,
                               float* partials, int* nblocks_out, long B, int d, int L, void* stream) {
    if (!x || !enc_img || !mask || !h1 || !h2 || !dmean || !dlogvar || !partials) return VPC_ERR_ARG;
    if (npass < 1 || npass > 2 || B <= 0 || precision < 0 || precision > 2) return VPC_ERR_ARG;
    if (d < 1 || (mask_augm ? 2 * d : d) > MAX_D || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (lat_pitch != L && lat_pitch != 16) return VPC_ERR_ARG;
    EncBwdArgs a{};
    a.x = x; a.img = enc_img; a.part = partials; a.B = B; a.d = d; a.L = L; a.npass = npass; a.lp = lat_pitch;
#ifdef VPC_ABLATE
    if (const char* e = getenv("VPC_DEBUG_ENC")) a.dbg = atoi(e);
#endif
    const TileShape ts = tile_shape(B, npass);
    a.ntiles = ts.ntiles; a.psplit = ts.small;
    bool vec = (d % 4 == 0) && aligned16(x);
    for (int p = 0; p < npass; ++p) {
        if (!mask[p] || !h1[p] || !h2[p] || !dmean[p] || !dlogvar[p]) return VPC_ERR_ARG;
        a.mask[p] = mask[p]; a.h1[p] = h1[p]; a.h2[p] = h2[p]; a.dmean[p] = dmean[p]; a.dlogvar[p] = dlogvar[p];
        vec = vec && ((uintptr_t)mask[p] % 4 == 0);
        if (!aligned16(h1[p]) || !aligned16(h2[p])) return VPC_ERR_ARG;
    }
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
