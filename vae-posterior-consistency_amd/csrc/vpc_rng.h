// Philox counter RNG and the two per-step draws of the fused steps (device code shared by vpc_misc.hip - the draw kernels -,
// vpc_small.hip, whose small-batch step kernel draws its own tile's mask_p and eps, and the row-tiled fp32 step's in-kernel draws:
// enc_fwd_draw_kernel in vpc_enc.hip draws mask_p for the mask words it holds, dec8_draw_kernel in vpc_dec8.hip the eps of the
// lane that forms z: same counters, same values).
// The counter arithmetic of a lane (the first part of this file) is plain C++ and also compiles in a host program.
#pragma once
#ifdef __HIPCC__
#include "vpc_device.h"
#define VPC_RNG_HD __host__ __device__ __forceinline__
#else
#include <cstdint>
#define VPC_RNG_HD inline
#endif

namespace vpc {

// Row-sharded normal draws: `out` is [planes][rows_local][pitch] (pitch % 4 == 0), the local shard of a global
// [planes][rows_global][pitch] array starting at row row_lo; the Philox counter of a 4-float group is its GLOBAL group
// index + offset, so every row gets the same eps whatever the sharding.  rows_local == 0: flat array, counter = g + offset.
struct EpsShard { long rows_local, rows_global, row_lo; int pitch; };
VPC_RNG_HD uint64_t eps_counter(const EpsShard& sh, long g) {
    if (sh.rows_local == 0) return (uint64_t)g;
    const long gpr = sh.pitch >> 2, gpp = sh.rows_local * gpr;  // groups per row / per local plane
    const long k = g / gpp, rem = g - k * gpp;
    return (uint64_t)((k * sh.rows_global + sh.row_lo) * gpr + rem);
}

// ---- in-kernel draws of the row-tiled step: which counters belong to a lane.  Lane (q, c) of wave w holds, of LOCAL row
// `row` (= 128 tile + 16 w + c) and column tile t, the four mask bytes of columns 16 t + 4 q .. + 3, and forms z[row][4 q .. 4 q + 3].
// mask_p (draw_mask_body): element i of the local [rows][dk] array is element elem_lo + i of the global one, its Philox group is
// that index / 8 and its 16-bit half that index % 8.  With dk % 8 == 0 and elem_lo = row_lo * dk no group straddles a row: the
// lane's four bytes are halves mask_lane_half0(q) .. + 3 of group mask_lane_group(...), i.e. the two words 2 (q & 1), 2 (q & 1) + 1
// of that call, and lanes q and q ^ 1 (same row) share the group.
VPC_RNG_HD long mask_lane_group(long elem_lo, long row, int dk, int t, int q) {
    return ((elem_lo + row * (long)dk) >> 3) + 2 * t + (q >> 1);
}
VPC_RNG_HD int mask_lane_half0(int q) { return 4 * (q & 1); }
// The two lanes of a group split the calls of a tile PAIR (2 u, 2 u + 1): lane q makes the call of tile mask_lane_call_tile(u, q)
// and hands the two words it does not use itself to lane q ^ 1, which needs exactly those (4 calls per lane and 8 tiles, not 8).
VPC_RNG_HD int mask_lane_call_tile(int u, int q) { return 2 * u + (q & 1); }
// eps: the counter (before the offset) of the group z[row][4 q .. 4 q + 3] of plane `plane`: eps_counter of its group index in
// the local [planes][rows_local][pitch] array, without the division.
VPC_RNG_HD uint64_t eps_lane_counter(const EpsShard& sh, int plane, long row, int q) {
    const long gpr = sh.pitch >> 2;
    return (uint64_t)(((long)plane * sh.rows_global + sh.row_lo + row) * gpr + q);
}

}  // namespace vpc

#ifdef __HIPCC__
namespace vpc {

// Philox4x32-10 counter RNG
struct U4 { uint32_t x, y, z, w; };
__device__ __forceinline__ U4 philox(uint64_t ctr, uint32_t stream, uint64_t seed) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = stream, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}
__device__ __forceinline__ float u01(uint32_t u) { return ((u >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// mask_out = mask_in & (U < keep_prob)   (create_missing_uci * mask, utils.py:36-39 + train.py:54-55)
// One Philox call serves 8 mask bytes: each 32-bit word gives two 16-bit uniforms (keep probability resolved to
// 2^-16, far below the sampling noise of any batch).
constexpr int MASK_PER_CALL = 8;
// `elem_lo` = index of this call's first element inside the GLOBAL array (data parallel: shard_lo * d): the Philox
// counter of an element is its global index / 8 + offset, so the drawn mask does not depend on how rows are sharded
__device__ __forceinline__ void draw_mask_body(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, long n,
                                               float keep_prob, uint64_t seed, uint64_t offset, long g, long elem_lo) {
    const long G = (elem_lo >> 3) + g;           // global group
    const long i0 = G * MASK_PER_CALL - elem_lo;  // local index of its first element (negative: group starts in the previous shard)
    if (i0 >= n) return;
    const U4 r = philox((uint64_t)G + offset, 0u, seed);
    const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
    const uint32_t thr = (uint32_t)(keep_prob * 65536.f + 0.5f);
    if (i0 >= 0 && i0 + MASK_PER_CALL - 1 < n && ((((uintptr_t)in + (uintptr_t)i0) | ((uintptr_t)out + (uintptr_t)i0)) & 7u) == 0) {
        uint32_t u[2] = {0x01010101u, 0x01010101u}, o[2] = {0u, 0u};
        if (in) {
            const uint2 v = *reinterpret_cast<const uint2*>(in + i0);
            u[0] = v.x; u[1] = v.y;
        }
#pragma unroll
        for (int j = 0; j < MASK_PER_CALL; ++j) {
            const uint32_t h = (rr[j >> 1] >> (16 * (j & 1))) & 0xffffu;
            if (((u[j >> 2] >> (8 * (j & 3))) & 0xffu) && h < thr) o[j >> 2] |= 1u << (8 * (j & 3));
        }
        *reinterpret_cast<uint2*>(out + i0) = make_uint2(o[0], o[1]);
    } else {
        for (int j = 0; j < MASK_PER_CALL && i0 + j < n; ++j) {
            if (i0 + j < 0) continue;
            const uint32_t h = (rr[j >> 1] >> (16 * (j & 1))) & 0xffffu;
            out[i0 + j] = ((in ? in[i0 + j] : 1) && h < thr) ? 1 : 0;
        }
    }
}

// The keep bits of four consecutive mask bytes from the two Philox words that hold their 16-bit halves (low half first, as
// draw_mask_body numbers them): 0x01 in byte k when half k < thr.  mask & keep_bits4 is draw_mask_body's output for 0 / 1 mask bytes.
__device__ __forceinline__ uint32_t mask_thr(float keep_prob) { return (uint32_t)(keep_prob * 65536.f + 0.5f); }
__device__ __forceinline__ uint32_t keep_bits4(uint32_t w0, uint32_t w1, uint32_t thr) {
    return ((w0 & 0xffffu) < thr ? 1u : 0u) | ((w0 >> 16) < thr ? 0x100u : 0u) | ((w1 & 0xffffu) < thr ? 0x10000u : 0u) |
           ((w1 >> 16) < thr ? 0x1000000u : 0u);
}

__device__ __forceinline__ void fill_normal_body(float* __restrict__ out, long n, uint64_t seed, uint64_t offset,
                                                 long g, const EpsShard& sh) {
    const long i0 = g * 4;
    if (i0 >= n) return;
    const U4 r = philox(eps_counter(sh, g) + offset, 1u, seed);
    // Box-Muller on the hardware transcendentals: v_log_f32 (log2), v_sqrt_f32 and v_sin / v_cos_f32, whose argument is in
    // revolutions - exactly the uniform.  (-2 ln u = -2 ln2 log2 u.)
    const float r0 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u01(r.x)));
    const float r1 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u01(r.z)));
    const float t0 = u01(r.y), t1 = u01(r.w);
    const float s0 = __builtin_amdgcn_sinf(t0), c0 = __builtin_amdgcn_cosf(t0);
    const float s1 = __builtin_amdgcn_sinf(t1), c1 = __builtin_amdgcn_cosf(t1);
    const float v[4] = {r0 * c0, r0 * s0, r1 * c1, r1 * s1};
    for (int j = 0; j < 4 && i0 + j < n; ++j) out[i0 + j] = v[j];
}

// The four normals of ONE group of the eps stream, in registers: exactly the values fill_normal_body stores for the group whose
// counter (eps_counter + offset) is `ctr` - same Philox call, same Box-Muller form.  (vpc_evalsmall.hip: the lane that forms
// z[row][4 q .. 4 q + 3] draws its own eps; nothing is written to memory.)
__device__ __forceinline__ f32x4 eps_normal4(uint64_t ctr, uint64_t seed) {
    const U4 r = philox(ctr, 1u, seed);
    const float r0 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u01(r.x)));
    const float r1 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u01(r.z)));
    const float t0 = u01(r.y), t1 = u01(r.w);
    const float s0 = __builtin_amdgcn_sinf(t0), c0 = __builtin_amdgcn_cosf(t0);
    const float s1 = __builtin_amdgcn_sinf(t1), c1 = __builtin_amdgcn_cosf(t1);
    return f32x4{r0 * c0, r0 * s0, r1 * c1, r1 * s1};
}

// ---- the draws of the AIS engines (vpc_ais.hip: the persistent kernel; vpc_aisg.hip: the GEMM-backed one; ais_draws_kernel)
constexpr uint32_t AIS_KIND_Z0 = 2u, AIS_KIND_V = 3u, AIS_KIND_U = 4u;  // Philox streams (0 / 1: the training-step draws)
constexpr int AIS_DRAW_MAX_L = 64;
// Draw counters: (global chain index, latent 4-group) in the low word, the 1-based temperature index j (0 for z0) in the
// high word, the kind as the Philox stream - independent of tile mapping, workgroup count and launch splitting.  Groups
// past the fourth (latent_dim > 16: the GEMM-backed engine only) go to bits 24.. of the high word, so j < 2^24.
__device__ __forceinline__ uint64_t ais_ctr(long chain, int group, int j) {
    return ((uint64_t)((uint32_t)j | ((uint32_t)(group >> 2) << 24)) << 32) | (uint64_t)(uint32_t)(chain * 4 + (group & 3));
}
// four standard normals (latent components 4 group .. 4 group + 3): the Box-Muller form of fill_normal_body
__device__ __forceinline__ f32x4 ais_normal4(long chain, int group, int j, uint32_t kind, uint64_t seed) {
    const U4 r = philox(ais_ctr(chain, group, j), kind, seed);
    const float r0 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u01(r.x)));
    const float r1 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u01(r.z)));
    const float t0 = u01(r.y), t1 = u01(r.w);
    return f32x4{r0 * __builtin_amdgcn_cosf(t0), r0 * __builtin_amdgcn_sinf(t0), r1 * __builtin_amdgcn_cosf(t1),
                 r1 * __builtin_amdgcn_sinf(t1)};
}
__device__ __forceinline__ float ais_uniform(long chain, int j, uint64_t seed) {
    return u01(philox(ais_ctr(chain, 0, j), AIS_KIND_U, seed).x);
}

// ---- the draws of the streaming imputations (vpc_miw_impute.hip: miw_impute_kernel and miw_impute_draws_kernel; vpc_nm_impute.hip:
// nm_impute_kernel)
constexpr uint32_t MIW_IMP_KIND_A = 5u, MIW_IMP_KIND_B = 6u;  // Philox streams of the sampler's draw and of the fresh draw
// Draw counter of latent components 4 group .. 4 group + 3 of sample s of GLOBAL data row grow (= row0 + row): the row, plus
// the call's offset, in the high word, 4 s + group in the low word, the plane as the Philox stream - independent of the
// chunk length, the grid and the workgroup that draws.  offset + grow < 2^32 and s < 2^30 (checked by the entries).
__device__ __forceinline__ uint64_t miw_imp_ctr(uint64_t offset, long grow, int s, int group) {
    return ((offset + (uint64_t)grow) << 32) | (uint64_t)(uint32_t)(4 * s + group);
}
// latent component l of that draw: the Box-Muller form of fill_normal_body
__device__ __forceinline__ float miw_imp_normal(uint64_t seed, uint64_t offset, int plane, long grow, int s, int l) {
    const U4 r = philox(miw_imp_ctr(offset, grow, s, l >> 2), plane ? MIW_IMP_KIND_B : MIW_IMP_KIND_A, seed);
    const bool hi = (l & 2) != 0;
    const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u01(hi ? r.z : r.x)));
    const float t = u01(hi ? r.w : r.y);
    return rad * ((l & 1) ? __builtin_amdgcn_sinf(t) : __builtin_amdgcn_cosf(t));
}

}  // namespace vpc
#endif  // __HIPCC__
