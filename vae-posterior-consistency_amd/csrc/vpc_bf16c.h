// Compact bf16 layer image and its wgrad staging (plain bf16: whole-step kernel vpc_step.hip, MNAR decoder / encoder kernels
// vpc_nmdec.hip).  The pair-slot image of vpc_bf16.h carries an unused lo half in plain bf16; this one does not.
//
// Layer image: `rows` rows of KP bf16 (KP = inputs padded to 32); the 16-byte slot pi = 4 kb + q of a row holds the k-slots
// (kb, q, 0..7) = input features 32 kb + 16 (j >> 2) + 4 q + (j & 3) (vpc_bf16.h), pi XOR-swizzled with a key of the row.
// The key makes the forward fragment read (ds_read_b128: 16 rows x one slot per lane group) conflict-free for every row
// pitch - rows of 128 / 64 bytes share a 256-byte bank row in pairs / fours, so the key is taken from the row bits above
// that - and, for 256-byte rows, spreads the 8 consecutive rows of a transposed read (ds_read_b64_tr_b16) over four slot
// groups (2-way instead of 4-way conflicts).
//
// Every kernel instantiates these templates directly, never through a forwarding wrapper.
#pragma once
#include "vpc_bf16.h"

namespace vpc {

template <int KP>
VPC_HD constexpr int c_key(int row) {
    return KP == 128 ? ((((row >> 1) & 3) << 2) | (((row >> 3) & 1) << 1) | (row & 1))
                     : ((row / (128 / KP)) & (KP / 8 - 1));
}
template <int KP>
VPC_HD constexpr int c_elem(int row, int f) {  // u16 index of (row, input feature f) inside the layer image
    return row * KP + (((4 * (f >> 5) + ((f >> 2) & 3)) ^ c_key<KP>(row)) << 3) + 4 * ((f >> 4) & 1) + (f & 3);
}

typedef bf16x8 Op;  // one MFMA operand: 8 k-slots per lane

__device__ __forceinline__ Op pack2(f32x4 t0, f32x4 t1) {
    const u32x4 h = {pk_bf16(t0[0], t0[1]), pk_bf16(t0[2], t0[3]), pk_bf16(t1[0], t1[1]), pk_bf16(t1[2], t1[3])};
    return __builtin_bit_cast(Op, h);
}
// forward A fragment: weight rows 16 mt + m, k-block kb
template <int KP>
__device__ __forceinline__ Op c_wfrag(const float* W, int mt, int kb, int m, int q) {
    return __builtin_bit_cast(Op, *reinterpret_cast<const f32x4*>(W + (16 * mt + m) * (KP / 2) + 4 * ((4 * kb + q) ^ c_key<KP>(m))));
}
// transposed A fragment (dgrad): in-feature tile mt, k-block kb of the layer's OUT features (rows of the image); SECOND = false:
// the image has no rows 32 kb + 16 .. 32 kb + 31, their k-slots are zero
template <int KP, bool SECOND = true>
__device__ __forceinline__ Op c_wfrag_T(const float* W, int mt, int kb, int lane) {
    const int q = lane >> 4, rr = (lane >> 2) & 3, pp = lane & 3;
    const int r0 = 32 * kb + 4 * q + rr, r1 = r0 + 16;
    const int pi = 4 * (mt >> 1) + pp, e = 2 * (mt & 1);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x4 zz = {0, 0, 0, 0};
    const s16x4 h0 = ds_tr16(W + r0 * (KP / 2) + 4 * (pi ^ c_key<KP>(r0)) + e);
    const s16x4 h1 = SECOND ? ds_tr16(W + r1 * (KP / 2) + 4 * (pi ^ c_key<KP>(r1)) + e) : zz;
    const s16x8 h = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    return __builtin_bit_cast(Op, h);
}
// ---- staging (bf_stage layout of vpc_bf16.h with FT slots per row): a packed operand (tiles 2 kb, 2 kb + 1 of the lane's row)
// into slots slot0 + 2 kb (+ 1).  The second tile is written where BOTH (every k-block of the operand has one) or, for an
// operand of NT tiles with NT odd, where it exists (2 kb + 1 < NT: a test on kb inside the k-block loop of the caller)
template <bool BOTH, int FT, int NT = 0>
__device__ __forceinline__ void st_op(float* st, int row, int slot0, int kb, int q, Op op) {
    const u32x4 h = __builtin_bit_cast(u32x4, op);
    const int o0 = bf_stage_off<FT>(row, slot0 + 2 * kb, q);
    *reinterpret_cast<u32x2*>(st + o0) = u32x2{h[0], h[1]};
    if (BOTH || 2 * kb + 1 < NT) *reinterpret_cast<u32x2*>(st + o0 + 64) = u32x2{h[2], h[3]};
}
// transposed read: rows 32 kb .. 32 kb + 31 of slot `slot` as one operand
template <int FT>
__device__ __forceinline__ Op st_frag(const float* st, int slot, int kb, int lane) {
    const int g = lane >> 4, rr = (lane >> 2) & 3, pp = lane & 3;
    const int off = bf_stage_off<FT>(32 * kb + 4 * g + rr, slot, pp);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x4 h0 = ds_tr16(st + off), h1 = ds_tr16(st + off + 128 * FT);
    const s16x8 h = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    return __builtin_bit_cast(Op, h);
}

}  // namespace vpc
