// Small-batch whole-step kernel, fp32 (gfx950): one workgroup of 8 waves per 16-ROW tile, the FEATURE tiles of every layer
// split over the waves ("N-split"), activations handed from layer to layer through LDS.
//
// Reference semantics: the Reg_VAE / vanilla_VAE training step of src/experiment_main/train.py:87-115 (src/models/VAE.py:496-507
// forward, :403-467 loss, autograd backward) - the same mathematics, fp32 v_mfma_f32_16x16x4_f32 products, weight images, loss
// coefficients and gradient partial-block layouts as vpc_encoder_fwd -> vpc_decoder_fused -> vpc_encoder_bwd with precision 0.
//
// Why.  The row-tiled kernels give a wave 16 batch rows and the whole MLP: a wave's life is the serial chain of all layers
// (~2 000 dependent MFMAs, 13 + 29 + 17 us for the three kernels at batch 64 - the reference's own batch size,
// Data/imputation_args.json - whatever the batch, with 8 of the chip's 1 024 SIMDs busy).  Here the 7 / 4 / 2 / 4 / 7 / 8 output
// tiles of a layer belong to different waves, so a layer is ~30 MFMAs deep instead of ~220 and the step is ONE launch; the price
// is a workgroup barrier per layer and that the weights are not LDS-resident: every wave reads the A fragments of its tile
// straight from the fp32 image in global memory (L2-resident, 193 KB; the row-tiled kernels' own image format, so Adam's
// re-pack serves both), requested one layer ahead.
// LDS: activations and their gradients of the tile as [16 rows][144] fp32 (features contiguous: the C-layout store of a tile
// is one ds_write_b128 per lane, the B operand of the next layer one ds_read_b128 per k-tile; the pitch of 144 dwords puts
// the four 4-row groups of a wgrad's dword reads on different banks).  wgrad contracts over the tile's 16 rows: four MFMAs
// per 16 x 16 gradient tile, operands read as dwords down the columns.
// Gradient accumulators live in registers across the tiles of a workgroup in the 8-wave slot layout of vpc_layout.h (the
// partial blocks are what vpc_reduce_step(_adam) expects).
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_small_device.h"
#include "vpc_rng.h"
#include "vpc_dec_args.h"

namespace vpc {

enum { B_XQ = 0, B_XP, B_H1Q, B_H1P, B_H2Q, B_H2P, B_ML, B_Z, B_G1, B_G2, B_DP, B_DG2, B_DG1, B_DMLQ, B_DMLP, B_DH2, B_DH1, B_COUNT };
constexpr int SMALL_LDS = (B_COUNT * SBUF + WAVES * LOSS_TERMS) * 4;
static_assert(SMALL_LDS <= 163840, "LDS budget");

struct SmallArgs {
    const float* x;
    const float* enc_img;
    const float* dec_img;
    const uint8_t* m[2];
    const uint8_t* mB[2];
    float cA[2], cE[2];
    const float* eps[2];
    const float* eps_ml;
    float* partE;
    float* partD;
    double* loss_part;
    float bq, bp, cr, wml, inv_B, x_logvar;
    long B;
    int d, L, npass, ntiles;
    // optional in-kernel draws of the step (vpc_step_small_draw_f32): the workgroup draws the mask_p bytes and the eps values of ITS
    // 16 rows with the counters vpc_draw_step would use, stores them where the step reads them (m[1], eps[...]) and goes on
    int draw;                    // 0: inputs are given; 1: draw eps (and mask_p when mask_in != NULL)
    int d_real;                  // mask-augmented kernels: obs_dim (d is the row pitch); in the padding in front of mask_in, so
                                 // the argument offsets of the plain kernels stay what they were
    const uint8_t* mask_in;      // mask that mask_p thins (NULL: no mask draw - vanilla_VAE)
    float keep_prob;
    float* eps_out; long n_eps;  // [planes][B][16] planes of normals, n_eps floats in all
    unsigned long long seed, off_mask, off_eps;
    const long long* state;
    long mask_elem_lo;
    EpsShard shard;
};
// what the point-net kernel (step_small_eddi_kernel) takes besides: the tile body names it pnx
struct SmallPointNet {
    int K;                       // emb_dim: width of the trunk's input agg
    const float* front;          // the front-end parameters in flat order: E [d_real][K] | t [d_real] | W [K][2+K] | c [K]
    float* partF;                // [tiles][2][K][d]: the tile's (dA | dC) block
    float* snap;                 // [n_front]: tile 0 leaves the parameters of this step here for the tail's chain rule
};
struct SmallPnArgs : SmallArgs { SmallPointNet pn; };

template <int DT>
__global__ __launch_bounds__(THREADS) void step_small_kernel(SmallArgs a) {
    constexpr int DTI = DT;
    constexpr bool AUG = false;
    constexpr bool PN = false;
    constexpr SmallPointNet pnx{};
    const unsigned tile_id = blockIdx.x;
#include "vpc_small_body.h"
}

// Reg_VAE_mask / vanilla_VAE_mask (src/models/VAE.py:510-667, 995-1116): encoder input [x*mask | mask] of DTI = dt_for(2 d) tiles,
// decoder output of DT = dt_for(d) tiles.
template <int DTI, int DT>
__global__ __launch_bounds__(THREADS) void step_small_aug_kernel(SmallArgs a) {
    constexpr bool AUG = true;
    constexpr bool PN = false;
    constexpr SmallPointNet pnx{};
    const unsigned tile_id = blockIdx.x;
#include "vpc_small_body.h"
}

// Reg_EDDI / vanilla_EDDI (src/models/VAE.py:670-853, 856-992): the point-net front-end (:719-733, 903-917) as the input stage -
// folded per workgroup into LDS -, the trunk K -> 100 -> 50 -> 2L as the body's encoder with DTI = dt_for(K) input tiles, decoder
// output of DT = dt_for(d) tiles; the encoder backward goes on to dagg = dh1 . W1 and the front-end's (dA | dC) block of the tile.
template <int DTI, int DT>
__global__ __launch_bounds__(THREADS) void step_small_eddi_kernel(SmallPnArgs a) {
    constexpr bool AUG = false;
    constexpr bool PN = true;
    const SmallPointNet& pnx = a.pn;
    const unsigned tile_id = blockIdx.x;
#include "vpc_small_body.h"
}

}  // namespace vpc

using namespace vpc;

// Rows up to which the library runs an fp32 step through vpc_step_small_f32 (0 = never): by default one round of workgroups
// (16 rows x CUs).  The kernel takes up to 2 x CUs tiles (the partial-block buffers' size).  VPC_TILE=16 forces this path for every batch, VPC_TILE=64 / 128 (the
// row-tiled workgroup shapes) switch it off, VPC_STEP_SMALL=n sets the row limit (A/B runs, tests).
extern "C" long vpc_step_small_max_rows(void) {
    long lim = 16L * num_cus();
    if (const char* e = getenv("VPC_TILE")) {
        const int v = atoi(e);
        if (v == 16) lim = 32L * num_cus();
        if (v == 64 || v == 128) lim = 0;
    }
    if (const char* e = getenv("VPC_STEP_SMALL")) lim = atol(e);
    return lim;
}

namespace vpc {
struct SmallDraw {
    int on; const uint8_t* mask_in; float keep_prob; float* eps_out; long n_eps; unsigned long long seed, off_mask, off_eps;
    const long long* state; long mask_elem_lo; EpsShard shard;
};
static int step_small_launch(const float* x, const float* enc_img, const float* dec_img, int npass,
                             const uint8_t* const* mask, const uint8_t* const* maskB, const VpcLossCoef* co,
                             const float* const* eps, const float* eps_ml, float inv_B, float x_logvar, float* partE, float* partD, double* loss_partials,
                             int* nblocks_out, long B, int d, int L, const SmallDraw& dr, void* stream, int d_real = 0,
                             const SmallPointNet* pn = nullptr) {
    // d_real != 0: the mask-augmented kernels - obs_dim d_real in rows of pitch d = 4 ceil(d_real / 4), encoder input 2 d_real wide;
    // with pn: the point-net kernels - the same rows, encoder input pn->K wide
    const bool aug = d_real != 0 && !pn;
    if (!x || !enc_img || !dec_img || !mask || !co || !eps || !partE || !partD || !loss_partials) return VPC_ERR_ARG;
    if (npass < 1 || npass > 2 || B <= 0) return VPC_ERR_ARG;
    if (d < 4 || d > MAX_D || d % 4 || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (aug && (d_real < 1 || d_real > d || d - d_real > 3 || 2 * d_real > MAX_D)) return VPC_ERR_SHAPE;
    // (d <= 64, K <= 32: the instantiations, and what the front-end's LDS workspace of the tile body is laid out for)
    if (pn && (d_real < 1 || d_real > d || d - d_real > 3 || d > 64 || pn->K < 1 || pn->K > 32)) return VPC_ERR_SHAPE;
    if (pn && (!pn->front || !pn->partF || !pn->snap || (uintptr_t)pn->front % 4 || (uintptr_t)pn->partF % 4 || (uintptr_t)pn->snap % 4))
        return VPC_ERR_ARG;
    if (!aligned16(x) || !aligned16(enc_img) || !aligned16(dec_img)) return VPC_ERR_ARG;
    if (co->wml != 0.f && !eps_ml) return VPC_ERR_ARG;
    SmallPnArgs a{};
    a.x = x; a.enc_img = enc_img; a.dec_img = dec_img; a.eps_ml = eps_ml; a.partE = partE; a.partD = partD;
    a.loss_part = loss_partials;
    set_loss_coef(a, *co, npass);
    a.inv_B = inv_B; a.x_logvar = x_logvar;
    a.B = B; a.d = d; a.d_real = d_real; a.L = L; a.npass = npass;
    if (pn) a.pn = *pn;
    for (int p = 0; p < npass; ++p) {
        if (!mask[p] || !eps[p]) return VPC_ERR_ARG;
        a.m[p] = mask[p]; a.mB[p] = maskB ? maskB[p] : nullptr; a.eps[p] = eps[p];
        if ((uintptr_t)a.m[p] % 4 || !aligned16(a.eps[p])) return VPC_ERR_ARG;
    }
    for (int p = 0; p < npass; ++p)  // the second loss mask of a pass must be the other pass's mask (as vpc_step_fused_bf16)
        if (a.mB[p] && (npass != 2 || a.mB[p] != a.m[1 - p])) return VPC_ERR_ARG;
    if ((B + 15) / 16 > 2L * num_cus()) return VPC_ERR_SHAPE;  // one workgroup per 16-row tile, at most 2 x CUs partial blocks
    if (dr.on) {
        // eps_out must be the planes the step reads: plane p = eps[p] (and eps_ml the next one), [B][16] each
        if (!dr.eps_out || dr.n_eps < B * 16 || dr.n_eps % (B * 16) || dr.eps_out != eps[0]) return VPC_ERR_ARG;
        if (npass == 2 && (eps[1] != dr.eps_out + B * 16 || dr.n_eps < 2 * B * 16)) return VPC_ERR_ARG;
        if (eps_ml && (eps_ml != dr.eps_out + 2 * B * 16 || dr.n_eps < 3 * B * 16)) return VPC_ERR_ARG;
        if (dr.mask_in && npass != 2) return VPC_ERR_ARG;
        if (dr.mask_elem_lo < 0) return VPC_ERR_ARG;
        a.draw = 1; a.mask_in = dr.mask_in; a.keep_prob = dr.keep_prob; a.eps_out = dr.eps_out; a.n_eps = dr.n_eps;
        a.seed = dr.seed; a.off_mask = dr.off_mask; a.off_eps = dr.off_eps; a.state = dr.state;
        a.mask_elem_lo = dr.mask_elem_lo; a.shard = dr.shard;
    }
    a.ntiles = (int)((B + 15) / 16);
    const int grid = a.ntiles;
    if (nblocks_out) *nblocks_out = grid;
    hipStream_t s = (hipStream_t)stream;
#define VPC_CASE(T)                                                                                        \
    case T: {                                                                                              \
        auto kern = step_small_kernel<T>;                                                                  \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), SMALL_LDS)) return VPC_ERR_HIP;            \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), SMALL_LDS, s, static_cast<const SmallArgs&>(a));   \
        return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;                                     \
    }
#define VPC_CASE_AUG(TI, T)                                                                                \
    case TI: {                                                                                             \
        auto kern = step_small_aug_kernel<TI, T>;                                                          \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), SMALL_LDS)) return VPC_ERR_HIP;            \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), SMALL_LDS, s, static_cast<const SmallArgs&>(a));   \
        return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;                                     \
    }
#define VPC_CASE_PN(TI, T)                                                                                 \
    case 4 * TI + T: {                                                                                     \
        auto kern = step_small_eddi_kernel<TI, T>;                                                         \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), SMALL_LDS)) return VPC_ERR_HIP;            \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), SMALL_LDS, s, a);                              \
        return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;                                     \
    }
    if (pn) {  // (input tiles, output tiles) = (dt_for(K), dt_for(d_real)): K <= 16, 32; d_real <= 16, 32, 64
        switch (4 * dt_for(pn->K) + dt_for(d_real)) {
            VPC_CASE_PN(1, 1) VPC_CASE_PN(1, 2) VPC_CASE_PN(1, 4) VPC_CASE_PN(2, 1) VPC_CASE_PN(2, 2) VPC_CASE_PN(2, 4)
        }
        return VPC_ERR_SHAPE;
    }
    if (aug) {  // (input tiles, output tiles) = (dt_for(2 d_real), dt_for(d_real)): d_real <= 8, 16, 32, 64
        switch (dt_for(2 * d_real)) { VPC_CASE_AUG(1, 1) VPC_CASE_AUG(2, 1) VPC_CASE_AUG(4, 2) VPC_CASE_AUG(8, 4) }
        return VPC_ERR_SHAPE;
    }
    switch (dt_for(d)) { VPC_CASE(1) VPC_CASE(2) VPC_CASE(4) VPC_CASE(8) }
#undef VPC_CASE_PN
#undef VPC_CASE_AUG
#undef VPC_CASE
    return VPC_ERR_SHAPE;
}
}  // namespace vpc

extern "C" int vpc_step_small_f32(const float* x, const float* enc_img, const float* dec_img, int npass,
                                  const uint8_t* const* mask, const uint8_t* const* maskB, const VpcLossCoef* co,
                                  const float* const* eps, const float* eps_ml, float inv_B, float x_logvar, float* partE, float* partD, double* loss_partials,
                                  int* nblocks_out, long B, int d, int L, void* stream) {
    return step_small_launch(x, enc_img, dec_img, npass, mask, maskB, co, eps, eps_ml, inv_B, x_logvar, partE,
                             partD, loss_partials, nblocks_out, B, d, L, SmallDraw{}, stream);
}

// vpc_draw_step + vpc_step_small_f32 in ONE launch: every workgroup draws the mask_p bytes (mask[1] = mask_in & keep, when mask_in !=
// NULL) and the normals of ITS 16 rows - eps_out = eps[0], planes [B][16]: eps[1] and eps_ml follow it; n_eps floats in all - with the
// Philox counters vpc_draw_step would use (seed, offsets, state, mask_elem_lo and the eps_* shard description as there), stores them
// where the step reads them, and runs the step.  Same draws, one launch less at the batch sizes where a launch is a fifth of the step.
extern "C" int vpc_step_small_draw_f32(const float* x, const float* enc_img, const float* dec_img, int npass,
                                       const uint8_t* const* mask, const uint8_t* const* maskB, const VpcLossCoef* co,
                                       const float* const* eps, const float* eps_ml, float inv_B, float x_logvar, float* partE, float* partD, double* loss_partials,
                                       int* nblocks_out, long B, int d, int L, const uint8_t* mask_in, float keep_prob,
                                       float* eps_out, long n_eps, unsigned long long seed, unsigned long long offset_mask,
                                       unsigned long long offset_eps, const long long* state, long mask_elem_lo,
                                       long eps_rows_local, long eps_rows_global, long eps_row_lo, int eps_pitch, void* stream) {
    if (eps_rows_local < 0 || (eps_rows_local > 0 && (eps_pitch != 16 || eps_rows_local != B || eps_row_lo < 0 ||
                                                      eps_row_lo + eps_rows_local > eps_rows_global)))
        return VPC_ERR_ARG;
    SmallDraw dr{1, mask_in, keep_prob, eps_out, n_eps, seed, offset_mask, offset_eps, state, mask_elem_lo,
                 EpsShard{eps_rows_local, eps_rows_global, eps_row_lo, eps_pitch}};
    return step_small_launch(x, enc_img, dec_img, npass, mask, maskB, co, eps, eps_ml, inv_B, x_logvar, partE,
                             partD, loss_partials, nblocks_out, B, d, L, dr, stream);
}

// ------------------------------------------------------------------------------------------------
// Ensemble: G independent models of one architecture in ONE launch (imputation.py:21-39 wraps train.py:28-117 in loops over
// missing rate, alpha and split: many runs of the same tiny model).  Workgroup (t, g) builds member g's SmallArgs - member 0's
// pointers plus g x the member strides, the coefficients / keep probability / seed of record g of the device-resident member
// table - and runs the tile body (vpc_small_body.h) on tile t: the single-model kernel's body, so member g's partial blocks, loss terms and draws
// are bit for bit those of its stand-alone step.
namespace vpc {
struct SmallMultiArgs {
    SmallArgs base;             // member 0's buffers, and everything the members share
    const VpcMember* members;   // [G] records
    long sx, sm, smp, seps, simg, sE, sD, sL;  // member strides in elements (sx / sm 0: one batch shared by all members)
    unsigned G, tiles;
    int order;
};
// The arguments of one member, as the tile body names them (the fields of SmallArgs), built in registers at kernel entry.  The
// per-pass arrays are pairs picked by a select: a struct that lives in registers cannot be indexed with the pass counter (it
// would be demoted to scratch).
template <class T>
struct PassPair {
    T v0, v1;
    __device__ __forceinline__ T operator[](int p) const { return p == 0 ? v0 : v1; }
};
// `How` says how the fields that are read late in the step come about (MemberEarly / MemberLate below).
template <class How>
struct MemberArgsOf {
    const float* x;
    const float* enc_img;
    const float* dec_img;
    PassPair<const uint8_t*> m;
    typename How::MaskB mB;
    PassPair<float> cA, cE;
    typename How::Eps eps;
    typename How::EpsMl eps_ml;
    typename How::PartE partE;
    typename How::PartD partD;
    typename How::LossPart loss_part;
    float bq, bp, cr, wml, inv_B, x_logvar;
    long B;
    int d, L, npass;
    int draw;
    int d_real;  // (read by the mask-augmented and point-net stages only)
    const uint8_t* mask_in;
    float keep_prob;
    float* eps_out; long n_eps;
    unsigned long long seed, off_mask, off_eps;
    const long long* state;
    long mask_elem_lo;
    EpsShard shard;
};
// MemberEarly: every field is a value made at kernel entry.
struct MemberEarly {
    using MaskB = PassPair<const uint8_t*>;
    using Eps = PassPair<const float*>;
    using EpsMl = const float*;
    using PartE = float*;
    using PartD = float*;
    using LossPart = double*;
    template <class A>
    static __device__ __forceinline__ void second_mask(A& a, unsigned, const VpcMember* r) {
        a.mB.v0 = r->use_maskB ? a.m.v1 : nullptr;  // (the E terms' second mask is the other pass's: cE[0] != 0)
        a.mB.v1 = nullptr;
    }
    template <class A>
    static __device__ __forceinline__ void planes_and_blocks(A& a, const SmallMultiArgs& ma, unsigned mem) {
        const SmallArgs& b = ma.base;
        // (the planes of a member follow each other)
        a.eps.v0 = b.eps[0] + mem * ma.seps;
        a.eps.v1 = b.eps[1] ? a.eps.v0 + b.B * 16 : nullptr;
        a.eps_ml = b.eps_ml ? a.eps.v0 + 2 * b.B * 16 : nullptr;
        a.partE = b.partE + mem * ma.sE;
        a.partD = b.partD + mem * ma.sD;
        a.loss_part = b.loss_part + mem * ma.sL;
    }
    template <class A>
    static __device__ __forceinline__ const float* plane0(const A& a, const SmallMultiArgs&, unsigned) { return a.eps.v0; }
};
using MemberArgs = MemberArgsOf<MemberEarly>;
// MemberLate: the fields the tile body reads from the decoder phases on - the eps planes, whether the E terms take the second
// mask, where the partial blocks and the loss terms go - are made WHERE they are read, from the kernel-argument segment and the
// member index.  Made at entry they sit in scalar registers through the encoder forward, the kernels are at the scalar limit
// there, and the compiler parks them in lanes of a vector register it then holds for the whole step: the one register the
// DT = 4 instantiations lack (8 bytes of scratch in step_small_multi_kernel<4>).  A read is made opaque, or it joins the loads
// of the kernel's entry again.  The kernel argument is ONE record at offset 0 of the segment.
template <class T>
__device__ __forceinline__ T kernarg_at(unsigned off) {
    asm volatile("" : "+s"(off));
    typedef const char __attribute__((address_space(4))) SegByte;
    typedef const T __attribute__((address_space(4))) SegT;
    return *(SegT*)((SegByte*)__builtin_amdgcn_kernarg_segment_ptr() + off);
}
template <class T, unsigned BASE, unsigned STRIDE>
struct LatePtr {  // member 0's pointer at BASE of the segment, the member stride (elements) at STRIDE
    unsigned mem;
    __device__ __forceinline__ operator T*() const { return kernarg_at<T*>(BASE) + mem * kernarg_at<long>(STRIDE); }
};
struct MemberLate {
    struct MaskB {  // (the tile body asks only whether there is a second mask: it takes the other pass's)
        unsigned mem;
        __device__ __forceinline__ bool operator[](int p) const {
            typedef const VpcMember __attribute__((address_space(4))) ConstMember;  // (the table is not written during the launch)
            const ConstMember* r = (const ConstMember*)kernarg_at<const VpcMember*>(offsetof(SmallMultiArgs, members));
            return p == 0 && r[mem].use_maskB != 0;
        }
    };
    struct Eps {  // plane p of the member: eps[0] + g x stride + p B 16 (the body reads plane p < npass only)
        unsigned mem;
        __device__ __forceinline__ const float* operator[](int p) const {
            return kernarg_at<const float*>(offsetof(SmallMultiArgs, base.eps)) + mem * kernarg_at<long>(offsetof(SmallMultiArgs, seps)) +
                   p * kernarg_at<long>(offsetof(SmallMultiArgs, base.B)) * 16;
        }
    };
    struct EpsMl {  // the third plane (read only where wml != 0: the host then gave three planes)
        unsigned mem;
        __device__ __forceinline__ operator const float*() const { return Eps{mem}[2]; }
    };
    using PartE = LatePtr<float, offsetof(SmallMultiArgs, base.partE), offsetof(SmallMultiArgs, sE)>;
    using PartD = LatePtr<float, offsetof(SmallMultiArgs, base.partD), offsetof(SmallMultiArgs, sD)>;
    using LossPart = LatePtr<double, offsetof(SmallMultiArgs, base.loss_part), offsetof(SmallMultiArgs, sL)>;
    template <class A>
    static __device__ __forceinline__ void second_mask(A& a, unsigned mem, const VpcMember*) { a.mB.mem = mem; }
    template <class A>
    static __device__ __forceinline__ void planes_and_blocks(A& a, const SmallMultiArgs&, unsigned mem) {
        a.eps.mem = a.eps_ml.mem = a.partE.mem = a.partD.mem = a.loss_part.mem = mem;
    }
    template <class A>
    static __device__ __forceinline__ const float* plane0(const A&, const SmallMultiArgs& ma, unsigned mem) {
        return ma.base.eps[0] + mem * ma.seps;  // (for the draws at kernel entry)
    }
};

template <int DT>
__global__ __launch_bounds__(THREADS) void step_small_multi_kernel(SmallMultiArgs ma) {
    constexpr int DTI = DT;
    constexpr bool AUG = false;
    constexpr bool PN = false;
    constexpr SmallPointNet pnx{};
    using MemberHow = MemberEarly;
#include "vpc_small_member.h"
#include "vpc_small_body.h"
}
// Reg_VAE_mask / vanilla_VAE_mask members: the frame of step_small_multi_kernel around the mask-augmented tile body
// (step_small_aug_kernel's).  ma.base.d_real is the members' obs_dim, ma.base.d the row pitch; the images have the mask-augmented layout.
template <int DTI, int DT>
__global__ __launch_bounds__(THREADS) void step_small_multi_aug_kernel(SmallMultiArgs ma) {
    constexpr bool AUG = true;
    constexpr bool PN = false;
    constexpr SmallPointNet pnx{};
    using MemberHow = MemberLate;
#include "vpc_small_member.h"
#include "vpc_small_body.h"
}

// Reg_EDDI / vanilla_EDDI members: the same frame around the point-net tile body (step_small_eddi_kernel's).  Member g's
// SmallPointNet is built in registers beside its MemberArgs: three pointers and K, named field by field (nothing the pass counter
// indexes, so nothing that would be demoted to scratch).  tile_id is the member's tile: every member's tile 0 leaves ITS snapshot.
struct SmallMultiPnArgs : SmallMultiArgs {
    SmallPointNet pn;     // member 0's front-end parameters, (dA | dC) blocks and snapshot
    long sP, sF, sS;      // member strides of those three, in floats
};
template <int DTI, int DT>
__global__ __launch_bounds__(THREADS) void step_small_multi_eddi_kernel(SmallMultiPnArgs ma) {
    constexpr bool AUG = false;
    constexpr bool PN = true;
    using MemberHow = MemberLate;
#include "vpc_small_member.h"
    SmallPointNet pnx;
    pnx.K = ma.pn.K;
    pnx.front = ma.pn.front + mem * ma.sP;
    pnx.partF = ma.pn.partF + mem * ma.sF;
    pnx.snap = ma.pn.snap + mem * ma.sS;
#include "vpc_small_body.h"
}

// The argument checks and the SmallMultiArgs of the three ensemble step entries.  d_real 0: the plain members (d is obs_dim);
// else d is the row pitch of obs_dim d_real.  Returns VPC_OK with `ma` and `grid` filled, or the refusal.
static int multi_prepare(SmallMultiArgs& ma, dim3& grid, const float* x, const uint8_t* mask, uint8_t* mask_p, float* eps,
                         const float* enc_img, const float* dec_img, const VpcMember* members, int G, int npass, int nplanes,
                         int draw, unsigned long long offset_mask, unsigned long long offset_eps, float inv_B, float x_logvar,
                         float* partE, float* partD, double* loss_partials, const long* strides, long B, int d, int d_real, int L,
                         int order) {
    if (!x || !mask || !eps || !enc_img || !dec_img || !members || !partE || !partD || !loss_partials || !strides) return VPC_ERR_ARG;
    if (G < 1 || npass < 1 || npass > 2 || B <= 0 || order < 0 || order > 1) return VPC_ERR_ARG;
    if (npass == 2 ? (!mask_p || nplanes < 2 || nplanes > 3) : nplanes != 1) return VPC_ERR_ARG;
    if (d < 4 || d > MAX_D || d % 4 || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (!aligned16(x) || !aligned16(enc_img) || !aligned16(dec_img) || !aligned16(eps)) return VPC_ERR_ARG;
    if ((uintptr_t)mask % 4 || (uintptr_t)mask_p % 4) return VPC_ERR_ARG;
    const long tiles = (B + 15) / 16;
    if (tiles > 2L * num_cus() || (long)G * tiles > VPC_MULTI_MAX_BLOCKS) return VPC_ERR_SHAPE;
    const long sx = strides[VPC_MS_X], sm = strides[VPC_MS_MASK], smp = strides[VPC_MS_MASK_P], seps = strides[VPC_MS_EPS],
               simg = strides[VPC_MS_IMG], sE = strides[VPC_MS_PARTE], sD = strides[VPC_MS_PARTD], sL = strides[VPC_MS_LOSS];
    const long nx = B * (long)d, ne = (long)nplanes * B * 16;
    // every member's slice inside its stride, 16-byte (masks: 4-byte) aligned; only read-only inputs may be shared (stride 0)
    if ((sx != 0 && sx < nx) || sx % 4 || (sm != 0 && sm < nx) || sm % 4) return VPC_ERR_ARG;
    if (npass == 2 && ((smp != 0 && smp < nx) || smp % 4 || (draw && smp == 0 && G > 1))) return VPC_ERR_ARG;
    if ((seps != 0 && seps < ne) || seps % 4 || (draw && seps == 0 && G > 1)) return VPC_ERR_ARG;
    if (simg <= 0 || simg % 4) return VPC_ERR_ARG;
    if (sE < tiles * ENC_PART || sE % 4 || sD < tiles * DEC_PART || sD % 4 || sL < tiles * LOSS_TERMS) return VPC_ERR_ARG;
    SmallArgs& a = ma.base;
    a.x = x; a.enc_img = enc_img; a.dec_img = dec_img; a.partE = partE; a.partD = partD; a.loss_part = loss_partials;
    a.inv_B = inv_B; a.x_logvar = x_logvar; a.B = B; a.d = d; a.d_real = d_real; a.L = L; a.npass = npass; a.ntiles = (int)tiles;
    a.m[0] = mask;
    a.eps[0] = eps;
    if (npass == 2) { a.m[1] = mask_p; a.eps[1] = eps + B * 16; }
    if (nplanes == 3) a.eps_ml = eps + 2 * B * 16;
    if (draw) {  // the draws of vpc_step_small_draw_f32 on an unsharded batch: member g with ITS seed, in its own element space
        a.draw = 1; a.mask_in = npass == 2 ? mask : nullptr; a.eps_out = eps; a.n_eps = ne;
        a.off_mask = offset_mask; a.off_eps = offset_eps; a.state = nullptr; a.mask_elem_lo = 0;
        a.shard = EpsShard{B, B, 0, 16};
    }
    ma.members = members;
    ma.sx = sx; ma.sm = sm; ma.smp = smp; ma.seps = seps; ma.simg = simg; ma.sE = sE; ma.sD = sD; ma.sL = sL;
    ma.G = (unsigned)G; ma.tiles = (unsigned)tiles; ma.order = order;
    grid = order == 0 ? dim3((unsigned)tiles, (unsigned)G) : dim3((unsigned)(8 * tiles), (unsigned)((G + 7) / 8));
    return VPC_OK;
}
}  // namespace vpc

#define VPC_MULTI_LAUNCH(KERN, ARGS)                                                                       \
    {                                                                                                      \
        auto kern = KERN;                                                                                  \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), SMALL_LDS)) return VPC_ERR_HIP;            \
        hipLaunchKernelGGL(kern, grid, dim3(THREADS), SMALL_LDS, (hipStream_t)stream, ARGS);               \
        return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;                                     \
    }

extern "C" int vpc_step_small_multi_f32(const float* x, const uint8_t* mask, uint8_t* mask_p, float* eps, const float* enc_img,
                                        const float* dec_img, const VpcMember* members, int G, int npass, int nplanes, int draw,
                                        unsigned long long offset_mask, unsigned long long offset_eps, float inv_B,
                                        float x_logvar, float* partE, float* partD, double* loss_partials, const long* strides,
                                        long B, int d, int L, int order, void* stream) {
    SmallMultiArgs ma{};
    dim3 grid;
    if (const int rc = multi_prepare(ma, grid, x, mask, mask_p, eps, enc_img, dec_img, members, G, npass, nplanes, draw, offset_mask,
                                     offset_eps, inv_B, x_logvar, partE, partD, loss_partials, strides, B, d, 0, L, order))
        return rc;
    switch (dt_for(d)) {
        case 1: VPC_MULTI_LAUNCH(step_small_multi_kernel<1>, ma)
        case 2: VPC_MULTI_LAUNCH(step_small_multi_kernel<2>, ma)
        case 4: VPC_MULTI_LAUNCH(step_small_multi_kernel<4>, ma)
        case 8: VPC_MULTI_LAUNCH(step_small_multi_kernel<8>, ma)
    }
    return VPC_ERR_SHAPE;
}

// The ensemble step for G Reg_VAE_mask / vanilla_VAE_mask members (vpc_step_small_aug(_draw)_f32 per member): d is the row pitch
// 4 ceil(d_real / 4) of x and the masks - the pitch the draws are made at -, the images are those of the mask-augmented layout.
extern "C" int vpc_step_small_multi_aug_f32(const float* x, const uint8_t* mask, uint8_t* mask_p, float* eps, const float* enc_img,
                                            const float* dec_img, const VpcMember* members, int G, int npass, int nplanes, int draw,
                                            unsigned long long offset_mask, unsigned long long offset_eps, float inv_B,
                                            float x_logvar, float* partE, float* partD, double* loss_partials, const long* strides,
                                            long B, int d, int d_real, int L, int order, void* stream) {
    // (the shape limits of step_small_launch's mask-augmented branch)
    if (d_real < 1 || d_real > d || d - d_real > 3 || 2 * d_real > MAX_D) return VPC_ERR_SHAPE;
    SmallMultiArgs ma{};
    dim3 grid;
    if (const int rc = multi_prepare(ma, grid, x, mask, mask_p, eps, enc_img, dec_img, members, G, npass, nplanes, draw, offset_mask,
                                     offset_eps, inv_B, x_logvar, partE, partD, loss_partials, strides, B, d, d_real, L, order))
        return rc;
    switch (dt_for(2 * d_real)) {
        case 1: VPC_MULTI_LAUNCH((step_small_multi_aug_kernel<1, 1>), ma)
        case 2: VPC_MULTI_LAUNCH((step_small_multi_aug_kernel<2, 1>), ma)
        case 4: VPC_MULTI_LAUNCH((step_small_multi_aug_kernel<4, 2>), ma)
        case 8: VPC_MULTI_LAUNCH((step_small_multi_aug_kernel<8, 4>), ma)
    }
    return VPC_ERR_SHAPE;
}

// The ensemble step for G Reg_EDDI / vanilla_EDDI members (vpc_step_small_eddi(_draw)_f32 per member): images of the point-net
// layout; front / front_partials / front_snapshot are member 0's, member g's lie strides[VPC_MS_PARAM] / [VPC_MS_PARTF] /
// [VPC_MS_SNAP] floats further (`front` sits inside the member's row of the parameter stack, behind trunk and decoder).
extern "C" int vpc_step_small_multi_eddi_f32(const float* x, const uint8_t* mask, uint8_t* mask_p, float* eps, const float* enc_img,
                                             const float* dec_img, const VpcMember* members, int G, int npass, int nplanes, int draw,
                                             unsigned long long offset_mask, unsigned long long offset_eps, float inv_B,
                                             float x_logvar, float* partE, float* partD, double* loss_partials, const long* strides,
                                             long B, int d, int d_real, int L, int K, const float* front, float* front_partials,
                                             float* front_snapshot, int order, void* stream) {
    // (the shape limits of step_small_launch's point-net branch, and its pointer checks)
    if (d_real < 1 || d_real > d || d - d_real > 3 || d > 64 || K < 1 || K > 32) return VPC_ERR_SHAPE;
    if (!front || !front_partials || !front_snapshot || (uintptr_t)front % 4 || (uintptr_t)front_partials % 4 ||
        (uintptr_t)front_snapshot % 4)
        return VPC_ERR_ARG;
    SmallMultiPnArgs ma{};
    dim3 grid;
    if (const int rc = multi_prepare(ma, grid, x, mask, mask_p, eps, enc_img, dec_img, members, G, npass, nplanes, draw, offset_mask,
                                     offset_eps, inv_B, x_logvar, partE, partD, loss_partials, strides, B, d, d_real, L, order))
        return rc;
    const long nfront = (long)d_real * K + d_real + (long)K * (2 + K) + K;
    ma.pn = SmallPointNet{K, front, front_partials, front_snapshot};
    ma.sP = strides[VPC_MS_PARAM]; ma.sF = strides[VPC_MS_PARTF]; ma.sS = strides[VPC_MS_SNAP];
    // the blocks and the snapshot are written by every member: never shared; the parameters are read here, but every member has its own row
    if (ma.sP < nfront || ma.sF < (long)ma.tiles * 2 * K * d || ma.sS < nfront) return VPC_ERR_ARG;
    switch (4 * dt_for(K) + dt_for(d_real)) {
        case 4 * 1 + 1: VPC_MULTI_LAUNCH((step_small_multi_eddi_kernel<1, 1>), ma)
        case 4 * 1 + 2: VPC_MULTI_LAUNCH((step_small_multi_eddi_kernel<1, 2>), ma)
        case 4 * 1 + 4: VPC_MULTI_LAUNCH((step_small_multi_eddi_kernel<1, 4>), ma)
        case 4 * 2 + 1: VPC_MULTI_LAUNCH((step_small_multi_eddi_kernel<2, 1>), ma)
        case 4 * 2 + 2: VPC_MULTI_LAUNCH((step_small_multi_eddi_kernel<2, 2>), ma)
        case 4 * 2 + 4: VPC_MULTI_LAUNCH((step_small_multi_eddi_kernel<2, 4>), ma)
    }
    return VPC_ERR_SHAPE;
}
#undef VPC_MULTI_LAUNCH

// The same step for Reg_VAE_mask / vanilla_VAE_mask (src/models/VAE.py:545-555, 1031-1041; src/experiment_main/train.py:87-115):
// encoder input [x*mask | mask] of width 2 d_real built in the kernel's input stage, images of the mask-augmented layout.  d is the
// row pitch of x and the masks, 4 ceil(d_real / 4), with mask 0 in the padding.
extern "C" int vpc_step_small_aug_f32(const float* x, const float* enc_img, const float* dec_img, int npass,
                                      const uint8_t* const* mask, const uint8_t* const* maskB, const VpcLossCoef* co,
                                      const float* const* eps, const float* eps_ml, float inv_B, float x_logvar, float* partE, float* partD, double* loss_partials,
                                      int* nblocks_out, long B, int d, int d_real, int L, void* stream) {
    if (d_real < 1) return VPC_ERR_SHAPE;
    return step_small_launch(x, enc_img, dec_img, npass, mask, maskB, co, eps, eps_ml, inv_B, x_logvar, partE,
                             partD, loss_partials, nblocks_out, B, d, L, SmallDraw{}, stream, d_real);
}

extern "C" int vpc_step_small_aug_draw_f32(const float* x, const float* enc_img, const float* dec_img, int npass,
                                           const uint8_t* const* mask, const uint8_t* const* maskB, const VpcLossCoef* co,
                                           const float* const* eps, const float* eps_ml, float inv_B, float x_logvar, float* partE, float* partD, double* loss_partials,
                                           int* nblocks_out, long B, int d, int d_real, int L, const uint8_t* mask_in, float keep_prob,
                                           float* eps_out, long n_eps, unsigned long long seed, unsigned long long offset_mask,
                                           unsigned long long offset_eps, const long long* state, long mask_elem_lo,
                                           long eps_rows_local, long eps_rows_global, long eps_row_lo, int eps_pitch, void* stream) {
    if (d_real < 1) return VPC_ERR_SHAPE;
    if (eps_rows_local < 0 || (eps_rows_local > 0 && (eps_pitch != 16 || eps_rows_local != B || eps_row_lo < 0 ||
                                                      eps_row_lo + eps_rows_local > eps_rows_global)))
        return VPC_ERR_ARG;
    SmallDraw dr{1, mask_in, keep_prob, eps_out, n_eps, seed, offset_mask, offset_eps, state, mask_elem_lo,
                 EpsShard{eps_rows_local, eps_rows_global, eps_row_lo, eps_pitch}};
    return step_small_launch(x, enc_img, dec_img, npass, mask, maskB, co, eps, eps_ml, inv_B, x_logvar, partE,
                             partD, loss_partials, nblocks_out, B, d, L, dr, stream, d_real);
}

// The same step for Reg_EDDI / vanilla_EDDI (src/models/VAE.py:713-741, 897-925 encoder; src/experiment_main/train.py:87-115): the
// images are those of the point-net layout (vpc_build_indices_pointnet: trunk K -> 100 -> 50 -> 2L, decoder L -> 50 -> 100 -> d_real),
// `front` the front-end parameters in flat order (type_pars1 | type_bias1 | pnp_encoder1.0.weight | .bias), read and folded by every
// workgroup.  Besides partE / partD the tiles write their (dA | dC) blocks [2][K][d] to front_partials and tile 0 a copy of `front`
// to front_snapshot (what vpc_reduce_step_adam_eddi's chain rule reads).  d is the row pitch 4 ceil(d_real / 4) of x and the masks.
extern "C" int vpc_step_small_eddi_f32(const float* x, const float* enc_img, const float* dec_img, int npass,
                                       const uint8_t* const* mask, const uint8_t* const* maskB, const VpcLossCoef* co,
                                       const float* const* eps, const float* eps_ml, float inv_B, float x_logvar, float* partE, float* partD, double* loss_partials,
                                       int* nblocks_out, long B, int d, int d_real, int L, int K, const float* front,
                                       float* front_partials, float* front_snapshot, void* stream) {
    if (d_real < 1) return VPC_ERR_SHAPE;
    const SmallPointNet pn{K, front, front_partials, front_snapshot};
    return step_small_launch(x, enc_img, dec_img, npass, mask, maskB, co, eps, eps_ml, inv_B, x_logvar, partE,
                             partD, loss_partials, nblocks_out, B, d, L, SmallDraw{}, stream, d_real, &pn);
}

extern "C" int vpc_step_small_eddi_draw_f32(const float* x, const float* enc_img, const float* dec_img, int npass,
                                            const uint8_t* const* mask, const uint8_t* const* maskB, const VpcLossCoef* co,
                                            const float* const* eps, const float* eps_ml, float inv_B, float x_logvar, float* partE, float* partD, double* loss_partials,
                                            int* nblocks_out, long B, int d, int d_real, int L, int K, const float* front,
                                            float* front_partials, float* front_snapshot, const uint8_t* mask_in, float keep_prob,
                                            float* eps_out, long n_eps, unsigned long long seed, unsigned long long offset_mask,
                                            unsigned long long offset_eps, const long long* state, long mask_elem_lo,
                                            long eps_rows_local, long eps_rows_global, long eps_row_lo, int eps_pitch, void* stream) {
    if (d_real < 1) return VPC_ERR_SHAPE;
    if (eps_rows_local < 0 || (eps_rows_local > 0 && (eps_pitch != 16 || eps_rows_local != B || eps_row_lo < 0 ||
                                                      eps_row_lo + eps_rows_local > eps_rows_global)))
        return VPC_ERR_ARG;
    const SmallPointNet pn{K, front, front_partials, front_snapshot};
    SmallDraw dr{1, mask_in, keep_prob, eps_out, n_eps, seed, offset_mask, offset_eps, state, mask_elem_lo,
                 EpsShard{eps_rows_local, eps_rows_global, eps_row_lo, eps_pitch}};
    return step_small_launch(x, enc_img, dec_img, npass, mask, maskB, co, eps, eps_ml, inv_B, x_logvar, partE,
                             partD, loss_partials, nblocks_out, B, d, L, dr, stream, d_real, &pn);
}
