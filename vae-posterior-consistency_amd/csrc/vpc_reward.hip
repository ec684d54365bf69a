// Active-variable-selection reward (BASELINE config 5), gfx950.
//
// Reference: R_lindley_chain / chaini_I / chaini_II, src/experiment_main/evaluate.py:514-634, driven by the
// candidate loop of active_learning_func (evaluate.py:424-433):  for every row n, candidate feature u (not yet
// observed) and MC imputation m
//     R[n][u] = 1/M sum_m [ KL_I(n,u,m) - KL_II(n,u,m) ],
//     KL_*  = 0.5 sum_L ( (mu_b - mu_a)^2 / exp(lv_a / 2) + exp(lv_b) / exp(lv_a) - 1 - lv_b + lv_a )      (sic: std)
// where (a, b) are two encoder calls that differ by revealing feature u (and, for KL_II, the target column in
// both).  The reference issues 4 * (d-1) * M encoder calls per acquisition step; here
//   * the "a" encodings do not depend on u      -> computed once per (n, m)   (mode A of the chain kernel)
//   * every encoding differs from the row's base encoding by a rank-1 update of the first layer
//       h1pre = W1 (x * mask) + b1 + W1[:,u] * im[m][n][u] (+ W1[:,T] * delta_T)
//     so layer 1 is an FMA per hidden unit and only layers 2-3 (100 -> 50 -> 2L) run on the matrix cores,
//     register-chained exactly like the training kernels (vpc_device.h), 16 MC samples per MFMA column tile,
//     two chains (I and II) per weight fragment.
//
// The first layer comes in three kinds (template parameter KIND; include/vpc.h VPC_REWARD_*), layers 2-3 and the KL
// epilogue are shared:
//   DENSE       Reg_VAE / vanilla_VAE (VAE.py:366-395), any input width: the update of candidate u is W1[:,u] * im_u.
//   DENSE_MASK  Reg_VAE_mask / vanilla_VAE_mask (input [x*mask | mask], VAE.py:545-548): revealing u also sets its mask
//               input, so the update gains the constant W1[:,d+u] (a second transposed table), and chain II's revealed
//               target gains W1[:,d+T] * (1 - mask_T).
//   POINTNET    Reg_EDDI / vanilla_EDDI (VAE.py:713-741): agg = sum_j mask_j relu(x_j A_j + C_j) (A | C folded by
//               vpc_eddi_fold), h1pre = W1 agg + b1 with W1 = pnp_encoder2.0 [100][K].  Revealing u adds
//               relu(im_u A_u + C_u) to agg, so the update is W1 relu(im_u A_u + C_u): ceil(K/4) MFMA k-steps per h1
//               tile, each lane building its B value with one FMA and one max.  Prep evaluates the base agg per
//               (n, m, chain), target adjustments included, and W1 agg + b1.
//
// The plain model at d <= 128 also runs with a member dimension (vpc_reward_matrix_multi: blockIdx.y = member, the kernel bodies of
// vpc_reward_prep_body.h / vpc_reward_chain_body.h on the member's operands), followed by the acquisition itself
// (acquire_multi_kernel: argmax per row, mask byte, action; evaluate.py:435-440): the loop of G models without a host round trip.
// The DENSE_MASK and POINTNET kinds have the member dimension too, within the widths of their members' forward kernels
// (vpc_reward_matrix_multi_ex: reward_prep_multi_kind_kernel / reward_chain_multi_kind_kernel).
#include "vpc_device.h"
#include "vpc_abi_internal.h"

namespace vpc {

constexpr int RW_WAVES = 4, RW_THREADS = RW_WAVES * 64;
constexpr int STAT = 64;  // floats per (n, m): [chain I | chain II] x [mean tile 16 | logvar tile 16]
constexpr int RK_DENSE = VPC_REWARD_DENSE, RK_DENSE_MASK = VPC_REWARD_DENSE_MASK, RK_POINTNET = VPC_REWARD_POINTNET;
constexpr int W23_FLOATS = H2P * 128 + 32 * 64;  // [W2 | W3] of the encoder image (EncImg oW2 .. total): the same for every d
constexpr int PN_MAX_K = 32;                     // point-net width (EDDI_MAX_K of vpc_eddi.hip)
constexpr int PN_FRAG = H1T * 64 * 4;            // floats of the W1 A fragments of one 16-wide group of K (four k-steps)
constexpr int RW_MAX_D = 4096;                   // input columns of the generalised entry (the models' obs_dim limit)

// ---- prep: base first-layer pre-activations per (n, m) and chain, and the first layer's update tables
//   pre[n][m][chain][112]: chain 0 (I) = base + W1[:,T] * mask_T * (xT_carry(m) - x_T),   xT_carry(0) = x_T,
//                                         xT_carry(m) = im[m-1][n][T]   (temp_x[loc,-1] is not reset, evaluate.py:531-536)
//                          chain 1 (II) = base + W1[:,T] * (im[m][n][T] - x_T * mask_T)  [+ W1[:,d+T] * (1 - mask_T)]
//   (POINTNET: W1 (agg_X + mask_T relu(xT_carry(m) A_T + C_T)) + b1 and W1 (agg_X + relu(im[m][n][T] A_T + C_T)) + b1,
//   agg_X = the sum over the observed features other than the target)
//   hidden unit f sits at position pos1_full(f) of the 112-wide rows (vpc_layout.h); unit 100 is the constant 1 of the
//   bias chain, the padding positions are 0.
//   WIDE: any number of input columns (128-column chunks); !WIDE is the d <= 128 form of the plain model.
template <int KIND, bool WIDE>
__global__ __launch_bounds__(128) void reward_prep_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                          const float* __restrict__ im, const float* __restrict__ W1,
                                                          const float* __restrict__ b1, const float* __restrict__ AC,
                                                          float* __restrict__ pre, float* __restrict__ W1T,
                                                          int* __restrict__ cand, float* __restrict__ R, int n, int d,
                                                          int M, int Mp, int K) {
#include "vpc_reward_prep_body.h"
}

struct RewardArgs {
    const float* w23;     // [W2 | W3] of a packed encoder image (W23_FLOATS)
    const float* pre;     // [n][Mp][2][112]
    const float* W1T;     // DENSE [d][112]; DENSE_MASK [2][d][112] (x half, mask half); POINTNET the W1 fragments [2][7][64][4]
    const float* AC;      // POINTNET: the folded front-end [2][K][d] (vpc_eddi_fold)
    const float* im;      // [M][n][d]
    const uint8_t* mask;  // [n][d]
    const int* cand;      // [n][d]: count, then the row's candidate features (reward_prep_kernel)
    int* next_item;       // MODE 1 work counter (zeroed by reward_prep_kernel)
    float* stat;          // [n][Mp][64]
    float* R;             // [n][d-1]
    int n, d, L, M, Mp, K;
};

// MODE 0 (A): items = rows; writes stat[n][m] = {mean_I, logvar_I, mean_II, logvar_II} (16-float tiles).  The A encodings have
//             no update: every kind runs the DENSE instantiation of this mode.
// MODE 1 (B): items = (row, chunk of RW_CH candidates); reads stat, writes R.  A chunk's (candidate, sample) pairs are FLATTENED
// into 16-column MFMA tiles: column c of tile t is pair f = 16 t + c -> candidate f / M, sample f % M.  (Per candidate the M
// samples padded to a multiple of 16 issued 64 columns for M = 50 - 22 % of the matrix work on padding, 50 % at M = 8; a full
// chunk of 8 candidates x 50 samples is exactly 25 tiles.)
constexpr int RW_CH = 4;
template <int KIND, int MODE>
__global__ __launch_bounds__(RW_THREADS) void reward_chain_kernel(RewardArgs a) {
#include "vpc_reward_chain_body.h"
}

// ---- the member dimension (plain model, d <= 128): blockIdx.y = member, every operand of member g `g * stride` elements after
// member 0's (stride 0: shared).  A workgroup serves ONE member - its LDS holds that member's [W2 | W3] - and runs the bodies above
// on the member's operands with its own candidate lists and work counter, so R[g] is what vpc_reward_matrix gives on them.
struct RewardMultiArgs {
    const float *x, *im, *W1, *b1, *w23;
    const uint8_t* mask;
    float *pre, *stat, *w1t, *R;
    long sx, sm, sim, sparam, simg, spre, sstat, sw1t, sR;
    int n, d, L, M, Mp;
};

// table: floats of the kind's first-layer table at the head of a member's w1t slice (reward_table_floats); AC, K: the member's
// folded front-end (POINTNET; null / 0 elsewhere)
__device__ __forceinline__ RewardArgs reward_member_args(const RewardMultiArgs& m, unsigned g, long table, const float* AC,
                                                         int K) {
    float* w1t = m.w1t + g * m.sw1t;
    int* cand = reinterpret_cast<int*>(w1t + table);
    return RewardArgs{m.w23 + g * m.simg, m.pre + g * m.spre, w1t, AC, m.im + g * m.sim, m.mask + g * m.sm, cand,
                      cand + (long)m.n * m.d, m.stat + g * m.sstat, m.R + g * m.sR, m.n, m.d, m.L, m.M, m.Mp, K};
}

__global__ __launch_bounds__(128) void reward_prep_multi_kernel(RewardMultiArgs m) {
    constexpr int KIND = RK_DENSE;
    constexpr bool WIDE = false;
    const unsigned g = blockIdx.y;
    const float* __restrict__ x = m.x + g * m.sx;
    const uint8_t* __restrict__ mask = m.mask + g * m.sm;
    const float* __restrict__ im = m.im + g * m.sim;
    const float* __restrict__ W1 = m.W1 + g * m.sparam;
    const float* __restrict__ b1 = m.b1 + g * m.sparam;
    const float* __restrict__ AC = nullptr;
    float* __restrict__ pre = m.pre + g * m.spre;
    float* __restrict__ W1T = m.w1t + g * m.sw1t;
    int* __restrict__ cand = reinterpret_cast<int*>(W1T + (long)m.d * H1P);
    float* __restrict__ R = m.R + g * m.sR;
    const int n = m.n, d = m.d, M = m.M, Mp = m.Mp, K = 0;
#include "vpc_reward_prep_body.h"
}

template <int MODE>
__global__ __launch_bounds__(RW_THREADS) void reward_chain_multi_kernel(RewardMultiArgs m) {
    constexpr int KIND = RK_DENSE;
    const RewardArgs a = reward_member_args(m, blockIdx.y, (long)m.d * H1P, nullptr, 0);
#include "vpc_reward_chain_body.h"
}

// ---- the member dimension for the other first-layer kinds (DENSE_MASK at 2 d <= 128, POINTNET at d <= 64): the same two wrappers
// with the kind as a template parameter and the instantiation choice of reward_launch - WIDE prep, mode 0 always RK_DENSE, mode 1
// the kind's - so that R[g] is what vpc_reward_matrix_ex gives on member g's operands.  m.w23 is member 0's [W2 | W3] (not an
// encoder image), m.W1 / m.b1 the kind's first layer ([100][2 d] / [100][K]); AC: member 0's folded front-end [2][K][d], sAC apart.
// (Kernels of their own, not a KIND parameter on the two above: the plain pair keeps its symbols and its instructions.)
struct RewardMultiKindArgs {
    RewardMultiArgs m;
    const float* AC;
    long sAC;
    int K;
};

// floats of a kind's first-layer table at the head of w1t: W1^T [d][112], its two halves, or the W1 fragments of two groups of K
__host__ __device__ constexpr long reward_table(int kind, int d) {
    return kind == RK_DENSE ? (long)d * H1P : kind == RK_DENSE_MASK ? 2L * d * H1P : 2L * PN_FRAG;
}

template <int KIND>
__global__ __launch_bounds__(128) void reward_prep_multi_kind_kernel(RewardMultiKindArgs ma) {
    constexpr bool WIDE = true;
    const RewardMultiArgs& m = ma.m;
    const unsigned g = blockIdx.y;
    const float* __restrict__ x = m.x + g * m.sx;
    const uint8_t* __restrict__ mask = m.mask + g * m.sm;
    const float* __restrict__ im = m.im + g * m.sim;
    const float* __restrict__ W1 = m.W1 + g * m.sparam;
    const float* __restrict__ b1 = m.b1 + g * m.sparam;
    const float* __restrict__ AC = KIND == RK_POINTNET ? ma.AC + g * ma.sAC : nullptr;
    float* __restrict__ pre = m.pre + g * m.spre;
    float* __restrict__ W1T = m.w1t + g * m.sw1t;
    int* __restrict__ cand = reinterpret_cast<int*>(W1T + reward_table(KIND, m.d));
    float* __restrict__ R = m.R + g * m.sR;
    const int n = m.n, d = m.d, M = m.M, Mp = m.Mp, K = ma.K;
#include "vpc_reward_prep_body.h"
}

// (three waves per SIMD asked for in the point-net MODE 1: the launch holds three workgroups per CU, and without the hint that
// instantiation takes 152 + 36 registers, two waves per SIMD, where reward_chain_kernel<RK_POINTNET, 1> takes 117 + 36)
template <int FKIND, int MODE>
__global__ __launch_bounds__(RW_THREADS, (FKIND == RK_POINTNET && MODE == 1) ? 3 : 1) void reward_chain_multi_kind_kernel(
    RewardMultiKindArgs ma) {
    // MODE 0 runs the body as RK_DENSE for every kind (reward_chain_kernel); the candidate lists and the work counter lie behind
    // the table of the member's kind in both modes
    constexpr int KIND = MODE == 0 ? RK_DENSE : FKIND;
    const RewardArgs a = reward_member_args(ma.m, blockIdx.y, reward_table(FKIND, ma.m.d),
                                            FKIND == RK_POINTNET ? ma.AC + blockIdx.y * ma.sAC : nullptr, ma.K);
#include "vpc_reward_chain_body.h"
}

// ---- acquire: per (member, row) the lowest index among the maxima of R[g][row][0..d-1) (torch.argmax on finite input; evaluate.py:
// 435-440), revealed in the member's mask(s) and written to the step's slot of the action history.  One wave per row.
struct AcquireArgs {
    const float* R;
    uint8_t *mask, *mask2;  // [n][pitch] bytes; mask2 (may be NULL): the same mask at a second row pitch
    int* action;            // member 0's slot of row 0; rows a_pitch ints apart
    long sR, sm, sm2, sa;
    int n, d, pitch, pitch2, a_pitch;
};

__global__ __launch_bounds__(RW_THREADS) void acquire_multi_kernel(AcquireArgs a) {
    const unsigned g = blockIdx.y;
    const int lane = threadIdx.x & 63, row = blockIdx.x * RW_WAVES + (threadIdx.x >> 6);
    if (row >= a.n) return;
    const int T = a.d - 1;
    const float* r = a.R + g * a.sR + (long)row * T;
    float best = -INFINITY;
    int bi = T;
    for (int u = lane; u < T; u += 64) {  // (ascending: the first of equal values stays)
        const float v = r[u];
        if (v > best) { best = v; bi = u; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (bi >= T) bi = 0;  // (no value above -inf: argmax's answer, and never an index outside the row)
    if (lane == 0) {
        a.mask[g * a.sm + (long)row * a.pitch + bi] = 1;
        if (a.mask2) a.mask2[g * a.sm2 + (long)row * a.pitch2 + bi] = 1;
        a.action[g * a.sa + (long)row * a.a_pitch] = bi;
    }
}

}  // namespace vpc

using namespace vpc;

namespace {
// the three launches of one reward matrix; the caller has checked the arguments
template <int KIND, bool WIDE>
int reward_launch(const float* x, const uint8_t* mask, const float* im, const float* W1, const float* b1, const float* AC, int K,
                  const float* w23, float* pre, float* stat, float* w1t, float* R, int n, int d, int L, int M, hipStream_t s) {
    const int Mp = (M + 15) / 16 * 16;
    const long table = KIND == RK_DENSE ? (long)d * H1P : KIND == RK_DENSE_MASK ? 2L * d * H1P : 2L * PN_FRAG;
    int* cand = reinterpret_cast<int*>(w1t + table);
    const int tail_blocks = KIND == RK_POINTNET ? 1 : (d + 7) / 8;
    hipLaunchKernelGGL((reward_prep_kernel<KIND, WIDE>), dim3(n + tail_blocks), dim3(128), 0, s, x, mask, im, W1, b1, AC, pre,
                       w1t, cand, R, n, d, M, Mp, K);
    RewardArgs a{w23, pre, w1t, AC, im, mask, cand, cand + (long)n * d, stat, R, n, d, L, M, Mp, K};
    const size_t ldsA = sizeof(float) * W23_FLOATS;
    const size_t ldsB = ldsA + (KIND == RK_POINTNET ? sizeof(float) * ((K + 15) / 16 * PN_FRAG) : 0);
    const int cap = num_cus() * 3;  // (2 and 4 - 6 resident workgroups per CU measured slower)
    int gA = (n + RW_WAVES - 1) / RW_WAVES;
    if (gA > cap) gA = cap;
    long itemsB = (long)n * ((d - 1 + RW_CH - 1) / RW_CH);
    int gB = (int)((itemsB + RW_WAVES - 1) / RW_WAVES < cap ? (itemsB + RW_WAVES - 1) / RW_WAVES : cap);
    if (!lds_attr_done(reinterpret_cast<const void*>(reward_chain_kernel<RK_DENSE, 0>), ldsA)) return VPC_ERR_HIP;
    if (!lds_attr_done(reinterpret_cast<const void*>(reward_chain_kernel<KIND, 1>), ldsB)) return VPC_ERR_HIP;
    hipLaunchKernelGGL((reward_chain_kernel<RK_DENSE, 0>), dim3(gA), dim3(RW_THREADS), ldsA, s, a);
    hipLaunchKernelGGL((reward_chain_kernel<KIND, 1>), dim3(gB), dim3(RW_THREADS), ldsB, s, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

long reward_table_floats(int kind, int d) { return reward_table(kind, d); }
}  // namespace

// Scratch sizes (floats) the caller must provide for vpc_reward_matrix.
extern "C" int vpc_reward_scratch(int n, int d, int M, long* pre_floats, long* stat_floats, long* w1t_floats) {
    if (n <= 0 || d < 2 || d > MAX_D || M <= 0) return VPC_ERR_ARG;
    const long Mp = (M + 15) / 16 * 16;
    if (pre_floats) *pre_floats = (long)n * Mp * 2 * H1P;
    if (stat_floats) *stat_floats = (long)n * Mp * STAT;
    if (w1t_floats) *w1t_floats = (long)d * H1P + (long)n * d + 4;  // W1^T, the rows' candidate lists (ints), a work counter
    return VPC_OK;
}

extern "C" int vpc_reward_matrix(const float* x, const uint8_t* mask, const float* im, const float* W1, const float* b1,
                                 const float* enc_img, float* pre, float* stat, float* w1t, float* R, int n, int d, int L,
                                 int M, void* stream) {
    if (!x || !mask || !im || !W1 || !b1 || !enc_img || !pre || !stat || !w1t || !R) return VPC_ERR_ARG;
    if (n <= 0 || M <= 0) return VPC_ERR_ARG;
    if (d < 2 || d > MAX_D || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (!aligned16(pre) || !aligned16(stat) || !aligned16(w1t)) return VPC_ERR_ARG;
    return reward_launch<RK_DENSE, false>(x, mask, im, W1, b1, nullptr, 0, enc_img + EncImg(dt_for(d)).oW2, pre, stat, w1t, R,
                                          n, d, L, M, (hipStream_t)stream);
}

extern "C" int vpc_reward_scratch_ex(int kind, int n, int d, int M, int K, long* pre_floats, long* stat_floats,
                                     long* w1t_floats) {
    if (kind < RK_DENSE || kind > RK_POINTNET || n <= 0 || d < 2 || d > RW_MAX_D || M <= 0) return VPC_ERR_ARG;
    if (kind == RK_POINTNET && (K < 1 || K > PN_MAX_K)) return VPC_ERR_ARG;
    const long Mp = (M + 15) / 16 * 16;
    if (pre_floats) *pre_floats = (long)n * Mp * 2 * H1P;
    if (stat_floats) *stat_floats = (long)n * Mp * STAT;
    if (w1t_floats) *w1t_floats = reward_table_floats(kind, d) + (long)n * d + 4;  // table, candidate lists, work counter
    return VPC_OK;
}

extern "C" int vpc_reward_matrix_ex(int kind, const float* x, const uint8_t* mask, const float* im, const float* W1,
                                    const float* b1, const float* AC, int K, const float* w23_img, float* pre, float* stat,
                                    float* w1t, float* R, int n, int d, int L, int M, void* stream) {
    if (!x || !mask || !im || !W1 || !b1 || !w23_img || !pre || !stat || !w1t || !R) return VPC_ERR_ARG;
    if (kind < RK_DENSE || kind > RK_POINTNET || n <= 0 || M <= 0) return VPC_ERR_ARG;
    if (d < 2 || d > RW_MAX_D || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (kind == RK_POINTNET && (!AC || K < 1 || K > PN_MAX_K)) return VPC_ERR_SHAPE;
    if (!aligned16(pre) || !aligned16(stat) || !aligned16(w1t) || !aligned16(w23_img)) return VPC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (kind == RK_DENSE_MASK)
        return reward_launch<RK_DENSE_MASK, true>(x, mask, im, W1, b1, nullptr, 0, w23_img, pre, stat, w1t, R, n, d, L, M, s);
    if (kind == RK_POINTNET)
        return reward_launch<RK_POINTNET, true>(x, mask, im, W1, b1, AC, K, w23_img, pre, stat, w1t, R, n, d, L, M, s);
    if (d <= MAX_D)  // the plain path's own instantiation
        return reward_launch<RK_DENSE, false>(x, mask, im, W1, b1, nullptr, 0, w23_img, pre, stat, w1t, R, n, d, L, M, s);
    return reward_launch<RK_DENSE, true>(x, mask, im, W1, b1, nullptr, 0, w23_img, pre, stat, w1t, R, n, d, L, M, s);
}

// ---- member dimension ------------------------------------------------------------------------------------------------------------
// Workspace floats PER MEMBER (each a multiple of 4, so that member slices stay 16-byte aligned).
extern "C" int vpc_reward_scratch_multi(int n, int d, int M, long* pre_floats, long* stat_floats, long* w1t_floats) {
    long w1t = 0;
    const int rc = vpc_reward_scratch(n, d, M, pre_floats, stat_floats, &w1t);
    if (rc != VPC_OK) return rc;
    if (w1t_floats) *w1t_floats = (w1t + 3) / 4 * 4;
    return VPC_OK;
}

extern "C" int vpc_reward_matrix_multi(const float* x, const uint8_t* mask, const float* im, const float* W1, const float* b1,
                                       const float* enc_img, float* pre, float* stat, float* w1t, float* R, int G, int chunk,
                                       const long* strides, int n, int d, int L, int M, void* stream) {
    if (!x || !mask || !im || !W1 || !b1 || !enc_img || !pre || !stat || !w1t || !R || !strides) return VPC_ERR_ARG;
    if (n <= 0 || M <= 0 || G < 1 || chunk < 1 || chunk > 65535) return VPC_ERR_ARG;
    if (d < 2 || d > MAX_D || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (!aligned16(pre) || !aligned16(stat) || !aligned16(w1t) || !aligned16(enc_img)) return VPC_ERR_ARG;
    const long Mp = (M + 15) / 16 * 16, nd = (long)n * d;
    const long sx = strides[VPC_RM_X], sm = strides[VPC_RM_MASK], sim = strides[VPC_RM_IM], sparam = strides[VPC_RM_PARAM],
               simg = strides[VPC_RM_IMG], spre = strides[VPC_RM_PRE], sstat = strides[VPC_RM_STAT], sw1t = strides[VPC_RM_W1T],
               sR = strides[VPC_RM_R];
    // every member's slice inside its stride; x may be shared (stride 0); the image and workspace slices stay 16-byte aligned
    if ((sx != 0 && sx < nd) || sm < nd || sim < (long)M * nd || sparam < (long)H1 * d + H1 || sR < (long)n * (d - 1))
        return VPC_ERR_ARG;
    if (simg <= 0 || simg % 4 || spre < (long)n * Mp * 2 * H1P || spre % 4 || sstat < (long)n * Mp * STAT || sstat % 4 ||
        sw1t < (long)d * H1P + nd + 4 || sw1t % 4)
        return VPC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = sizeof(float) * W23_FLOATS;
    if (!lds_attr_done(reinterpret_cast<const void*>(reward_chain_multi_kernel<0>), lds)) return VPC_ERR_HIP;
    if (!lds_attr_done(reinterpret_cast<const void*>(reward_chain_multi_kernel<1>), lds)) return VPC_ERR_HIP;
    const long itemsB = (long)n * ((d - 1 + RW_CH - 1) / RW_CH);
    // members [g0, g0 + gc) go through the workspaces (held for `chunk` members) one chunk after the other on the stream
    for (int g0 = 0; g0 < G; g0 += chunk) {
        const int gc = G - g0 < chunk ? G - g0 : chunk;
        RewardMultiArgs m{x + g0 * sx, im + g0 * sim, W1 + g0 * sparam, b1 + g0 * sparam, enc_img + EncImg(dt_for(d)).oW2 + g0 * simg,
                          mask + g0 * sm, pre, stat, w1t, R + g0 * sR, sx, sm, sim, sparam, simg, spre, sstat, sw1t, sR,
                          n, d, L, M, (int)Mp};
        // per member the grid of vpc_reward_matrix, the chunk's total held to the same 3 workgroups per CU (the hand-out order of
        // the items is all that depends on it)
        const long cap = ((long)num_cus() * 3 + gc - 1) / gc;
        long gA = (n + RW_WAVES - 1) / RW_WAVES, gB = (itemsB + RW_WAVES - 1) / RW_WAVES;
        if (gA > cap) gA = cap;
        if (gB > cap) gB = cap;
        hipLaunchKernelGGL(reward_prep_multi_kernel, dim3(n + (d + 7) / 8, gc), dim3(128), 0, s, m);
        hipLaunchKernelGGL(reward_chain_multi_kernel<0>, dim3((unsigned)gA, gc), dim3(RW_THREADS), lds, s, m);
        hipLaunchKernelGGL(reward_chain_multi_kernel<1>, dim3((unsigned)gB, gc), dim3(RW_THREADS), lds, s, m);
        if (hipGetLastError() != hipSuccess) return VPC_ERR_HIP;
    }
    return VPC_OK;
}

// ---- ... for the mask-augmented and the point-net members
namespace {
// the shape limits of the family members' forward kernels (vpc_impute_small_multi_aug_f32 / _eddi_f32)
int reward_multi_ex_shape(int kind, int d, int K) {
    if (kind == RK_DENSE_MASK) return d >= 2 && 2 * d <= MAX_D ? VPC_OK : VPC_ERR_SHAPE;
    if (kind == RK_POINTNET) return d >= 2 && d <= 64 && K >= 1 && K <= PN_MAX_K ? VPC_OK : VPC_ERR_SHAPE;
    return VPC_ERR_ARG;  // (the plain kind has vpc_reward_matrix_multi)
}

template <int KIND>
int reward_multi_launch(const RewardMultiKindArgs& ma, int gc, hipStream_t s) {
    const RewardMultiArgs& m = ma.m;
    const size_t ldsA = sizeof(float) * W23_FLOATS;
    const size_t ldsB = ldsA + (KIND == RK_POINTNET ? sizeof(float) * ((ma.K + 15) / 16 * PN_FRAG) : 0);
    if (!lds_attr_done(reinterpret_cast<const void*>(reward_chain_multi_kind_kernel<KIND, 0>), ldsA)) return VPC_ERR_HIP;
    if (!lds_attr_done(reinterpret_cast<const void*>(reward_chain_multi_kind_kernel<KIND, 1>), ldsB)) return VPC_ERR_HIP;
    // per member the grids of reward_launch, the chunk's total held to 3 workgroups per CU as in vpc_reward_matrix_multi
    const long itemsB = (long)m.n * ((m.d - 1 + RW_CH - 1) / RW_CH);
    const long cap = ((long)num_cus() * 3 + gc - 1) / gc;
    long gA = (m.n + RW_WAVES - 1) / RW_WAVES, gB = (itemsB + RW_WAVES - 1) / RW_WAVES;
    if (gA > cap) gA = cap;
    if (gB > cap) gB = cap;
    const int tail_blocks = KIND == RK_POINTNET ? 1 : (m.d + 7) / 8;
    hipLaunchKernelGGL(reward_prep_multi_kind_kernel<KIND>, dim3(m.n + tail_blocks, gc), dim3(128), 0, s, ma);
    hipLaunchKernelGGL((reward_chain_multi_kind_kernel<KIND, 0>), dim3((unsigned)gA, gc), dim3(RW_THREADS), ldsA, s, ma);
    hipLaunchKernelGGL((reward_chain_multi_kind_kernel<KIND, 1>), dim3((unsigned)gB, gc), dim3(RW_THREADS), ldsB, s, ma);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}
}  // namespace

extern "C" int vpc_reward_scratch_multi_ex(int kind, int n, int d, int M, int K, long* pre_floats, long* stat_floats,
                                           long* w1t_floats) {
    if (n <= 0 || M <= 0) return VPC_ERR_ARG;
    int rc = reward_multi_ex_shape(kind, d, K);
    if (rc != VPC_OK) return rc;
    long w1t = 0;
    rc = vpc_reward_scratch_ex(kind, n, d, M, K, pre_floats, stat_floats, &w1t);
    if (rc != VPC_OK) return rc;
    if (w1t_floats) *w1t_floats = (w1t + 3) / 4 * 4;
    return VPC_OK;
}

extern "C" int vpc_reward_matrix_multi_ex(int kind, const float* x, const uint8_t* mask, const float* im, const float* W1,
                                          const float* b1, const float* AC, int K, const float* w23_img, float* pre, float* stat,
                                          float* w1t, float* R, int G, int chunk, const long* strides, int n, int d, int L, int M,
                                          void* stream) {
    if (!x || !mask || !im || !W1 || !b1 || !w23_img || !pre || !stat || !w1t || !R || !strides) return VPC_ERR_ARG;
    if (n <= 0 || M <= 0 || G < 1 || chunk < 1 || chunk > 65535) return VPC_ERR_ARG;
    const int rc = reward_multi_ex_shape(kind, d, K);
    if (rc != VPC_OK) return rc;
    if (L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (kind == RK_POINTNET && (!AC || (uintptr_t)AC % 4)) return VPC_ERR_ARG;
    if (!aligned16(pre) || !aligned16(stat) || !aligned16(w1t) || !aligned16(w23_img)) return VPC_ERR_ARG;
    const long Mp = (M + 15) / 16 * 16, nd = (long)n * d;
    const long sx = strides[VPC_RM_X], sm = strides[VPC_RM_MASK], sim = strides[VPC_RM_IM], sparam = strides[VPC_RM_PARAM],
               simg = strides[VPC_RM_IMG], spre = strides[VPC_RM_PRE], sstat = strides[VPC_RM_STAT], sw1t = strides[VPC_RM_W1T],
               sR = strides[VPC_RM_R], sAC = strides[VPC_RM_AC];
    const long din = kind == RK_DENSE_MASK ? 2L * d : K;  // columns of W1
    // every member's slice inside its stride; x may be shared (stride 0); the image and workspace slices stay 16-byte aligned
    if ((sx != 0 && sx < nd) || sm < nd || sim < (long)M * nd || sparam < (long)H1 * din + H1 || sR < (long)n * (d - 1))
        return VPC_ERR_ARG;
    if (simg < W23_FLOATS || simg % 4 || spre < (long)n * Mp * 2 * H1P || spre % 4 || sstat < (long)n * Mp * STAT || sstat % 4 ||
        sw1t < reward_table_floats(kind, d) + nd + 4 || sw1t % 4)
        return VPC_ERR_ARG;
    if (kind == RK_POINTNET && sAC < 2L * K * d) return VPC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    for (int g0 = 0; g0 < G; g0 += chunk) {
        const int gc = G - g0 < chunk ? G - g0 : chunk;
        const RewardMultiKindArgs ma{
            RewardMultiArgs{x + g0 * sx, im + g0 * sim, W1 + g0 * sparam, b1 + g0 * sparam, w23_img + g0 * simg, mask + g0 * sm, pre,
                            stat, w1t, R + g0 * sR, sx, sm, sim, sparam, simg, spre, sstat, sw1t, sR, n, d, L, M, (int)Mp},
            kind == RK_POINTNET ? AC + g0 * sAC : nullptr, sAC, kind == RK_POINTNET ? K : 0};
        const int lrc = kind == RK_DENSE_MASK ? reward_multi_launch<RK_DENSE_MASK>(ma, gc, s)
                                              : reward_multi_launch<RK_POINTNET>(ma, gc, s);
        if (lrc != VPC_OK) return lrc;
    }
    return VPC_OK;
}

extern "C" int vpc_acquire_multi(const float* R, long R_stride, uint8_t* mask, long mask_stride, int mask_pitch, uint8_t* mask2,
                                 long mask2_stride, int mask2_pitch, int* action, long action_stride, int action_pitch, int G,
                                 int n, int d, void* stream) {
    if (!R || !mask || !action || (uintptr_t)R % 4 || (uintptr_t)action % 4) return VPC_ERR_ARG;
    if (G < 1 || G > 65535 || n < 1) return VPC_ERR_ARG;
    if (d < 2 || d > MAX_D) return VPC_ERR_SHAPE;
    if (R_stride < (long)n * (d - 1) || mask_pitch < d || mask_stride < (long)n * mask_pitch || action_pitch < 1 ||
        action_stride < (long)(n - 1) * action_pitch + 1)
        return VPC_ERR_ARG;
    if (mask2 && (mask2_pitch < d || mask2_stride < (long)n * mask2_pitch)) return VPC_ERR_ARG;
    AcquireArgs a{R, mask, mask2, action, R_stride, mask_stride, mask2_stride, action_stride, n, d, mask_pitch, mask2_pitch,
                  action_pitch};
    hipLaunchKernelGGL(acquire_multi_kernel, dim3((n + RW_WAVES - 1) / RW_WAVES, G), dim3(RW_THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}
