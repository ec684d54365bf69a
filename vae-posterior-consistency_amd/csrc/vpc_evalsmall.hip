// Evaluate-stage forward of an ensemble, fp32 (gfx950): G members x (MC pass x batch x 16-row tile) in one launch, and the
// launch that turns the tile records into the four numbers eval_vae reports.
//
// Reference semantics: the loop body of eval_vae (src/experiment_main/evaluate.py:136-297) for Reg_VAE / vanilla_VAE: model.forward
// (src/models/VAE.py:496-507; :1153-1169) -> model.loss(llh_eval=True, stage='evaluate') (VAE.py:410-420: only the q pass reaches an
// output; mask_p, alpha and the p pass do not) -> the RMSE on ~mask (evaluate.py:229-234), then the mean over the batches of a pass
// and over the M passes (evaluate.py:238-245).
//
// eval_small_kernel: one workgroup of 8 waves per 16-row tile, the feature tiles of a layer split over the waves as in
// step_small_kernel (vpc_small.hip): stage order, MFMA shapes and the one-stage-ahead weight-fragment requests are those of phase
// "E" (pass 0) and of the decoder forward of the tile body (vpc_small_body.h), the helpers those of vpc_small_device.h.  Seven
// activation buffers (X, H1, H2, ML, Z, G1, G2) of 9 216 bytes: two workgroups per CU.  A tile lies inside ONE batch (the
// per-batch quantities are non-linear); the host's tile table says where its rows are.  Five sums per tile, one record of doubles
// per (member, tile), no atomics.
// eval_small_aug_kernel / eval_small_eddi_kernel: the same body for Reg_VAE_mask / vanilla_VAE_mask members (VAE.py:570-580,
// :1053-1060: input [x*mask | mask]) and for Reg_EDDI / vanilla_EDDI members (VAE.py:757-767, :935-950: the point-net front-end,
// folded per workgroup in the buffers that are idle until the first encoder stage); same LDS, same records, same reduce launch.
// eval_reduce_multi_kernel: blockIdx.y = member; tiles -> batches -> passes -> out[g][4] in fp64, in a fixed order.
// impute_small_kernel: the same forward (ONE body text, vpc_evalsmall_body.h) keeping x_hat instead of the sums - the M Monte-Carlo
// forwards of active_learning_func (evaluate.py:380-414) for G members: x_hat per draw row, or the target column's squared error
// (impute_small_aug_kernel / impute_small_eddi_kernel: the same for mask-augmented and point-net members);
// target_mse_multi_kernel: the mean of those errors per member (evaluate.py:390-392), fp64 in a fixed order.
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_small_device.h"
#include "vpc_rng.h"

namespace vpc {

enum { E_X = 0, E_H1, E_H2, E_ML, E_Z, E_G1, E_G2, E_COUNT };
constexpr int EVAL_TERMS = VPC_EVAL_TERMS;  // S_A, S_I, SQ, CNT, KL
constexpr int EVAL_LDS = (E_COUNT * SBUF + WAVES * EVAL_TERMS) * 4;
static_assert(2 * EVAL_LDS <= 163840, "two workgroups per CU");

struct EvalArgs {
    const float* x;              // member 0's [N][d] data
    const uint8_t* mask;         // member 0's [N][d] mask bytes
    const float* eps;            // member 0's [R][16] injected normals (draw == 0)
    const float* enc_img;
    const float* dec_img;
    const VpcMember* members;
    const long long* tiles;      // [n_tiles][4]: data row, valid rows, draw row, batch
    double* part;                // member 0's [n_tiles][EVAL_TERMS] records
    long sx, sm, seps, simg, spart;  // member strides in elements (sx / sm / seps 0: shared by all members)
    long N, R;                   // data rows, draw rows
    unsigned long long offset;   // Philox offset of the call (draw != 0)
    long tile0;                  // first tile of this launch
    float x_logvar;
    int d, d_real, L, draw;
};

// What becomes of x_hat: OUT_SUMS the five sums of the tile's record, OUT_XHAT / OUT_SQERR what impute_small_kernel writes.
enum { OUT_SUMS = 0, OUT_XHAT, OUT_SQERR };
// The point-net kernel's own arguments (an empty record elsewhere): the front-end is read from the members' rows of the parameter
// stack [trunk | decoder | front-end], no copy.
struct EvalPointNet {
    int K;               // emb_dim
    const float* front;  // member 0's front-end parameters (E [d_real][K] | t [d_real] | W [K][2+K] | c [K])
    long sP;             // member stride of `front` in floats
};
struct EvalPnArgs : EvalArgs { EvalPointNet pn; };

template <int DT>
__global__ __launch_bounds__(THREADS) void eval_small_kernel(EvalArgs a) {
    constexpr int DTI = DT;
    constexpr bool AUG = false;
    constexpr bool PN = false;
    constexpr EvalPointNet pnx{};
    constexpr int OUT = OUT_SUMS;
    float* const out = nullptr;
    const long sout = 0;
#include "vpc_evalsmall_body.h"
}
// Reg_VAE_mask / vanilla_VAE_mask members (src/models/VAE.py:570-580, 1053-1060): encoder input [x*mask | mask] of DTI =
// dt_for(2 d_real) tiles built in the input stage, decoder output of DT = dt_for(d_real) tiles; a.d is the row pitch.
template <int DTI, int DT>
__global__ __launch_bounds__(THREADS) void eval_small_aug_kernel(EvalArgs a) {
    constexpr bool AUG = true;
    constexpr bool PN = false;
    constexpr EvalPointNet pnx{};
    constexpr int OUT = OUT_SUMS;
    float* const out = nullptr;
    const long sout = 0;
#include "vpc_evalsmall_body.h"
}
// Reg_EDDI / vanilla_EDDI members (VAE.py:757-767, 935-950): the point-net front-end as the input stage, the trunk as the body's
// encoder with DTI = dt_for(K) input tiles, decoder output of DT = dt_for(d_real) tiles.
template <int DTI, int DT>
__global__ __launch_bounds__(THREADS) void eval_small_eddi_kernel(EvalPnArgs pa) {
    constexpr bool AUG = false;
    constexpr bool PN = true;
    const EvalArgs& a = pa;
    const EvalPointNet& pnx = pa.pn;
    constexpr int OUT = OUT_SUMS;
    float* const out = nullptr;
    const long sout = 0;
#include "vpc_evalsmall_body.h"
}

// The same forward, x_hat kept: MODE 0 writes x_hat[g][draw row][0..d_real), MODE 1 (x_hat[T] - x[T])^2 of the target column
// T = d_real - 1 per draw row (the M passes of active_learning_func's imputation and of its target MSE, evaluate.py:390-414).
constexpr int IMPUTE_LDS = E_COUNT * SBUF * 4;
static_assert(2 * IMPUTE_LDS <= 163840, "two workgroups per CU");
struct ImputeArgs {
    EvalArgs e;   // (part unused)
    float* out;   // member 0's [R][d_real] (MODE 0) or [R] (MODE 1)
    long sout;    // member stride in floats
};
template <int DT, int MODE>
__global__ __launch_bounds__(THREADS) void impute_small_kernel(ImputeArgs ia) {
    constexpr int DTI = DT;  // (plain members only)
    constexpr bool AUG = false;
    constexpr bool PN = false;
    constexpr EvalPointNet pnx{};
    constexpr int OUT = MODE == 0 ? OUT_XHAT : OUT_SQERR;
    const EvalArgs& a = ia.e;
    float* const out = ia.out;
    const long sout = ia.sout;
#include "vpc_evalsmall_body.h"
}
// ... for Reg_VAE_mask / vanilla_VAE_mask members: the input stage of eval_small_aug_kernel, the outputs of impute_small_kernel
// (the body's AUG / PN stages and its OUT stage share no code: the input stage ends at E_X, the output stage starts at `pre`).
template <int DTI, int DT, int MODE>
__global__ __launch_bounds__(THREADS) void impute_small_aug_kernel(ImputeArgs ia) {
    constexpr bool AUG = true;
    constexpr bool PN = false;
    constexpr EvalPointNet pnx{};
    constexpr int OUT = MODE == 0 ? OUT_XHAT : OUT_SQERR;
    const EvalArgs& a = ia.e;
    float* const out = ia.out;
    const long sout = ia.sout;
#include "vpc_evalsmall_body.h"
}
// ... and for Reg_EDDI / vanilla_EDDI members: the input stage of eval_small_eddi_kernel.
struct ImputePnArgs : ImputeArgs { EvalPointNet pn; };
template <int DTI, int DT, int MODE>
__global__ __launch_bounds__(THREADS) void impute_small_eddi_kernel(ImputePnArgs pa) {
    constexpr bool AUG = false;
    constexpr bool PN = true;
    const EvalPointNet& pnx = pa.pn;
    constexpr int OUT = MODE == 0 ? OUT_XHAT : OUT_SQERR;
    const EvalArgs& a = pa.e;
    float* const out = pa.out;
    const long sout = pa.sout;
#include "vpc_evalsmall_body.h"
}

// ---- tiles -> batches -> passes -> out[g][4]
constexpr int RED_WAVES = 8;
struct EvalReduceArgs {
    const double* part;          // member 0's [n_tiles][EVAL_TERMS]
    const long long* batches;    // [n_batches][4]: rows, pass, first tile, tiles
    const long long* passes;     // [M][2]: first batch, batches
    const VpcMember* members;
    float* out;                  // [G][4]: rmse, elbo, negll, negll_imp
    long spart, n_tiles, n_batches;
    int M, d_real;
};

__device__ __forceinline__ double wave_sum_f64(double v) {  // (fixed order: a butterfly)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(RED_WAVES * 64) void eval_reduce_multi_kernel(EvalReduceArgs a) {
    __shared__ double tot[RED_WAVES][4];
    const unsigned mem = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double* part = a.part + mem * a.spart;
    const double bw = (double)a.members[mem].co.bq;  // the member's KL weight
    constexpr double HL2PI = 0.91893853320467274;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};  // this wave's passes p = w, w + RED_WAVES, ...: sum of the pass means
    for (int p = w; p < a.M; p += RED_WAVES) {
        long b0 = a.passes[2 * p], nb = a.passes[2 * p + 1];
        if (b0 < 0 || nb < 0 || b0 + nb > a.n_batches) nb = 0;  // (fence, as in the forward kernel; an empty pass gives 0 / 0)
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (long b = b0 + lane; b < b0 + nb; b += 64) {
            const long long* be = a.batches + 4 * b;
            const double n_b = (double)be[0];
            long t0 = be[2], nt = be[3];
            if (t0 < 0 || nt < 0 || t0 + nt > a.n_tiles) nt = 0;
            double s[EVAL_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (long t = t0; t < t0 + nt; ++t)
#pragma unroll
                for (int i = 0; i < EVAL_TERMS; ++i) s[i] += part[t * EVAL_TERMS + i];
            const double c = n_b * (double)a.d_real * HL2PI;  // masked entries contribute the constant too
            const double negll = (s[0] + c) / n_b, negll_imp = (s[1] + c) / n_b;
            v[0] += sqrt(s[2] / s[3]);  // no unobserved entry: 0 / 0 = NaN, as evaluate.py:232-234
            v[1] += negll + bw * s[4] / n_b;
            v[2] += negll;
            v[3] += negll_imp;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += wave_sum_f64(v[i]) / (double)nb;  // mean over the batches of the pass
    }
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) tot[w][i] = acc[i];
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = 0.0;
        for (int k = 0; k < RED_WAVES; ++k) t += tot[k][threadIdx.x];
        a.out[mem * 4 + threadIdx.x] = (float)(t / (double)a.M);  // mean over the passes
    }
}

// ---- out[g * out_stride] = mean of sq[g][0..R), blockIdx.y = member: fp64 in a fixed order (thread t sums rows t, t + 512, ..; a
// butterfly per wave; the waves in order)
__global__ __launch_bounds__(RED_WAVES * 64) void target_mse_multi_kernel(const float* __restrict__ sq, long ssq, long R,
                                                                          float* __restrict__ out, long out_stride) {
    __shared__ double tot[RED_WAVES];
    const unsigned mem = blockIdx.y;
    const float* s = sq + mem * ssq;
    double v = 0.0;
    for (long r = threadIdx.x; r < R; r += RED_WAVES * 64) v += (double)s[r];
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) tot[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < RED_WAVES; ++k) t += tot[k];
        out[mem * out_stride] = (float)(t / (double)R);
    }
}

}  // namespace vpc

using namespace vpc;

namespace {
// the checks and the argument record the two forward entries share (everything but where the result goes)
int eval_forward_args(const float* x, const uint8_t* mask, const float* eps, const float* enc_img, const float* dec_img,
                      const VpcMember* members, int G, const long long* tiles, long n_tiles, long N, long R, int draw,
                      unsigned long long offset, float x_logvar, const long* strides, int d, int d_real, int L, int max_blocks,
                      EvalArgs& a) {
    if (!x || !mask || !enc_img || !dec_img || !members || !tiles || !strides) return VPC_ERR_ARG;
    if (G < 1 || G > 65535 || n_tiles < 1 || N < 1 || R < 1 || max_blocks < 0) return VPC_ERR_ARG;
    if (!draw && !eps) return VPC_ERR_ARG;
    if (d < 4 || d > MAX_D || d % 4 || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (d_real < 1 || d_real > d || dt_for(d_real) != dt_for(d)) return VPC_ERR_ARG;
    if (!aligned16(x) || !aligned16(enc_img) || !aligned16(dec_img) || !aligned16(eps)) return VPC_ERR_ARG;
    if ((uintptr_t)mask % 4 || (uintptr_t)tiles % 8) return VPC_ERR_ARG;
    const long sx = strides[VPC_MS_X], sm = strides[VPC_MS_MASK], seps = strides[VPC_MS_EPS], simg = strides[VPC_MS_IMG];
    // every member's slice inside its stride, 16-byte (masks: 4-byte) aligned; the read-only inputs may be shared (stride 0)
    if ((sx != 0 && sx < N * (long)d) || sx % 4 || (sm != 0 && sm < N * (long)d) || sm % 4) return VPC_ERR_ARG;
    if (!draw && ((seps != 0 && seps < R * 16) || seps % 4)) return VPC_ERR_ARG;
    if (simg <= 0 || simg % 4) return VPC_ERR_ARG;
    a = EvalArgs{};
    a.x = x; a.mask = mask; a.eps = draw ? nullptr : eps; a.enc_img = enc_img; a.dec_img = dec_img; a.members = members;
    a.tiles = tiles;
    a.sx = sx; a.sm = sm; a.seps = draw ? 0 : seps; a.simg = simg;
    a.N = N; a.R = R; a.offset = offset; a.x_logvar = x_logvar; a.d = d; a.d_real = d_real; a.L = L; a.draw = draw ? 1 : 0;
    return VPC_OK;
}

// The grid is (tiles of the chunk, G): consecutive workgroups are tiles of one member, so the workgroups in flight read one or two
// members' images.  A launch holds at most max_blocks workgroups (0: VPC_EVAL_MAX_BLOCKS); the tile table is walked in chunks:
// launch(first tile, grid) starts one of them.
template <class Launch>
int eval_chunks(long n_tiles, int G, int max_blocks, Launch launch) {
    const long cap = max_blocks ? max_blocks : VPC_EVAL_MAX_BLOCKS;
    const long per = cap / G > 0 ? cap / G : 1;
    for (long t0 = 0; t0 < n_tiles; t0 += per) {
        const long nt = n_tiles - t0 < per ? n_tiles - t0 : per;
        if (!launch(t0, dim3((unsigned)nt, (unsigned)G))) return VPC_ERR_HIP;
        if (hipGetLastError() != hipSuccess) return VPC_ERR_HIP;
    }
    return VPC_OK;
}
}  // namespace

extern "C" int vpc_eval_small_multi_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img,
                                        const float* dec_img, const VpcMember* members, int G, const long long* tiles,
                                        long n_tiles, long N, long R, int draw, unsigned long long offset, float x_logvar,
                                        double* part, const long* strides, int d, int d_real, int L, int max_blocks,
                                        void* stream) {
    if (!part || (uintptr_t)part % 8) return VPC_ERR_ARG;
    EvalArgs a;
    const int rc = eval_forward_args(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar,
                                     strides, d, d_real, L, max_blocks, a);
    if (rc != VPC_OK) return rc;
    if (strides[VPC_MS_LOSS] < n_tiles * EVAL_TERMS) return VPC_ERR_ARG;
    a.part = part;
    a.spart = strides[VPC_MS_LOSS];
    hipStream_t s = (hipStream_t)stream;
    return eval_chunks(n_tiles, G, max_blocks, [&](long t0, dim3 grid) {
        a.tile0 = t0;
#define VPC_CASE(T)                                                                                        \
    case T: {                                                                                              \
        auto kern = eval_small_kernel<T>;                                                                  \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), EVAL_LDS)) return false;                   \
        hipLaunchKernelGGL(kern, grid, dim3(THREADS), EVAL_LDS, s, a);                                     \
        return true;                                                                                       \
    }
        switch (dt_for(d)) { VPC_CASE(1) VPC_CASE(2) VPC_CASE(4) VPC_CASE(8) }
#undef VPC_CASE
        return false;
    });
}

// The evaluate-stage forward of G Reg_VAE_mask / vanilla_VAE_mask members: d is the row pitch 4 ceil(d_real / 4) of x and the mask,
// the images are those of the mask-augmented layout.
extern "C" int vpc_eval_small_multi_aug_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img,
                                            const float* dec_img, const VpcMember* members, int G, const long long* tiles,
                                            long n_tiles, long N, long R, int draw, unsigned long long offset, float x_logvar,
                                            double* part, const long* strides, int d, int d_real, int L, int max_blocks,
                                            void* stream) {
    // (the shape limits of vpc_step_small_multi_aug_f32)
    if (d_real < 1 || d_real > d || d - d_real > 3 || 2 * d_real > MAX_D) return VPC_ERR_SHAPE;
    if (!part || (uintptr_t)part % 8) return VPC_ERR_ARG;
    EvalArgs a;
    const int rc = eval_forward_args(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar,
                                     strides, d, d_real, L, max_blocks, a);
    if (rc != VPC_OK) return rc;
    if (strides[VPC_MS_LOSS] < n_tiles * EVAL_TERMS) return VPC_ERR_ARG;
    a.part = part;
    a.spart = strides[VPC_MS_LOSS];
    hipStream_t s = (hipStream_t)stream;
    return eval_chunks(n_tiles, G, max_blocks, [&](long t0, dim3 grid) {
        a.tile0 = t0;
#define VPC_CASE(TI, T)                                                                                    \
    case TI: {                                                                                             \
        auto kern = eval_small_aug_kernel<TI, T>;                                                          \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), EVAL_LDS)) return false;                   \
        hipLaunchKernelGGL(kern, grid, dim3(THREADS), EVAL_LDS, s, a);                                     \
        return true;                                                                                       \
    }
        // (input tiles, output tiles) = (dt_for(2 d_real), dt_for(d_real)): d_real <= 8, 16, 32, 64
        switch (dt_for(2 * d_real)) { VPC_CASE(1, 1) VPC_CASE(2, 1) VPC_CASE(4, 2) VPC_CASE(8, 4) }
#undef VPC_CASE
        return false;
    });
}

// ... and of G Reg_EDDI / vanilla_EDDI members: images of the point-net layout; `front` is member 0's front-end parameters, member
// g's lie strides[VPC_MS_PARAM] floats further (inside the member's row of the parameter stack, behind trunk and decoder).
extern "C" int vpc_eval_small_multi_eddi_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img,
                                             const float* dec_img, const VpcMember* members, int G, const long long* tiles,
                                             long n_tiles, long N, long R, int draw, unsigned long long offset, float x_logvar,
                                             double* part, const long* strides, int d, int d_real, int L, int K,
                                             const float* front, int max_blocks, void* stream) {
    // (the shape limits of vpc_step_small_multi_eddi_f32, and its pointer checks)
    if (d_real < 1 || d_real > 64 || d_real > d || d - d_real > 3 || d > 64 || K < 1 || K > 32) return VPC_ERR_SHAPE;
    if (!front || (uintptr_t)front % 4) return VPC_ERR_ARG;
    if (!part || (uintptr_t)part % 8) return VPC_ERR_ARG;
    EvalPnArgs a;
    const int rc = eval_forward_args(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar,
                                     strides, d, d_real, L, max_blocks, a);
    if (rc != VPC_OK) return rc;
    if (strides[VPC_MS_LOSS] < n_tiles * EVAL_TERMS) return VPC_ERR_ARG;
    const long nfront = (long)d_real * K + d_real + (long)K * (2 + K) + K;
    if (strides[VPC_MS_PARAM] < nfront) return VPC_ERR_ARG;  // (read only, but every member has its own row)
    a.part = part;
    a.spart = strides[VPC_MS_LOSS];
    a.pn = EvalPointNet{K, front, strides[VPC_MS_PARAM]};
    hipStream_t s = (hipStream_t)stream;
    return eval_chunks(n_tiles, G, max_blocks, [&](long t0, dim3 grid) {
        a.tile0 = t0;
#define VPC_CASE(TI, T)                                                                                    \
    case 4 * TI + T: {                                                                                     \
        auto kern = eval_small_eddi_kernel<TI, T>;                                                         \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), EVAL_LDS)) return false;                   \
        hipLaunchKernelGGL(kern, grid, dim3(THREADS), EVAL_LDS, s, a);                                     \
        return true;                                                                                       \
    }
        // (input tiles, output tiles) = (dt_for(K), dt_for(d_real)): K <= 16, 32; d_real <= 16, 32, 64
        switch (4 * dt_for(K) + dt_for(d_real)) {
            VPC_CASE(1, 1) VPC_CASE(1, 2) VPC_CASE(1, 4) VPC_CASE(2, 1) VPC_CASE(2, 2) VPC_CASE(2, 4)
        }
#undef VPC_CASE
        return false;
    });
}

extern "C" int vpc_impute_small_multi_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img,
                                          const float* dec_img, const VpcMember* members, int G, const long long* tiles,
                                          long n_tiles, long N, long R, int draw, unsigned long long offset, float x_logvar,
                                          int mode, float* out, long out_stride, const long* strides, int d, int d_real, int L,
                                          int max_blocks, void* stream) {
    if (!out || (uintptr_t)out % 4 || mode < 0 || mode > 1) return VPC_ERR_ARG;
    ImputeArgs ia;
    const int rc = eval_forward_args(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar,
                                     strides, d, d_real, L, max_blocks, ia.e);
    if (rc != VPC_OK) return rc;
    if (out_stride < (mode == 0 ? R * (long)d_real : R)) return VPC_ERR_ARG;  // a draw row < R is the only row written
    ia.out = out;
    ia.sout = out_stride;
    hipStream_t s = (hipStream_t)stream;
    return eval_chunks(n_tiles, G, max_blocks, [&](long t0, dim3 grid) {
        ia.e.tile0 = t0;
#define VPC_CASE(T, MODE)                                                                                  \
    case 2 * T + MODE: {                                                                                   \
        auto kern = impute_small_kernel<T, MODE>;                                                          \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), IMPUTE_LDS)) return false;                 \
        hipLaunchKernelGGL(kern, grid, dim3(THREADS), IMPUTE_LDS, s, ia);                                  \
        return true;                                                                                       \
    }
        switch (2 * dt_for(d) + mode) {
            VPC_CASE(1, 0) VPC_CASE(2, 0) VPC_CASE(4, 0) VPC_CASE(8, 0) VPC_CASE(1, 1) VPC_CASE(2, 1) VPC_CASE(4, 1) VPC_CASE(8, 1)
        }
#undef VPC_CASE
        return false;
    });
}

// vpc_impute_small_multi_f32 for G Reg_VAE_mask / vanilla_VAE_mask members: shape limits and pointer checks of
// vpc_eval_small_multi_aug_f32, the out / out_stride checks of the plain impute entry.
extern "C" int vpc_impute_small_multi_aug_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img,
                                              const float* dec_img, const VpcMember* members, int G, const long long* tiles,
                                              long n_tiles, long N, long R, int draw, unsigned long long offset, float x_logvar,
                                              int mode, float* out, long out_stride, const long* strides, int d, int d_real,
                                              int L, int max_blocks, void* stream) {
    if (d_real < 1 || d_real > d || d - d_real > 3 || 2 * d_real > MAX_D) return VPC_ERR_SHAPE;
    if (!out || (uintptr_t)out % 4 || mode < 0 || mode > 1) return VPC_ERR_ARG;
    ImputeArgs ia;
    const int rc = eval_forward_args(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar,
                                     strides, d, d_real, L, max_blocks, ia.e);
    if (rc != VPC_OK) return rc;
    if (out_stride < (mode == 0 ? R * (long)d_real : R)) return VPC_ERR_ARG;
    ia.out = out;
    ia.sout = out_stride;
    hipStream_t s = (hipStream_t)stream;
    return eval_chunks(n_tiles, G, max_blocks, [&](long t0, dim3 grid) {
        ia.e.tile0 = t0;
#define VPC_CASE(TI, T, MODE)                                                                              \
    case 2 * TI + MODE: {                                                                                  \
        auto kern = impute_small_aug_kernel<TI, T, MODE>;                                                  \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), IMPUTE_LDS)) return false;                 \
        hipLaunchKernelGGL(kern, grid, dim3(THREADS), IMPUTE_LDS, s, ia);                                  \
        return true;                                                                                       \
    }
        // (input tiles, output tiles) as vpc_eval_small_multi_aug_f32
        switch (2 * dt_for(2 * d_real) + mode) {
            VPC_CASE(1, 1, 0) VPC_CASE(2, 1, 0) VPC_CASE(4, 2, 0) VPC_CASE(8, 4, 0)
            VPC_CASE(1, 1, 1) VPC_CASE(2, 1, 1) VPC_CASE(4, 2, 1) VPC_CASE(8, 4, 1)
        }
#undef VPC_CASE
        return false;
    });
}

// ... and for G Reg_EDDI / vanilla_EDDI members: limits and checks of vpc_eval_small_multi_eddi_f32.
extern "C" int vpc_impute_small_multi_eddi_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img,
                                               const float* dec_img, const VpcMember* members, int G, const long long* tiles,
                                               long n_tiles, long N, long R, int draw, unsigned long long offset, float x_logvar,
                                               int mode, float* out, long out_stride, const long* strides, int d, int d_real,
                                               int L, int K, const float* front, int max_blocks, void* stream) {
    if (d_real < 1 || d_real > 64 || d_real > d || d - d_real > 3 || d > 64 || K < 1 || K > 32) return VPC_ERR_SHAPE;
    if (!front || (uintptr_t)front % 4) return VPC_ERR_ARG;
    if (!out || (uintptr_t)out % 4 || mode < 0 || mode > 1) return VPC_ERR_ARG;
    ImputePnArgs ia;
    const int rc = eval_forward_args(x, mask, eps, enc_img, dec_img, members, G, tiles, n_tiles, N, R, draw, offset, x_logvar,
                                     strides, d, d_real, L, max_blocks, ia.e);
    if (rc != VPC_OK) return rc;
    if (out_stride < (mode == 0 ? R * (long)d_real : R)) return VPC_ERR_ARG;
    const long nfront = (long)d_real * K + d_real + (long)K * (2 + K) + K;
    if (strides[VPC_MS_PARAM] < nfront) return VPC_ERR_ARG;  // (read only, but every member has its own row)
    ia.out = out;
    ia.sout = out_stride;
    ia.pn = EvalPointNet{K, front, strides[VPC_MS_PARAM]};
    hipStream_t s = (hipStream_t)stream;
    return eval_chunks(n_tiles, G, max_blocks, [&](long t0, dim3 grid) {
        ia.e.tile0 = t0;
#define VPC_CASE(TI, T, MODE)                                                                              \
    case 8 * TI + 2 * T + MODE: {                                                                          \
        auto kern = impute_small_eddi_kernel<TI, T, MODE>;                                                 \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), IMPUTE_LDS)) return false;                 \
        hipLaunchKernelGGL(kern, grid, dim3(THREADS), IMPUTE_LDS, s, ia);                                  \
        return true;                                                                                       \
    }
        // (input tiles, output tiles) as vpc_eval_small_multi_eddi_f32
        switch (8 * dt_for(K) + 2 * dt_for(d_real) + mode) {
            VPC_CASE(1, 1, 0) VPC_CASE(1, 2, 0) VPC_CASE(1, 4, 0) VPC_CASE(2, 1, 0) VPC_CASE(2, 2, 0) VPC_CASE(2, 4, 0)
            VPC_CASE(1, 1, 1) VPC_CASE(1, 2, 1) VPC_CASE(1, 4, 1) VPC_CASE(2, 1, 1) VPC_CASE(2, 2, 1) VPC_CASE(2, 4, 1)
        }
#undef VPC_CASE
        return false;
    });
}

extern "C" int vpc_target_mse_multi(const float* sq, long sq_stride, long R, int G, float* out, long out_stride, void* stream) {
    if (!sq || !out || (uintptr_t)sq % 4 || (uintptr_t)out % 4) return VPC_ERR_ARG;
    if (G < 1 || G > 65535 || R < 1 || sq_stride < R || out_stride < 1) return VPC_ERR_ARG;
    hipLaunchKernelGGL(target_mse_multi_kernel, dim3(1, (unsigned)G), dim3(RED_WAVES * 64), 0, (hipStream_t)stream, sq, sq_stride,
                       R, out, out_stride);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

extern "C" int vpc_eval_reduce_multi(const double* part, const long long* batches, long n_batches, const long long* passes,
                                     int M, const VpcMember* members, int G, long part_stride, long n_tiles, int d_real,
                                     float* out, void* stream) {
    if (!part || !batches || !passes || !members || !out) return VPC_ERR_ARG;
    if (G < 1 || G > 65535 || M < 1 || n_batches < 1 || n_tiles < 1 || d_real < 1 || d_real > MAX_D) return VPC_ERR_ARG;
    if (part_stride < n_tiles * EVAL_TERMS) return VPC_ERR_ARG;
    if ((uintptr_t)part % 8 || (uintptr_t)batches % 8 || (uintptr_t)passes % 8 || (uintptr_t)out % 4) return VPC_ERR_ARG;
    EvalReduceArgs a{part, batches, passes, members, out, part_stride, n_tiles, n_batches, M, d_real};
    hipLaunchKernelGGL(eval_reduce_multi_kernel, dim3(1, (unsigned)G), dim3(RED_WAVES * 64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}
