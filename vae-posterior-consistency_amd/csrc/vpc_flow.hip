// Elementwise / reduction kernels of the flow path (reference src/models/VAE.py: VAEFlow :1860-1996, REG_VAEFlow
// :1999-2124, Flow :1816-1854, PiecewiseLinearCDF :1781-1813, unconstrained_linear_spline / linear_spline
// :1680-1774).  The layers are the generic fp32 GEMMs of vpc_gemm.hip; what is specific to the family runs here:
//
//   flow_prep   per step: mask_p draw (REG), the stacked encoder input [x*m | m] of the q and p passes, eps ~ N(0,1)
//   flow_fwd    eps -> three piecewise-linear CDF layers conditioned on t = seq_encoder(..) -> (z, z_log_prob)
//   flow_bwd    d / d t of the same, the forward recomputed from (t, eps)
//   flow_loss   Gaussian NLL + flow KL (+ the REG terms), forward and backward, in two launches: one wave per data row
//               (terms, gradients, per-workgroup partials), then one workgroup sums the partials in a fixed order
//
// Lane mapping of flow_fwd / flow_bwd: one thread per (row, latent i).  The thread owns the ten logits of its latent
// (t[row][10 i .. 10 i + 9]), the row's ten mask bits and the softmax / cumulative sum in registers; every per-bin
// lookup is an unrolled select, never a dynamically indexed register array, so nothing spills.  The three layers
// share one pdf: all three read the context t * [|eps| <= 1] (the reference's in-place multiply, :1695-1696, masks
// bin j with latent j's mask, and layers 2 and 3 see only clamped, inside inputs).
//
// The batch-global predicate torch.any(inside) (:1698) is taken per pass (rows [p B, (p + 1) B)) by every workgroup
// itself: it scans the pass's eps in blockDim-sized chunks (wave vote + one barrier) and stops at the first chunk that
// holds an inside element - one chunk for any non-degenerate draw.  No extra launch, no atomics, no host sync.
// No float atomics anywhere; every reduction has a fixed order, so the results are bit-reproducible.
#include "vpc_abi_internal.h"
#include "vpc_flow_loss_args.h"
#include "vpc_rng.h"

namespace vpc {

// the per-pass flags (f0: pass 0, f1: pass 1) of the rows [row0, row1] this workgroup covers (R = P * B, P <= 2)
__device__ __forceinline__ void flow_flags(const float* __restrict__ eps, long R, long B, long row0, long row1,
                                           bool& f0, bool& f1) {
    __shared__ int sh[4];
    const long last = row1 < R ? row1 : R - 1;
    f0 = row0 < B ? flow_pass_inside(eps, B, sh) : false;
    f1 = last >= B ? flow_pass_inside(eps + B * FLOW_L, B, sh) : false;
}

__global__ void __launch_bounds__(256) flow_fwd_kernel(const float* __restrict__ t, long ldt,
                                                       const float* __restrict__ eps, float* __restrict__ z,
                                                       float* __restrict__ zlp, long R, long B) {
#include "vpc_flow_fwd_body.h"
}

__global__ void __launch_bounds__(256) flow_bwd_kernel(const float* __restrict__ t, long ldt,
                                                       const float* __restrict__ eps, const float* __restrict__ dz,
                                                       const float* __restrict__ dz2, const float* __restrict__ dzlp,
                                                       float* __restrict__ dt, long lddt, long R, long B) {
#include "vpc_flow_bwd_body.h"
}

__global__ void __launch_bounds__(256) flow_prep_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                        const float* __restrict__ mp_in, float* __restrict__ mp_out,
                                                        float* __restrict__ xin, long B, int d, float keep_prob,
                                                        float* __restrict__ eps, long n_eps, uint64_t seed,
                                                        uint64_t offset, uint64_t offset_eps, unsigned gm) {
#include "vpc_flow_prep_body.h"
}

// ---- launch 1: one wave per data row b (both passes)
// partial columns: 0 RE_q, 1 RE_p, 2 KL_q, 3 KL_p, 4 KL_reg, 5 NLL of x*mask*~mask_p, 6 RE_q on ~mask
__global__ void __launch_bounds__(256) flow_loss_rows_kernel(FlowLossArgs a) {
#include "vpc_flow_loss_rows_body.h"
}

// ---- launch 2: one workgroup; column c of the partials summed by 32 lanes in a strided fixed order, then in lane order
__global__ void __launch_bounds__(256) flow_loss_reduce_kernel(FlowLossArgs a) {
#include "vpc_flow_loss_reduce_body.h"
}

// ================================================================================================ the ensemble forms
// G members in one launch (include/vpc.h, vpc_flow_*_multi): blockIdx.y = member, blockIdx.x = the workgroup's index among the
// member's workgroups.  A workgroup runs the stand-alone body on member g's arrays (base + g * stride), so a member's result
// does not depend on G.  torch.any(inside) (:1698) becomes a predicate per (member, pass): flow_pass_inside sees member g's
// eps rows of that pass only.
__global__ void __launch_bounds__(256) flow_fwd_multi_kernel(const float* __restrict__ t0, long ldt, long s_t,
                                                             const float* __restrict__ eps0, float* __restrict__ z0,
                                                             float* __restrict__ zlp0, long s10, long R, long B) {
    const long mem = blockIdx.y;
    const float* __restrict__ t = t0 + mem * s_t;
    const float* __restrict__ eps = eps0 + mem * s10;
    float* __restrict__ z = z0 + mem * s10;
    float* __restrict__ zlp = zlp0 + mem * s10;
#include "vpc_flow_fwd_body.h"
}

__global__ void __launch_bounds__(256) flow_bwd_multi_kernel(const float* __restrict__ t0, long ldt, long s_t,
                                                             const float* __restrict__ eps0, const float* __restrict__ dz0,
                                                             const float* __restrict__ dz20, const float* __restrict__ dzlp0,
                                                             long s10, float* __restrict__ dt0, long lddt, long sdt, long R,
                                                             long B) {
    const long mem = blockIdx.y;
    const float* __restrict__ t = t0 + mem * s_t;
    const float* __restrict__ eps = eps0 + mem * s10;
    const float* __restrict__ dz = dz0 ? dz0 + mem * s10 : nullptr;
    const float* __restrict__ dz2 = dz20 ? dz20 + mem * s10 : nullptr;
    const float* __restrict__ dzlp = dzlp0 ? dzlp0 + mem * s10 : nullptr;
    float* __restrict__ dt = dt0 + mem * sdt;
#include "vpc_flow_bwd_body.h"
}

// member g draws mask_p and eps with seed_g and keep_prob_g at the counters of the stand-alone prep
__global__ void __launch_bounds__(256) flow_prep_multi_kernel(const float* __restrict__ x0, long sx, const float* __restrict__ m0,
                                                              long sm, float* __restrict__ mp0, long smp, int draw,
                                                              float* __restrict__ xin0, long sxin, long B, int d,
                                                              float* __restrict__ eps0, long n_eps, long seps,
                                                              const VpcFlowMember* __restrict__ members, uint64_t offset,
                                                              uint64_t offset_eps, unsigned gm) {
    const long mem = blockIdx.y;
    const VpcFlowMember* rec = members + mem;  // (uniform address: scalar loads)
    const float* __restrict__ x = x0 + mem * sx;
    const float* __restrict__ m = m0 + mem * sm;
    float* mp = mp0 ? mp0 + mem * smp : nullptr;
    const float* __restrict__ mp_in = draw ? nullptr : mp;
    float* __restrict__ mp_out = draw ? mp : nullptr;
    float* __restrict__ xin = xin0 + mem * sxin;
    float* __restrict__ eps = eps0 ? eps0 + mem * seps : nullptr;
    const float keep_prob = rec->keep_prob;
    const uint64_t seed = rec->seed;
#include "vpc_flow_prep_body.h"
}

struct FlowLossMultiArgs {
    FlowLossArgs base;                 // member 0's arrays; alpha / beta come from the member table
    long sx, sm, smp, sxm, s10, sg;    // floats between two members' x / mask / mask_p / x_mean / [B][10] arrays / g_x_mean
    const VpcFlowMember* members;
};
__device__ __forceinline__ FlowLossArgs flow_loss_member(const FlowLossMultiArgs& ma, const long mem) {
    FlowLossArgs a = ma.base;
    const VpcFlowMember* r = ma.members + mem;
    a.x += mem * ma.sx; a.m += mem * ma.sm;
    if (a.mp) a.mp += mem * ma.smp;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (a.xm[p]) a.xm[p] += mem * ma.sxm;
        if (a.z[p]) a.z[p] += mem * ma.s10;
        if (a.zlp[p]) a.zlp[p] += mem * ma.s10;
        if (a.gxm[p]) a.gxm[p] += mem * ma.sg;
        if (a.gz[p]) a.gz[p] += mem * ma.s10;
        if (a.gzlp[p]) a.gzlp[p] += mem * ma.s10;
    }
    a.part += mem * a.nblk * 8;
    a.out8 += mem * 8;
    if (a.loss_f32) a.loss_f32 += mem;
    if (a.accum) a.accum += mem;
    a.alpha = r->alpha;
    a.beta = r->beta;
    return a;
}
__global__ void __launch_bounds__(256) flow_loss_rows_multi_kernel(FlowLossMultiArgs ma) {
    const FlowLossArgs a = flow_loss_member(ma, blockIdx.y);
#include "vpc_flow_loss_rows_body.h"
}
__global__ void __launch_bounds__(256) flow_loss_reduce_multi_kernel(FlowLossMultiArgs ma) {
    const FlowLossArgs a = flow_loss_member(ma, blockIdx.y);
#include "vpc_flow_loss_reduce_body.h"
}

}  // namespace vpc

using namespace vpc;

static inline bool flow_rows_ok(long R, long B) { return R > 0 && B > 0 && R % B == 0 && R / B <= 2 && R <= (1L << 26); }

extern "C" {

int vpc_flow_prep(const float* x, const float* mask, const float* mask_p_in, float* mask_p_out, float* xin,
                  float* eps_out, long n_eps, long B, int d, float keep_prob, unsigned long long seed,
                  unsigned long long offset, unsigned long long offset_eps, void* stream) {
    if (!x || !mask || !xin || B <= 0 || d <= 0 || B * d > (1L << 31) || n_eps < 0 || (n_eps > 0 && !eps_out))
        return VPC_ERR_ARG;
    const long groups = (B * d + 3) / 4, ge = (n_eps + 3) / 4;
    const unsigned gm = (unsigned)((groups + 255) / 256), gn = (unsigned)((ge + 255) / 256);
    hipLaunchKernelGGL(flow_prep_kernel, dim3(gm + gn), dim3(256), 0, (hipStream_t)stream, x, mask, mask_p_in,
                       mask_p_out, xin, B, d, keep_prob, eps_out, n_eps, (uint64_t)seed, (uint64_t)offset,
                       (uint64_t)offset_eps, gm);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_flow_fwd(const float* t, long ldt, const float* eps, float* z, float* z_log_prob, long R, long B,
                 void* stream) {
    if (!t || !eps || !z || !z_log_prob || ldt < FLOW_CTX || !flow_rows_ok(R, B)) return VPC_ERR_ARG;
    const long n = R * FLOW_L;
    hipLaunchKernelGGL(flow_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, ldt,
                       eps, z, z_log_prob, R, B);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_flow_bwd(const float* t, long ldt, const float* eps, const float* dz, const float* dz2, const float* dz_log_prob,
                 float* dt, long lddt, long R, long B, void* stream) {
    if (!t || !eps || !dt || ldt < FLOW_CTX || lddt < FLOW_CTX || !flow_rows_ok(R, B)) return VPC_ERR_ARG;
    const long n = R * FLOW_L;
    hipLaunchKernelGGL(flow_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, ldt,
                       eps, dz, dz2, dz_log_prob, dt, lddt, R, B);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

long vpc_flow_loss_scratch(long B) { return B > 0 ? flow_loss_blocks(B) * 8 * 8 : 0; }

// argument checks and the kernels' record of vpc_flow_loss and vpc_flow_loss_multi (one member's arrays)
static int flow_loss_setup(const float* x, const float* mask, const float* mask_p, const float* x_mean_q, const float* x_mean_p,
                           long ldxm, const float* z_q, const float* z_p, const float* z_log_prob_q,
                           const float* z_log_prob_p, float* g_x_mean_q, float* g_x_mean_p, long ldg, float* g_z_q,
                           float* g_z_p, float* g_z_log_prob_q, float* g_z_log_prob_p, void* scratch, double* out8,
                           float* loss_f32, float* accum, long B, int d, int stage, float alpha, float beta, float gscale,
                           int gated, FlowLossArgs& a) {
    if (!x || !mask || !x_mean_q || !z_q || !z_log_prob_q || !scratch || !out8 || B <= 0 || d <= 0 || ldxm < d ||
        B > (1L << 26) || (stage != VPC_FLOW_TRAIN && stage != VPC_FLOW_EVAL))
        return VPC_ERR_ARG;
    const bool reg = mask_p != nullptr, ptrain = reg && stage == VPC_FLOW_TRAIN;
    if (ptrain && (!x_mean_p || !z_p || !z_log_prob_p)) return VPC_ERR_ARG;
    const bool grad = g_x_mean_q != nullptr;
    if (grad && (!g_z_q || !g_z_log_prob_q || ldg < d)) return VPC_ERR_ARG;
    if (grad && reg && (!g_x_mean_p || !g_z_p || !g_z_log_prob_p)) return VPC_ERR_ARG;
    if ((uintptr_t)scratch & 7u) return VPC_ERR_ARG;
    a = FlowLossArgs{};
    a.x = x; a.m = mask; a.mp = mask_p;
    a.xm[0] = x_mean_q; a.xm[1] = x_mean_p; a.ldxm = ldxm;
    a.z[0] = z_q; a.z[1] = z_p; a.zlp[0] = z_log_prob_q; a.zlp[1] = z_log_prob_p;
    a.ldg = ldg;
    if (grad) {
        a.gxm[0] = g_x_mean_q; a.gz[0] = g_z_q; a.gzlp[0] = g_z_log_prob_q;
        if (reg) { a.gxm[1] = g_x_mean_p; a.gz[1] = g_z_p; a.gzlp[1] = g_z_log_prob_p; }
    }
    a.part = (double*)scratch;
    a.out8 = out8; a.loss_f32 = loss_f32; a.accum = accum;
    a.B = (int)B; a.d = d; a.P = mask_p ? 2 : 1; a.eval = stage == VPC_FLOW_EVAL; a.gated = gated;
    a.nblk = (int)flow_loss_blocks(B);
    a.alpha = alpha; a.beta = beta; a.gscale = gscale;
    flow_loss_obs(a);
    return VPC_OK;
}

int vpc_flow_loss(const float* x, const float* mask, const float* mask_p, const float* x_mean_q, const float* x_mean_p,
                  long ldxm, const float* z_q, const float* z_p, const float* z_log_prob_q, const float* z_log_prob_p,
                  float* g_x_mean_q, float* g_x_mean_p, long ldg, float* g_z_q, float* g_z_p, float* g_z_log_prob_q,
                  float* g_z_log_prob_p, void* scratch, long scratch_bytes, double* out8, float* loss_f32, float* accum,
                  long B, int d, int stage, float alpha, float beta, float gscale, int gated, void* stream) {
    FlowLossArgs a;
    const int rc = flow_loss_setup(x, mask, mask_p, x_mean_q, x_mean_p, ldxm, z_q, z_p, z_log_prob_q, z_log_prob_p, g_x_mean_q,
                                   g_x_mean_p, ldg, g_z_q, g_z_p, g_z_log_prob_q, g_z_log_prob_p, scratch, out8, loss_f32,
                                   accum, B, d, stage, alpha, beta, gscale, gated, a);
    if (rc != VPC_OK) return rc;
    if (scratch_bytes < vpc_flow_loss_scratch(B)) return VPC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(flow_loss_rows_kernel, dim3((unsigned)a.nblk), dim3(256), 0, st, a);
    hipLaunchKernelGGL(flow_loss_reduce_kernel, dim3(1), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

// ---- the ensemble entries
static inline bool flow_members_ok(const void* members, int G) { return members && G >= 1 && G <= VPC_FLOW_MULTI_MAX_MEMBERS; }
// a member stride that holds the member's slice; shared = true admits 0 (one array read by every member)
static inline bool flow_stride_ok(long stride, long slice, bool shared = false) {
    return stride >= slice || (shared && stride == 0);
}

int vpc_flow_multi_prep(const float* x, long x_stride, const float* mask, long mask_stride, float* mask_p, long mask_p_stride,
                        float* xin, long xin_stride, float* eps, long eps_stride, const VpcFlowMember* members, int G, int draw,
                        long R, long B, int d, unsigned long long offset, unsigned long long offset_eps, void* stream) {
    if (!x || !mask || !xin || B <= 0 || d <= 0 || B * d > (1L << 31) || !flow_rows_ok(R, B) || !flow_members_ok(members, G))
        return VPC_ERR_ARG;
    const bool two = R == 2 * B;
    if ((two && !mask_p) || (!two && mask_p) || (draw && !eps)) return VPC_ERR_ARG;
    if (!flow_stride_ok(x_stride, B * d, true) || !flow_stride_ok(mask_stride, B * d, true) ||
        (two && !flow_stride_ok(mask_p_stride, B * d)) || !flow_stride_ok(xin_stride, R * 2 * d) ||
        (draw && !flow_stride_ok(eps_stride, R * FLOW_L)))
        return VPC_ERR_ARG;
    const long n_eps = draw ? R * FLOW_L : 0;
    const long groups = (B * d + 3) / 4, ge = (n_eps + 3) / 4;
    const unsigned gm = (unsigned)((groups + 255) / 256), gn = (unsigned)((ge + 255) / 256);
    hipLaunchKernelGGL(flow_prep_multi_kernel, dim3(gm + gn, (unsigned)G), dim3(256), 0, (hipStream_t)stream, x, x_stride, mask,
                       mask_stride, mask_p, mask_p_stride, draw != 0, xin, xin_stride, B, d, draw ? eps : nullptr, n_eps,
                       eps_stride, members, (uint64_t)offset, (uint64_t)offset_eps, gm);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_flow_fwd_multi(const float* t, long ldt, long t_stride, const float* eps, float* z, float* z_log_prob, long stride10,
                       int G, long R, long B, void* stream) {
    if (!t || !eps || !z || !z_log_prob || ldt < FLOW_CTX || !flow_rows_ok(R, B) || G < 1 || G > VPC_FLOW_MULTI_MAX_MEMBERS)
        return VPC_ERR_ARG;
    if (!flow_stride_ok(t_stride, (R - 1) * ldt + FLOW_CTX) || !flow_stride_ok(stride10, R * FLOW_L)) return VPC_ERR_ARG;
    const long n = R * FLOW_L;
    hipLaunchKernelGGL(flow_fwd_multi_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)G), dim3(256), 0, (hipStream_t)stream,
                       t, ldt, t_stride, eps, z, z_log_prob, stride10, R, B);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_flow_bwd_multi(const float* t, long ldt, long t_stride, const float* eps, const float* dz, const float* dz2,
                       const float* dz_log_prob, long stride10, float* dt, long lddt, long dt_stride, int G, long R, long B,
                       void* stream) {
    if (!t || !eps || !dt || ldt < FLOW_CTX || lddt < FLOW_CTX || !flow_rows_ok(R, B) || G < 1 ||
        G > VPC_FLOW_MULTI_MAX_MEMBERS)
        return VPC_ERR_ARG;
    if (!flow_stride_ok(t_stride, (R - 1) * ldt + FLOW_CTX) || !flow_stride_ok(dt_stride, (R - 1) * lddt + FLOW_CTX) ||
        !flow_stride_ok(stride10, R * FLOW_L))
        return VPC_ERR_ARG;
    const long n = R * FLOW_L;
    hipLaunchKernelGGL(flow_bwd_multi_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)G), dim3(256), 0, (hipStream_t)stream,
                       t, ldt, t_stride, eps, dz, dz2, dz_log_prob, stride10, dt, lddt, dt_stride, R, B);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

long vpc_flow_loss_multi_scratch(int G, long B) { return G > 0 ? G * vpc_flow_loss_scratch(B) : 0; }

int vpc_flow_loss_multi(const float* x, long x_stride, const float* mask, long mask_stride, const float* mask_p,
                        long mask_p_stride, const float* x_mean_q, const float* x_mean_p, long ldxm, long x_mean_stride,
                        const float* z_q, const float* z_p, const float* z_log_prob_q, const float* z_log_prob_p,
                        float* g_x_mean_q, float* g_x_mean_p, long ldg, long g_stride, float* g_z_q, float* g_z_p,
                        float* g_z_log_prob_q, float* g_z_log_prob_p, long stride10, void* scratch, long scratch_bytes,
                        double* out8, float* loss_f32, float* accum, const VpcFlowMember* members, int G, long B, int d,
                        int stage, float gscale, int gated, void* stream) {
    FlowLossMultiArgs ma{};
    const int rc = flow_loss_setup(x, mask, mask_p, x_mean_q, x_mean_p, ldxm, z_q, z_p, z_log_prob_q, z_log_prob_p, g_x_mean_q,
                                   g_x_mean_p, ldg, g_z_q, g_z_p, g_z_log_prob_q, g_z_log_prob_p, scratch, out8, loss_f32,
                                   accum, B, d, stage, 0.f, 0.f, gscale, gated, ma.base);
    if (rc != VPC_OK) return rc;
    if (!flow_members_ok(members, G) || scratch_bytes < vpc_flow_loss_multi_scratch(G, B)) return VPC_ERR_ARG;
    const long Rm = (mask_p ? 2 : 1) * B;  // a member's x_mean / z / gradient arrays hold the q rows, then the p rows
    if (!flow_stride_ok(x_stride, B * d, true) || !flow_stride_ok(mask_stride, B * d, true) ||
        (mask_p && !flow_stride_ok(mask_p_stride, B * d)) || !flow_stride_ok(x_mean_stride, (Rm - 1) * ldxm + d) ||
        (g_x_mean_q && !flow_stride_ok(g_stride, (Rm - 1) * ldg + d)) || !flow_stride_ok(stride10, Rm * FLOW_L))
        return VPC_ERR_ARG;
    ma.sx = x_stride; ma.sm = mask_stride; ma.smp = mask_p_stride; ma.sxm = x_mean_stride; ma.s10 = stride10; ma.sg = g_stride;
    ma.members = members;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(flow_loss_rows_multi_kernel, dim3((unsigned)ma.base.nblk, (unsigned)G), dim3(256), 0, st, ma);
    hipLaunchKernelGGL(flow_loss_reduce_multi_kernel, dim3(1, (unsigned)G), dim3(256), 0, st, ma);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
