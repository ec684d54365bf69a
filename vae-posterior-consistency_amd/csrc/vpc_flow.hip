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
#include "vpc_flow_device.h"
#include "vpc_rng.h"

namespace vpc {

constexpr int FLOW_WAVES = 4;

__device__ __forceinline__ float flow_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// torch.any(|eps| <= 1) over the B x 10 draws of one pass; uniform across the workgroup (every thread must call it)
__device__ bool flow_pass_inside(const float* __restrict__ eps, long B, int* sh) {
    const long n = B * FLOW_L;
    const int nw = (int)(blockDim.x >> 6), wv = (int)(threadIdx.x >> 6);
    for (long c = 0; c < n; c += blockDim.x) {
        const long i = c + threadIdx.x;
        const int v = __any(i < n && fabsf(eps[i]) <= 1.f);
        if ((threadIdx.x & 63) == 0) sh[wv] = v;
        __syncthreads();
        int any = 0;
        for (int w = 0; w < nw; ++w) any |= sh[w];
        __syncthreads();  // sh is rewritten by the next chunk
        if (any) return true;
    }
    return false;
}

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
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long row0 = (long)blockIdx.x * blockDim.x / FLOW_L, row1 = ((long)blockIdx.x + 1) * blockDim.x / FLOW_L;
    bool f0, f1;
    flow_flags(eps, R, B, row0, row1, f0, f1);
    if (g >= R * FLOW_L) return;
    const long r = g / FLOW_L;
    const int i = (int)(g - r * FLOW_L);
    const float e = eps[g];
    const float lp = -(e * e) / 2.f - FLOW_HALF_LOG_2PI;  // Normal(0, 1).log_prob (:1826-1828)
    if (!(r < B ? f0 : f1)) {  // no inside element in this pass: every layer is the identity with logabsdet 0 (:1698)
        z[g] = e;
        zlp[g] = lp;
        return;
    }
    float m[FLOW_L];
    flow_mask(eps + r * FLOW_L, m);
    FlowPdf s;
    flow_pdf(t + r * ldt + i * FLOW_L, m, s);
    float in = fabsf(e) <= 1.f ? e : 0.f;  // outside inputs are zeroed, then splined (:1694)
    float ld = 0.f;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const FlowStep st = flow_step(s, in);
        in = flow_out(st);
        ld += flow_lad(st);
    }
    z[g] = in;
    zlp[g] = lp - ld;
}

__global__ void __launch_bounds__(256) flow_bwd_kernel(const float* __restrict__ t, long ldt,
                                                       const float* __restrict__ eps, const float* __restrict__ dz,
                                                       const float* __restrict__ dz2, const float* __restrict__ dzlp,
                                                       float* __restrict__ dt, long lddt, long R, long B) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long row0 = (long)blockIdx.x * blockDim.x / FLOW_L, row1 = ((long)blockIdx.x + 1) * blockDim.x / FLOW_L;
    bool f0, f1;
    flow_flags(eps, R, B, row0, row1, f0, f1);
    if (g >= R * FLOW_L) return;
    const long r = g / FLOW_L;
    const int i = (int)(g - r * FLOW_L);
    float* o = dt + r * lddt + i * FLOW_L;
    if (!(r < B ? f0 : f1)) {  // identity layers: t is not read
#pragma unroll
        for (int j = 0; j < FLOW_L; ++j) o[j] = 0.f;
        return;
    }
    float m[FLOW_L];
    flow_mask(eps + r * FLOW_L, m);
    FlowPdf s;
    flow_pdf(t + r * ldt + i * FLOW_L, m, s);
    FlowStep st[3];
    float in = fabsf(eps[g]) <= 1.f ? eps[g] : 0.f;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        st[l] = flow_step(s, in);
        in = flow_out(st[l]);
    }
    float gout = (dz ? dz[g] : 0.f) + (dz2 ? dz2[g] : 0.f);
    const float glad = dzlp ? -dzlp[g] : 0.f;  // z_log_prob = log_prob - sum of the three logabsdet
    float du[FLOW_L];
#pragma unroll
    for (int j = 0; j < FLOW_L; ++j) du[j] = 0.f;
#pragma unroll
    for (int l = 2; l >= 0; --l) {
        // out = clamp(cdf[bin] + alpha pdf[bin], 0, 1) * 2 - 1; clamp passes the gradient on [0, 1] (torch.clamp)
        const float go = (st[l].o >= 0.f && st[l].o <= 1.f) ? 2.f * gout : 0.f;
        const int bin = st[l].bin;
        float cb = 0.f;
#pragma unroll
        for (int j = 0; j < FLOW_L; ++j)
            if (j == bin) cb = s.cdf[j];
        const float ap = st[l].alpha * st[l].pb;
#pragma unroll
        for (int j = 0; j < FLOW_L; ++j) {
            const float pj = s.pdf[j];
            const float djb = j == bin ? 1.f : 0.f;
            // d cdf[bin] / d u_j = pdf_j ([j < bin] - cdf[bin]),  d pdf[bin] / d u_j = pdf[bin] ([j == bin] - pdf_j)
            du[j] += go * (pj * ((j < bin ? 1.f : 0.f) - cb) + ap * (djb - pj)) + glad * (djb - pj);
        }
        gout = go * (float)FLOW_L * 0.5f * st[l].pb;  // d out / d in = 10 pdf[bin]; layer 1's input (eps) is a leaf
    }
#pragma unroll
    for (int j = 0; j < FLOW_L; ++j) o[j] = du[j] * m[j];  // the in-place context mask of layer 1
}

__global__ void __launch_bounds__(256) flow_prep_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                        const float* __restrict__ mp_in, float* __restrict__ mp_out,
                                                        float* __restrict__ xin, long B, int d, float keep_prob,
                                                        float* __restrict__ eps, long n_eps, uint64_t seed,
                                                        uint64_t offset, uint64_t offset_eps, unsigned gm) {
    if (blockIdx.x >= gm) {
        fill_normal_body(eps, n_eps, seed, offset_eps, (long)(blockIdx.x - gm) * blockDim.x + threadIdx.x,
                         EpsShard{0, 0, 0, 4});
        return;
    }
    const long n = B * d;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i0 = g * 4;
    if (i0 >= n) return;
    const bool two = mp_in || mp_out;
    U4 r{0, 0, 0, 0};
    if (mp_out && !mp_in) r = philox((uint64_t)g + offset, 0u, seed);  // the counters of vpc_nm_prep's mask_p draw
    const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
    for (int j = 0; j < 4 && i0 + j < n; ++j) {
        const long e = i0 + j;
        const long b = e / d;
        const int k = (int)(e - b * d);
        const float xv = x[e], mv = m[e];
        float* q = xin + b * 2 * d;
        q[k] = xv * mv;
        q[d + k] = mv;
        if (two) {
            const float pv = mp_in ? mp_in[e] : (u01(rr[j]) < keep_prob ? mv : 0.f);
            if (mp_out) mp_out[e] = pv;
            float* pp = xin + (B + b) * 2 * d;
            pp[k] = xv * pv;
            pp[d + k] = pv;
        }
    }
}

struct FlowLossArgs {
    const float* x; const float* m; const float* mp;   // [B][d]; mp = nullptr for VAEFlow
    const float* xm[2]; long ldxm;                     // x_mean of the q / p pass, [B][ldxm]
    const float* z[2]; const float* zlp[2];            // [B][10] each
    float* gxm[2]; long ldg; float* gz[2]; float* gzlp[2];  // gradients (gxm[0] nullptr: forward only)
    double* part;                                      // [nblk][8]
    double* out8; float* loss_f32; float* accum;
    int B, d, P, eval, gated, nblk;
    float alpha, beta, gscale, var, logs;
};

// -Normal(loc * w, exp(-8 w / 2)).log_prob(x * w) for a 0/1 weight w (neg_gaussian_log_likelihood, :1987-1989)
__device__ __forceinline__ float flow_nll(const FlowLossArgs& a, float x, float xr, float w) {
    if (w == 0.f) return FLOW_HALF_LOG_2PI;
    const float dv = x - xr;
    return dv * dv / (2.f * a.var) + a.logs + FLOW_HALF_LOG_2PI;
}

// ---- launch 1: one wave per data row b (both passes)
// partial columns: 0 RE_q, 1 RE_p, 2 KL_q, 3 KL_p, 4 KL_reg, 5 NLL of x*mask*~mask_p, 6 RE_q on ~mask
__global__ void __launch_bounds__(256) flow_loss_rows_kernel(FlowLossArgs a) {
    __shared__ float sh[FLOW_WAVES][7];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * FLOW_WAVES + wv;
    const int d = a.d, B = a.B;
    const bool reg = a.P == 2, train = !a.eval;
    const bool pp = reg && train;  // the p pass enters the loss
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (b < B) {
        const float* x = a.x + (long)b * d;
        const float* mq = a.m + (long)b * d;
        const float* mpp = reg ? a.mp + (long)b * d : nullptr;
        const float* xq = a.xm[0] + (long)b * a.ldxm;
        const float* xp = pp ? a.xm[1] + (long)b * a.ldxm : nullptr;
        const float al = a.alpha;
        // coefficients of the unscaled loss: REG train loss_q + alpha (KL_reg - loss_q + loss_p + NLL_r) (:2086-2093)
        const float c_q = pp ? 1.f - al : 1.f, c_r = pp ? al : 0.f, c_p = pp ? al : 0.f;
        const float gs = a.gscale / a.var;
        for (int k = lane; k < d; k += 64) {
            const float xv = x[k], m = mq[k], rq = xq[k];
            acc[0] += flow_nll(a, xv, rq, m);
            acc[6] += flow_nll(a, xv, rq, 1.f - m);
            float wr = 0.f;
            if (reg) {
                wr = m * (1.f - mpp[k]);
                acc[5] += flow_nll(a, xv, rq, wr);
            }
            if (a.gxm[0]) {
                float gq = (c_q * m + c_r * wr) * (rq - xv) * gs;
                if (a.gated) gq *= rq * (1.f - rq);
                a.gxm[0][(long)b * a.ldg + k] = gq;
                if (a.gxm[1]) {
                    float gp = 0.f;
                    if (pp) {
                        const float rp = xp[k];
                        gp = c_p * mpp[k] * (rp - xv) * gs;
                        if (a.gated) gp *= rp * (1.f - rp);
                    }
                    a.gxm[1][(long)b * a.ldg + k] = gp;
                }
            }
            if (pp) acc[1] += flow_nll(a, xv, xp[k], mpp[k]);
        }
        if (lane < FLOW_L) {
            const long iq = (long)b * FLOW_L + lane;
            const float zq = a.z[0][iq], lq = a.zlp[0][iq];
            acc[2] = lq - (-(zq * zq) / 2.f - FLOW_HALF_LOG_2PI);  // z_log_prob - prior.log_prob(z)
            float sgn = 0.f;
            if (pp) {
                const float zp = a.z[1][iq], lpp = a.zlp[1][iq];
                acc[3] = lpp - (-(zp * zp) / 2.f - FLOW_HALF_LOG_2PI);
                acc[4] = fabsf(lq - lpp);
                sgn = lq > lpp ? 1.f : (lq < lpp ? -1.f : 0.f);
                if (a.gz[1]) {
                    a.gz[1][iq] = a.gscale * c_p * a.beta * zp;
                    a.gzlp[1][iq] = a.gscale * (c_p * a.beta - al * sgn);
                }
            } else if (a.gz[1]) {  // REG evaluate stage: the p pass does not enter the loss
                a.gz[1][iq] = 0.f;
                a.gzlp[1][iq] = 0.f;
            }
            if (a.gz[0]) {
                a.gz[0][iq] = a.gscale * c_q * a.beta * zq;
                a.gzlp[0][iq] = a.gscale * (c_q * a.beta + al * sgn);
            }
        }
#pragma unroll
        for (int c = 0; c < 7; ++c) acc[c] = flow_wave_sum(acc[c]);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 7; ++c) sh[wv][c] = acc[c];
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        double s = 0.0;
        for (int w = 0; w < FLOW_WAVES; ++w) s += (double)sh[w][threadIdx.x];
        a.part[(long)blockIdx.x * 8 + threadIdx.x] = s;
    }
}

// ---- launch 2: one workgroup; column c of the partials summed by 32 lanes in a strided fixed order, then in lane order
__global__ void __launch_bounds__(256) flow_loss_reduce_kernel(FlowLossArgs a) {
    __shared__ double sh[8][33];
    const int c = threadIdx.x >> 5, l = threadIdx.x & 31;
    double s = 0.0;
    if (c < 7)
        for (int i = l; i < a.nblk; i += 32) s += a.part[(long)i * 8 + c];
    sh[c][l] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[7];
        for (int k = 0; k < 7; ++k) {
            double u = 0.0;
            for (int j = 0; j < 32; ++j) u += sh[k][j];
            t[k] = u;
        }
        const double al = a.alpha, be = a.beta;
        const double loss_q = t[0] + be * t[2];
        double loss = loss_q;
        if (a.P == 2 && !a.eval) loss = loss_q + al * (t[4] - loss_q + (t[1] + be * t[3]) + t[5]);
        double* o = a.out8;
        o[0] = loss;   // unscaled; train_loss = loss / B
        o[1] = t[0];   // RE_q (VAEFlow: RE_)
        o[2] = t[1];   // RE_p
        o[3] = t[2];   // KL_q
        o[4] = t[3];   // KL_p
        o[5] = t[4];   // KL_reg
        o[6] = t[5];   // NLL of x * mask * ~mask_p
        o[7] = t[6];   // RE_q_imputed (NLL on ~mask)
        const float tl = (float)(loss / a.B);
        if (a.loss_f32) a.loss_f32[0] = tl;
        if (a.accum) a.accum[0] += tl;
    }
}

}  // namespace vpc

using namespace vpc;

static inline long flow_loss_blocks(long B) { return (B + FLOW_WAVES - 1) / FLOW_WAVES; }

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

int vpc_flow_loss(const float* x, const float* mask, const float* mask_p, const float* x_mean_q, const float* x_mean_p,
                  long ldxm, const float* z_q, const float* z_p, const float* z_log_prob_q, const float* z_log_prob_p,
                  float* g_x_mean_q, float* g_x_mean_p, long ldg, float* g_z_q, float* g_z_p, float* g_z_log_prob_q,
                  float* g_z_log_prob_p, void* scratch, long scratch_bytes, double* out8, float* loss_f32, float* accum,
                  long B, int d, int stage, float alpha, float beta, float gscale, int gated, void* stream) {
    if (!x || !mask || !x_mean_q || !z_q || !z_log_prob_q || !scratch || !out8 || B <= 0 || d <= 0 || ldxm < d ||
        B > (1L << 26) || (stage != VPC_FLOW_TRAIN && stage != VPC_FLOW_EVAL))
        return VPC_ERR_ARG;
    const bool reg = mask_p != nullptr, ptrain = reg && stage == VPC_FLOW_TRAIN;
    if (ptrain && (!x_mean_p || !z_p || !z_log_prob_p)) return VPC_ERR_ARG;
    const bool grad = g_x_mean_q != nullptr;
    if (grad && (!g_z_q || !g_z_log_prob_q || ldg < d)) return VPC_ERR_ARG;
    if (grad && reg && (!g_x_mean_p || !g_z_p || !g_z_log_prob_p)) return VPC_ERR_ARG;
    if (scratch_bytes < vpc_flow_loss_scratch(B) || ((uintptr_t)scratch & 7u)) return VPC_ERR_ARG;
    FlowLossArgs a{};
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
    const float sc = expf(-8.f / 2.f);  // x_logvar = obs_logvar * ones = -8 (:1943-1948); scale = exp(logvar / 2)
    a.var = sc * sc;
    a.logs = logf(sc);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(flow_loss_rows_kernel, dim3((unsigned)a.nblk), dim3(256), 0, st, a);
    hipLaunchKernelGGL(flow_loss_reduce_kernel, dim3(1), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
