// Elementwise / reduction kernels of the MIWAE path (reference src/models/VAE.py: MIWAE :3011-3134, Reg_MIWAE
// :3137-3301).  The layers are the generic fp32 GEMMs of vpc_gemm.hip; what is specific to the family runs here:
//
//   miw_sample     z[b,s,:] = mean[b] + softplus(raw[b]) * eps[b,s,:]                     (encoder :3059-3070 / :3188-3200)
//   miw_heads      (sigmoid | softplus + 0.001 | softplus + 3) of the [M][3d] decoder head GEMM     (decoder :3072-3076)
//   miw_loss       Student-t importance-weighted bound, forward and backward, in three launches:
//                    rows   per (pass, row, sample): masked Student-t sums, logpz - logq on the fresh draw, KL_reg
//                    slots  per (pass, slot): log-sum-exp with the reference's row/sample pairing, the softmax weights
//                           (scaled into gradient seeds), fixed-order loss partials, the llh_eval imputation
//                    grad   per element: decoder-head gradients; per (pass, row, l): encoder-head gradients; one
//                           workgroup reduces the loss partials in a fixed order into out8
//
// The pairing couples rows across the whole batch, so the exchange between the per-row sums and the per-slot
// log-sum-exp goes through a scratch buffer between launches.  No float atomics; bit-reproducible.
#include "vpc_abi_internal.h"
#include "../../include/vpc.h"
#include "vpc_miw_device.h"

namespace vpc {

constexpr int MIW_WAVES = 4;  // waves per 256-thread workgroup of the row / slot kernels

struct MiwLossArgs {
    const float* x; const float* m; const float* mp;   // [B][d]; mp = nullptr for MIWAE
    const float* y[2]; long ldy; int raw;               // decoder heads of the q / p pass, rows b*S+s, [mean d | scale d | df d]
    const float* h[2];                                  // encoder heads [B][mean L | scale L] (activated)
    const float* e[2];                                  // fresh draws of loss(), [B][S][L]
    float* gy[2]; long ldg;                             // gradients w.r.t. the decoder heads (raw or activated as `raw`)
    float* gh[2];                                       // gradients w.r.t. the activated encoder heads [B][2L]
    float* xm_imp;                                      // [B][d] or nullptr
    float* lpo[2]; float* lw[2]; float* gpo[2]; float* gw[2];  // [B*S] each
    float* lpm; float* rl; float* kl;                   // [B*S], [B*S], [B]
    double* part;                                       // [nslot_blocks][8]
    double* out8; float* loss_f32; float* accum;
    int B, S, d, L, P, pairing, nslot_blocks;
    float alpha;
};

// ---- launch 1: one wave per (pass, row b, sample s)
__global__ void __launch_bounds__(256) miw_rows_kernel(MiwLossArgs a) {
    const int lane = threadIdx.x & 63;
    const long N = (long)a.B * a.S;
    const long gw = (long)blockIdx.x * MIW_WAVES + (threadIdx.x >> 6);
    if (gw >= a.P * N) return;
    const int p = (int)(gw / N);
    const long r = gw - p * N;
    const int b = (int)(r / a.S), s = (int)(r - (long)b * a.S);
    const int d = a.d, L = a.L;
    const float* x = a.x + (long)b * d;
    const float* mq = a.m + (long)b * d;
    const float* mpp = a.mp ? a.mp + (long)b * d : nullptr;
    const float* mrow = p == 0 ? mq : mpp;
    const float* y = a.y[p] + r * a.ldy;
    float so = 0.f, sm = 0.f, sr = 0.f;
    for (int k = lane; k < d; k += 64) {
        const MiwHead h = miw_head(y, d, k, a.raw);
        const float lp = miw_student_lp(x[k], h);
        so += lp * mrow[k];
        if (p == 0) {
            sm += lp * (1.f - mq[k]);
            if (mpp) sr += lp * mq[k] * (1.f - mpp[k]);
        }
    }
    // logpz - logq of the fresh draw z2 = mean + scale * e (VAE.py:3087-3091 / :3216-3220, :3237-3240)
    const float* hh = a.h[p] + (long)b * 2 * L;
    const float* e = a.e[p] + r * L;
    float slw = 0.f;
    for (int l = lane; l < L; l += 64) {
        const float mu = hh[l], sc = hh[L + l];
        const float z = mu + sc * e[l];
        const float dz = z - mu;
        const float lpz = -0.5f * z * z - MIW_HALF_LOG_2PI;
        const float lq = -(dz * dz) / (2.f * sc * sc) - logf(sc) - MIW_HALF_LOG_2PI;
        slw += lpz - lq;
    }
    so = miw_wave_sum(so);
    slw = miw_wave_sum(slw);
    if (p == 0) {
        sm = miw_wave_sum(sm);
        sr = miw_wave_sum(sr);
    }
    float skl = 0.f;
    const bool do_kl = p == 0 && a.P == 2 && s == 0;
    if (do_kl) {  // KL(N(mean_q, scale_q) || N(mean_p, scale_p)) summed over l (VAE.py:3249, :3253-3258)
        const float* hp = a.h[1] + (long)b * 2 * L;
        for (int l = lane; l < L; l += 64) {
            const float r1 = hh[L + l] / hp[L + l];
            const float vr = r1 * r1;
            const float t1 = (hh[l] - hp[l]) / hp[L + l];
            skl += 0.5f * (vr + t1 * t1 - 1.f - logf(vr));
        }
        skl = miw_wave_sum(skl);
    }
    if (lane == 0) {
        a.lpo[p][r] = so;
        a.lw[p][r] = slw;
        if (p == 0) {
            a.lpm[r] = sm;
            if (a.P == 2) a.rl[r] = sr;
        }
        if (do_kl) a.kl[b] = skl;
    }
}

// the row of the likelihood term in slot (i, j): reference pairing = flat index i*B + j of the [S, B] reshape of the
// (row, sample)-ordered sums (VAE.py:3078-3081); per-row pairing = row j, sample i
__device__ __forceinline__ long miw_lpo_row(int pairing, int i, int j, int B, int S) {
    return pairing == VPC_MIW_PAIR_REFERENCE ? (long)i * B + j : (long)j * S + i;
}

// ---- launch 2: one wave per slot j, both passes; four waves per workgroup -> one row of partials per workgroup
__global__ void __launch_bounds__(256) miw_slots_kernel(MiwLossArgs a) {
    __shared__ double sh[MIW_WAVES][5];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = blockIdx.x * MIW_WAVES + wv;
    const int B = a.B, S = a.S;
    float lse[2] = {0.f, 0.f}, srl = 0.f, skl = 0.f, slm = 0.f;
    if (j < B) {
        for (int p = 0; p < a.P; ++p) {
            float mx = -INFINITY;
            for (int i = lane; i < S; i += 64)
                mx = fmaxf(mx, a.lpo[p][miw_lpo_row(a.pairing, i, j, B, S)] + a.lw[p][(long)j * S + i]);
            mx = miw_wave_max(mx);
            float se = 0.f;
            for (int i = lane; i < S; i += 64)
                se += expf(a.lpo[p][miw_lpo_row(a.pairing, i, j, B, S)] + a.lw[p][(long)j * S + i] - mx);
            se = miw_wave_sum(se);
            lse[p] = mx + logf(se);
            // gradient seed of the slot: d loss / d a[i, j] = coef * softmax_i
            const float coef = a.P == 2 ? (p == 0 ? -(1.f - a.alpha) : -a.alpha) / B : -1.f / B;
            if (a.gy[0]) {
                for (int i = lane; i < S; i += 64) {
                    const long ro = miw_lpo_row(a.pairing, i, j, B, S), rw = (long)j * S + i;
                    const float w = expf(a.lpo[p][ro] + a.lw[p][rw] - lse[p]);
                    a.gpo[p][ro] = coef * w;
                    a.gw[p][rw] = coef * w;
                }
            }
        }
        // llh_eval: the q-pass weights of slot j applied to the un-mixed x_mean[j, i, :] (VAE.py:3096-3098 / :3267-3269)
        if (a.xm_imp) {
            for (int k = lane; k < a.d; k += 64) {
                float acc = 0.f;
                for (int i = 0; i < S; ++i) {
                    const long rw = (long)j * S + i;
                    const float w = expf(a.lpo[0][miw_lpo_row(a.pairing, i, j, B, S)] + a.lw[0][rw] - lse[0]);
                    const float* y = a.y[0] + rw * a.ldy;
                    acc += w * (a.raw ? miw_sigmoid(y[k]) : y[k]);
                }
                a.xm_imp[(long)j * a.d + k] = acc;
            }
        }
        // per-row sums of the same workgroup's rows (rows j*S .. j*S + S - 1)
        for (int s = lane; s < S; s += 64) {
            slm += a.lpm[(long)j * S + s];
            if (a.P == 2) srl += a.rl[(long)j * S + s];
        }
        slm = miw_wave_sum(slm);
        srl = miw_wave_sum(srl);
        if (a.P == 2) skl = a.kl[j];
    }
    if (lane == 0) {
        sh[wv][0] = lse[0]; sh[wv][1] = lse[1]; sh[wv][2] = srl; sh[wv][3] = skl; sh[wv][4] = slm;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        double t = 0.0;
        for (int w = 0; w < MIW_WAVES; ++w) t += sh[w][threadIdx.x];
        a.part[(long)blockIdx.x * 8 + threadIdx.x] = t;
    }
}

// ---- launch 3: gradients + the fixed-order loss reduction
__global__ void __launch_bounds__(256) miw_grad_kernel(MiwLossArgs a, int nblk_elem, int nblk_head) {
    const int B = a.B, S = a.S, d = a.d, L = a.L;
    const long N = (long)B * S;
    if ((int)blockIdx.x < nblk_elem) {
        const long t = (long)blockIdx.x * 256 + threadIdx.x;
        if (t >= a.P * N * d) return;
        const int p = (int)(t / (N * d));
        const long rem = t - p * N * d;
        const long r = rem / d;
        const int k = (int)(rem - r * d);
        const int b = (int)(r / S);
        const float mq = a.m[(long)b * d + k];
        const float mv = p == 0 ? mq : a.mp[(long)b * d + k];
        float g = a.gpo[p][r] * mv;
        if (p == 0 && a.P == 2) g -= a.alpha / (float)N * mq * (1.f - a.mp[(long)b * d + k]);  // - alpha * reg_like
        const MiwHead h = miw_head(a.y[p] + r * a.ldy, d, k, a.raw);
        const float x = a.x[(long)b * d + k];
        const float y = (x - h.mu) / h.sc;
        const float tt = y * y / h.v, u = 1.f + tt;
        float gmu = g * (h.v + 1.f) * y / (h.v * h.sc * u);
        float gsc = g * (-1.f / h.sc + (h.v + 1.f) * tt / (h.sc * u));
        float gv = g * (miw_half_digamma_diff(h.v) - 0.5f / h.v - 0.5f * log1pf(tt) + (h.v + 1.f) * tt / (2.f * h.v * u));
        if (a.raw) {
            gmu *= miw_sigmoid_d(h.a0);
            gsc *= miw_softplus_d(h.a1);
            gv *= miw_softplus_d(h.a2);
        }
        float* go = a.gy[p] + r * a.ldg;
        go[k] = gmu;
        go[d + k] = gsc;
        go[2 * d + k] = gv;
        return;
    }
    if ((int)blockIdx.x < nblk_elem + nblk_head) {
        const long t = (long)(blockIdx.x - nblk_elem) * 256 + threadIdx.x;
        if (t >= (long)a.P * B * L) return;
        const int p = (int)(t / ((long)B * L));
        const long rem = t - (long)p * B * L;
        const int b = (int)(rem / L), l = (int)(rem - (long)b * L);
        const float* hh = a.h[p] + (long)b * 2 * L;
        const float mu = hh[l], sc = hh[L + l];
        float gm = 0.f, gs = 0.f;
        for (int s = 0; s < S; ++s) {  // d(logpz - logq)/d mean = -z2, d/d scale = -z2 e + 1/scale
            const long r = (long)b * S + s;
            const float e = a.e[p][r * L + l];
            const float z = mu + sc * e;
            const float w = a.gw[p][r];
            gm -= w * z;
            gs += w * (1.f / sc - z * e);
        }
        if (a.P == 2) {  // + alpha * d KL_reg, KL_reg = mean over [B, S, L] (each (b, l) S times)
            const float* hq = a.h[0] + (long)b * 2 * L;
            const float* hp = a.h[1] + (long)b * 2 * L;
            const float mq = hq[l], sq = hq[L + l], mp = hp[l], sp = hp[L + l];
            const float c = a.alpha / ((float)B * L);
            const float dm = mq - mp, isp2 = 1.f / (sp * sp);
            if (p == 0) {
                gm += c * dm * isp2;
                gs += c * (sq * isp2 - 1.f / sq);
            } else {
                gm -= c * dm * isp2;
                gs += c * (1.f / sp - (sq * sq + dm * dm) * isp2 / sp);
            }
        }
        float* go = a.gh[p] + (long)b * 2 * L;
        go[l] = gm;
        go[L + l] = gs;
        return;
    }
    // the last workgroup: loss partials of the slot launch, summed in block order
    __shared__ double tot[5];
    if (threadIdx.x < 5) {
        double t = 0.0;
        for (int i = 0; i < a.nslot_blocks; ++i) t += a.part[(long)i * 8 + threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double nb_q = -tot[0] / B;
        const double nb_p = a.P == 2 ? -tot[1] / B : 0.0;
        const double reg_like = tot[2] / (double)N;
        const double kl = tot[3] / ((double)B * L);
        const double al = a.alpha;
        const double loss = a.P == 2 ? nb_q + al * (kl - nb_q + nb_p - reg_like) : nb_q;  // VAE.py:3250-3251
        double* o = a.out8;
        o[0] = loss; o[1] = nb_q; o[2] = nb_p; o[3] = kl; o[4] = reg_like;
        o[5] = tot[4] / ((double)B * 5000.0);  // VAE.py:3099: logpxobsgivenz_imp.sum() / (B * 5000), a literal
        o[6] = tot[0]; o[7] = tot[1];
        if (a.loss_f32) a.loss_f32[0] = (float)loss;
        if (a.accum) a.accum[0] += (float)loss;
    }
}

__global__ void miw_sample_kernel(const float* __restrict__ heads, float* __restrict__ hact, const float* __restrict__ eps,
                                  float* __restrict__ z, long R, int S, int L) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * S * L) return;
    const long r = t / ((long)S * L);
    const long rem = t - r * S * L;
    const int s = (int)(rem / L), l = (int)(rem - (long)s * L);
    const float mu = heads[r * 2 * L + l];
    const float sc = miw_softplus(heads[r * 2 * L + L + l]);
    z[t] = eps ? mu + eps[t] * sc : mu;
    if (hact && s == 0) {
        hact[r * 2 * L + l] = mu;
        hact[r * 2 * L + L + l] = sc;
    }
}

__global__ void miw_sample_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ eps,
                                      const float* __restrict__ heads, const float* __restrict__ g_hact,
                                      float* __restrict__ out, long R, int S, int L) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * L) return;
    const long r = t / L;
    const int l = (int)(t - r * L);
    float gm = g_hact ? g_hact[r * 2 * L + l] : 0.f;
    float gs = g_hact ? g_hact[r * 2 * L + L + l] : 0.f;
    if (dz) {
        for (int s = 0; s < S; ++s) {
            const long i = (r * S + s) * L + l;
            gm += dz[i];
            if (eps) gs += dz[i] * eps[i];
        }
    }
    out[r * 2 * L + l] = gm;
    out[r * 2 * L + L + l] = gs * miw_softplus_d(heads[r * 2 * L + L + l]);
}

__global__ void miw_heads_kernel(const float* __restrict__ yr, const float* __restrict__ gact, float* __restrict__ out,
                                 long M, int d) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M * d) return;
    const long m = t / d;
    const int k = (int)(t - m * d);
    const float* y = yr + m * 3 * d;
    float* o = out + m * 3 * d;
    if (!gact) {
        const MiwHead h = miw_head(y, d, k, 1);
        o[k] = h.mu; o[d + k] = h.sc; o[2 * d + k] = h.v;
        return;
    }
    const float* g = gact + m * 3 * d;
    o[k] = g[k] * miw_sigmoid_d(y[k]);
    o[d + k] = g[d + k] * miw_softplus_d(y[d + k]);
    o[2 * d + k] = g[2 * d + k] * miw_softplus_d(y[2 * d + k]);
}

}  // namespace vpc

using namespace vpc;

static inline long miw_slot_blocks(long B) { return (B + MIW_WAVES - 1) / MIW_WAVES; }

extern "C" {

int vpc_miw_sample(const float* heads, float* hact, const float* eps, float* z, long R, int S, int L, void* stream) {
    if (!heads || !z || R <= 0 || S <= 0 || L <= 0) return VPC_ERR_ARG;
    const long n = R * S * L;
    hipLaunchKernelGGL(miw_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, heads,
                       hact, eps, z, R, S, L);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_sample_bwd(const float* dz, const float* eps, const float* heads, const float* g_hact, float* out, long R,
                       int S, int L, void* stream) {
    if (!heads || !out || R <= 0 || S <= 0 || L <= 0) return VPC_ERR_ARG;
    const long n = R * L;
    hipLaunchKernelGGL(miw_sample_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dz,
                       eps, heads, g_hact, out, R, S, L);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_heads(const float* y_raw, float* y_act, long M, int d, void* stream) {
    if (!y_raw || !y_act || M <= 0 || d <= 0) return VPC_ERR_ARG;
    const long n = M * d;
    hipLaunchKernelGGL(miw_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y_raw,
                       (const float*)nullptr, y_act, M, d);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_heads_bwd(const float* y_raw, const float* g_act, float* g_raw, long M, int d, void* stream) {
    if (!y_raw || !g_act || !g_raw || M <= 0 || d <= 0) return VPC_ERR_ARG;
    const long n = M * d;
    hipLaunchKernelGGL(miw_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y_raw,
                       g_act, g_raw, M, d);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

long vpc_miw_loss_scratch(long B, int S) {
    const long N = B * S;
    const long floats = 2 * 4 * N + 2 * N + B;  // lpo lw gpo gw per pass, lpm rl, kl
    return ((floats * 4 + 63) / 64) * 64 + miw_slot_blocks(B) * 8 * 8;
}

int vpc_miw_loss(const float* x, const float* mask, const float* mask_p, const float* y_q, const float* y_p, long ldy,
                 int raw, const float* heads_q, const float* heads_p, const float* eps_q, const float* eps_p,
                 float* g_y_q, float* g_y_p, long ldg, float* g_heads_q, float* g_heads_p, float* xm_imp,
                 void* scratch, long scratch_bytes, double* out8, float* loss_f32, float* accum, long B, int S, int d,
                 int L, double alpha, int pairing, void* stream) {
    const bool reg = mask_p != nullptr;
    if (!x || !mask || !y_q || !heads_q || !eps_q || !scratch || !out8 || B <= 0 || S <= 0 || d <= 0 || L <= 0 ||
        ldy < 3 * d || B * S > (1L << 30))
        return VPC_ERR_ARG;
    if (reg && (!y_p || !heads_p || !eps_p)) return VPC_ERR_ARG;
    if (pairing != VPC_MIW_PAIR_REFERENCE && pairing != VPC_MIW_PAIR_PER_ROW) return VPC_ERR_ARG;
    const bool grad = g_y_q != nullptr;
    if (grad && (!g_heads_q || ldg < 3 * d || (reg && (!g_y_p || !g_heads_p)))) return VPC_ERR_ARG;
    if (scratch_bytes < vpc_miw_loss_scratch(B, S) || ((uintptr_t)scratch & 7u)) return VPC_ERR_ARG;
    const long N = B * S;
    MiwLossArgs a{};
    a.x = x; a.m = mask; a.mp = mask_p;
    a.y[0] = y_q; a.y[1] = y_p; a.ldy = ldy; a.raw = raw;
    a.h[0] = heads_q; a.h[1] = heads_p;
    a.e[0] = eps_q; a.e[1] = eps_p;
    a.gy[0] = g_y_q; a.gy[1] = g_y_p; a.ldg = ldg;
    a.gh[0] = g_heads_q; a.gh[1] = g_heads_p;
    a.xm_imp = xm_imp;
    float* f = (float*)scratch;
    for (int p = 0; p < 2; ++p) {
        a.lpo[p] = f; f += N;
        a.lw[p] = f; f += N;
        a.gpo[p] = f; f += N;
        a.gw[p] = f; f += N;
    }
    a.lpm = f; f += N;
    a.rl = f; f += N;
    a.kl = f; f += B;
    const long fbytes = (((long)(f - (float*)scratch) * 4 + 63) / 64) * 64;
    a.part = (double*)((char*)scratch + fbytes);
    a.out8 = out8; a.loss_f32 = loss_f32; a.accum = accum;
    a.B = (int)B; a.S = S; a.d = d; a.L = L; a.P = reg ? 2 : 1; a.pairing = pairing;
    a.nslot_blocks = (int)miw_slot_blocks(B);
    a.alpha = (float)alpha;
    hipStream_t st = (hipStream_t)stream;
    const long rows = a.P * N;
    hipLaunchKernelGGL(miw_rows_kernel, dim3((unsigned)((rows + MIW_WAVES - 1) / MIW_WAVES)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(miw_slots_kernel, dim3((unsigned)a.nslot_blocks), dim3(256), 0, st, a);
    const long ne = grad ? (a.P * N * d + 255) / 256 : 0;
    const long nh = grad ? ((long)a.P * B * L + 255) / 256 : 0;
    if (ne + nh + 1 > 0x7fffffffL) return VPC_ERR_ARG;
    hipLaunchKernelGGL(miw_grad_kernel, dim3((unsigned)(ne + nh + 1)), dim3(256), 0, st, a, (int)ne, (int)nh);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
