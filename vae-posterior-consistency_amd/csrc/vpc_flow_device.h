// Device functions of the piecewise-linear CDF posterior (reference src/models/VAE.py: Flow :1816-1854, linear_spline
// :1725-1774) shared by the flow path (vpc_flow.hip) and the flow reward (vpc_flowreward.hip): softmax + cumulative sum
// of a latent's ten masked logits, one spline step, its output and log-determinant, the latent mask of a draw.
#pragma once
#include "vpc_abi_internal.h"

namespace vpc {

constexpr int FLOW_L = VPC_FLOW_LATENT;  // latent dim = bins per spline = 10 (the reference's hard-coded reshape)
constexpr int FLOW_CTX = FLOW_L * FLOW_L;
constexpr float FLOW_HALF_LOG_2PI = 0.91893853320467274f;
constexpr float FLOW_LOG_NBINS = 2.30258509299404568f;  // -np.log(bin_width), bin_width = 1 / 10 (:1768)

// softmax + exclusive cumulative sum of the ten masked logits of latent i (linear_spline :1725-1730)
struct FlowPdf { float pdf[FLOW_L], cdf[FLOW_L]; };  // cdf[k] = sum_{j < k} pdf[j] = F.pad(cumsum)[k]

__device__ __forceinline__ void flow_pdf(const float* __restrict__ t, const float (&m)[FLOW_L], FlowPdf& s) {
    float u[FLOW_L];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < FLOW_L; ++j) {
        u[j] = t[j] * m[j];
        mx = fmaxf(mx, u[j]);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < FLOW_L; ++j) {
        s.pdf[j] = expf(u[j] - mx);
        sum += s.pdf[j];
    }
    const float inv = 1.f / sum;
    float c = 0.f;
#pragma unroll
    for (int j = 0; j < FLOW_L; ++j) {
        s.pdf[j] *= inv;
        s.cdf[j] = c;
        c += s.pdf[j];
    }
}

// one forward spline of an input in [-1, 1] (linear_spline, inverse = False, :1761-1774)
struct FlowStep { int bin; float alpha, pb, o; };  // o: the unclamped [0, 1] output

__device__ __forceinline__ FlowStep flow_step(const FlowPdf& s, float in) {
    FlowStep r;
    const float bp = (in + 1.f) / 2.f * (float)FLOW_L;
    int bin = (int)floorf(bp);
    if (bin >= FLOW_L) bin = FLOW_L - 1;
    r.bin = bin;
    r.alpha = bp - (float)bin;
    float c = 0.f, p = 0.f;
#pragma unroll
    for (int j = 0; j < FLOW_L; ++j)
        if (j == bin) {
            c = s.cdf[j];
            p = s.pdf[j];
        }
    r.pb = p;
    r.o = c + r.alpha * p;
    return r;
}
__device__ __forceinline__ float flow_out(const FlowStep& st) { return fminf(fmaxf(st.o, 0.f), 1.f) * 2.f - 1.f; }
__device__ __forceinline__ float flow_lad(const FlowStep& st) { return logf(st.pb) + FLOW_LOG_NBINS; }

__device__ __forceinline__ void flow_mask(const float* __restrict__ e, float (&m)[FLOW_L]) {
#pragma unroll
    for (int j = 0; j < FLOW_L; ++j) m[j] = fabsf(e[j]) <= 1.f ? 1.f : 0.f;
}

}  // namespace vpc
