// Device helpers of the MIWAE path (reference src/models/VAE.py: MIWAE :3011-3134, Reg_MIWAE :3137-3301): the softplus /
// sigmoid pairs of the sampler and the decoder heads, the Student-t log-density and the wave reductions.  Shared by
// vpc_miw.hip (the elementwise and loss kernels), vpc_miw_small.hip (the small-batch fused step) and vpc_miw_impute.hip (the
// streaming imputation): one definition, included by all, so that the fused stages evaluate the expressions the float64 tests
// hold.
#pragma once
#include <hip/hip_runtime.h>

namespace vpc {

constexpr float MIW_HALF_LOG_PI = 0.57236494292470008f;
constexpr float MIW_HALF_LOG_2PI = 0.91893853320467274f;

__device__ __forceinline__ float miw_softplus(float v) { return v > 20.f ? v : log1pf(expf(v)); }
__device__ __forceinline__ float miw_softplus_d(float v) {  // torch's Softplus backward: identity above the threshold
    if (v > 20.f) return 1.f;
    const float z = expf(v);
    return z / (z + 1.f);
}
__device__ __forceinline__ float miw_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
// sigmoid'(v) = mu (1 - mu) without forming 1 - mu (which loses every digit of it once mu is within rounding of 1)
__device__ __forceinline__ float miw_sigmoid_d(float v) {
    const float z = expf(-fabsf(v));
    return z / ((1.f + z) * (1.f + z));
}

__device__ __forceinline__ float miw_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float miw_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// 0.5 * (digamma((v + 1) / 2) - digamma(v / 2)) for v >= 3, formed as ONE difference: two digammas near log(v / 2) would
// cancel to about 1 / (2 v) and leave their rounding (1e-7 of log(v / 2)) behind, which the df gradient then loses a
// further factor 2 v of against its - 0.5 / v term.  With x_b = v / 2, x_a = x_b + 1/2: the recurrence up to x_b >= 6
// contributes 1 / x_b - 1 / x_a = 0.5 / (x_a x_b) per step, the logarithms of the asymptotic series log1p(0.5 / x_b),
// its - 1 / (2 x) terms 0.25 / (x_a x_b); the remaining series terms are below 3e-3 each.
__device__ __forceinline__ float miw_half_digamma_diff(float v) {
    float xb = 0.5f * v, xa = xb + 0.5f, r = 0.f;
    while (xb < 6.f) {
        r += 0.5f / (xa * xb);
        xa += 1.f;
        xb += 1.f;
    }
    const float ia = 1.f / xa, ib = 1.f / xb, a2 = ia * ia, b2 = ib * ib;
    const float sa = a2 * (1.f / 12.f - a2 * (1.f / 120.f - a2 * (1.f / 252.f)));
    const float sb = b2 * (1.f / 12.f - b2 * (1.f / 120.f - b2 * (1.f / 252.f)));
    return 0.5f * (r + log1pf(0.5f * ib) + 0.25f * ia * ib - (sa - sb));
}

// the three decoder heads of element k of one row: raw != 0 -> apply the transforms of VAE.py:3072-3076
struct MiwHead { float mu, sc, v, a0, a1, a2; };
__device__ __forceinline__ MiwHead miw_head(const float* y, int d, int k, int raw) {
    MiwHead h;
    h.a0 = y[k]; h.a1 = y[d + k]; h.a2 = y[2 * d + k];
    if (raw) {
        h.mu = miw_sigmoid(h.a0);
        h.sc = miw_softplus(h.a1) + 0.001f;
        h.v = miw_softplus(h.a2) + 3.f;
    } else {
        h.mu = h.a0; h.sc = h.a1; h.v = h.a2;
    }
    return h;
}

// StudentT(loc, scale, df).log_prob(x), torch's formula
__device__ __forceinline__ float miw_student_lp(float x, const MiwHead& h) {
    const float y = (x - h.mu) / h.sc;
    const float Z = logf(h.sc) + 0.5f * logf(h.v) + MIW_HALF_LOG_PI + lgammaf(0.5f * h.v) - lgammaf(0.5f * (h.v + 1.f));
    return -0.5f * (h.v + 1.f) * log1pf(y * y / h.v) - Z;
}

}  // namespace vpc
