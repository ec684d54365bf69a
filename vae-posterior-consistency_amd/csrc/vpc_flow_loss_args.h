// What the kernels of the flow path (vpc_flow.hip) and of the batched flow evaluation (vpc_floweval.hip) share beyond the
// spline itself (vpc_flow_device.h): the wave sum, the batch-global predicate torch.any(|eps| <= 1) over a run of rows, the
// record of the two loss launches and the Gaussian NLL term.  The bodies vpc_flow_loss_rows_body.h /
// vpc_flow_loss_reduce_body.h / vpc_flow_fwd_elem_body.h expect these names in scope.
#pragma once
#include "vpc_flow_device.h"

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

}  // namespace vpc

// one wave per data row: workgroups (= partial blocks) of a loss launch on B rows
static inline long flow_loss_blocks(long B) { return (B + vpc::FLOW_WAVES - 1) / vpc::FLOW_WAVES; }

// x_logvar = obs_logvar * ones = -8 (:1943-1948); scale = exp(logvar / 2): the record's var and log scale
static inline void flow_loss_obs(vpc::FlowLossArgs& a) {
    const float sc = expf(-8.f / 2.f);
    a.var = sc * sc;
    a.logs = logf(sc);
}
