// Device helpers of the MNAR path (reference src/models/VAE.py: REG_notMIWAE_v2 :2327-2505, notMIWAE_myversion :2691-2847):
// the constant of the Gaussian log-density and the scalar softplus / sigmoid of the self-masking missingness model.  Shared by
// vpc_nm.hip (the fused loss kernel) and vpc_nm_impute.hip (the streaming imputation): one definition, included by both.
#pragma once
#include <hip/hip_runtime.h>

namespace vpc {

constexpr float NM_HALF_LOG_2PI = 0.91893853320467274f;

// hardware exp / log / rcp (v_exp_f32, v_log_f32, v_rcp_f32: <= 1-2 ulp) for the per-element work of the loss kernel;
// the once-per-workgroup W transforms and the scalar log-sum-exp keep the IEEE routines
__device__ __forceinline__ float fexp(float v) { return __expf(v); }
__device__ __forceinline__ float frcp(float v) { return __builtin_amdgcn_rcpf(v); }
__device__ __forceinline__ float softplus_f(float v) { return v > 20.f ? v : log1pf(expf(v)); }
__device__ __forceinline__ float sigmoid_f(float v) {
    const float e = expf(-fabsf(v));
    return v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

}  // namespace vpc
