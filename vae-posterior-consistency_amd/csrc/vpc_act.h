// Activation codes of the GEMM layer ops (include/vpc.h: 0 none, 1 ELU, 2 Sigmoid below `split` / Hardtanh(-10, 0) from it on,
// 3 ReLU), their forward and derivative forms and the once-per-tile dispatch.  Shared by vpc_gemm.hip and vpc_rows.hip
// (DESIGN.md section 2.17); moved out of vpc_gemm.hip as they were.
#pragma once
#include <hip/hip_runtime.h>

namespace vpc {

enum { ACT_NONE = 0, ACT_ELU = 1, ACT_SIGMOID_HARDTANH = 2, ACT_RELU = 3 };

// The activation code is a kernel ARGUMENT; it is dispatched ONCE per tile (act_dispatch) into code specialised on it,
// never per element: a per-element `switch` costs a branch forest per value (the first build of the epilogue spent as
// long in it as in the MFMAs of a K = 128 layer).
template <int ACT>
__device__ __forceinline__ float act_fwd(float v, bool second) {
    // hardware exp / rcp (v_exp_f32, v_rcp_f32): |abs err| < 2e-7 on outputs in (-1, 1)
    if (ACT == ACT_ELU) return v > 0.f ? v : __expf(v) - 1.f;
    if (ACT == ACT_SIGMOID_HARDTANH) return second ? __builtin_amdgcn_fmed3f(v, -10.f, 0.f) : __builtin_amdgcn_rcpf(1.f + __expf(-v));
    if (ACT == ACT_RELU) return fmaxf(v, 0.f);
    return v;
}
// derivative of the activation expressed through its OUTPUT y
template <int ACT>
__device__ __forceinline__ float act_grad(float y, bool second) {
    if (ACT == ACT_ELU) return y > 0.f ? 1.f : y + 1.f;
    if (ACT == ACT_SIGMOID_HARDTANH) return second ? ((y > -10.f && y < 0.f) ? 1.f : 0.f) : y * (1.f - y);
    if (ACT == ACT_RELU) return y > 0.f ? 1.f : 0.f;
    return 1.f;
}
template <int V> struct ActC { static constexpr int value = V; };
template <typename F>
__device__ __forceinline__ void act_dispatch(int act, F&& f) {
    switch (act) {
        case ACT_ELU: f(ActC<ACT_ELU>{}); break;
        case ACT_SIGMOID_HARDTANH: f(ActC<ACT_SIGMOID_HARDTANH>{}); break;
        case ACT_RELU: f(ActC<ACT_RELU>{}); break;
        default: f(ActC<ACT_NONE>{}); break;
    }
}

}  // namespace vpc
