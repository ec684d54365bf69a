// The body of flow_fwd_kernel and flow_fwd_multi_kernel (vpc_flow.hip), included as text so that both kernels are one piece of code and
// the stand-alone kernel compiles to the instructions it had with these lines spelled out in it.  blockIdx.x is the workgroup's
// index among ONE member's workgroups in both.  In scope at the point of inclusion: `t`, `ldt`, `eps`, `z`, `zlp` (this member's arrays), `R`, `B`.
// (No include guard: a code fragment.)
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long row0 = (long)blockIdx.x * blockDim.x / FLOW_L, row1 = ((long)blockIdx.x + 1) * blockDim.x / FLOW_L;
    bool f0, f1;
    flow_flags(eps, R, B, row0, row1, f0, f1);
    if (g >= R * FLOW_L) return;
    const long r = g / FLOW_L;
    const int i = (int)(g - r * FLOW_L);
    const bool any_inside = r < B ? f0 : f1;  // the predicate of the row's pass
#include "vpc_flow_fwd_elem_body.h"
