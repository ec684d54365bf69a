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
