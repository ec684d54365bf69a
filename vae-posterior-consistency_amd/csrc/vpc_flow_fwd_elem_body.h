// One (row, latent) element of Flow.forward (VAE.py:1816-1831), the tail of every flow-forward kernel (vpc_flow_fwd_body.h:
// flow_fwd_kernel, flow_fwd_multi_kernel; vpc_floweval.hip: flow_fwd_tiles_kernel), included as text so that all of them run
// one piece of per-element arithmetic.  In scope at the point of inclusion: `t`, `ldt`, `eps`, `z`, `zlp`, the element's flat
// index `g`, its row `r` and latent `i`, and `any_inside` = torch.any(inside) (:1698) of the batch the row belongs to.
// (No include guard: a code fragment.)
    const float e = eps[g];
    const float lp = -(e * e) / 2.f - FLOW_HALF_LOG_2PI;  // Normal(0, 1).log_prob (:1826-1828)
    if (!any_inside) {  // no inside element in this batch: every layer is the identity with logabsdet 0 (:1698)
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
