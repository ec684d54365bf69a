// The body of flow_bwd_kernel and flow_bwd_multi_kernel (vpc_flow.hip), included as text so that both kernels are one piece of code and
// the stand-alone kernel compiles to the instructions it had with these lines spelled out in it.  blockIdx.x is the workgroup's
// index among ONE member's workgroups in both.  In scope at the point of inclusion: `t`, `ldt`, `eps`, `dz`, `dz2`, `dzlp`, `dt`, `lddt` (this member's arrays), `R`, `B`.
// (No include guard: a code fragment.)
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
