// The body of flow_loss_rows_kernel and flow_loss_rows_multi_kernel (vpc_flow.hip), included as text so that both kernels are one piece of code and
// the stand-alone kernel compiles to the instructions it had with these lines spelled out in it.  blockIdx.x is the workgroup's
// index among ONE member's workgroups in both.  In scope at the point of inclusion: `a` (FlowLossArgs: this member's arrays and coefficients).
// (No include guard: a code fragment.)
    __shared__ float sh[FLOW_WAVES][7];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * FLOW_WAVES + wv;
    const int d = a.d, B = a.B;
    const bool reg = a.P == 2, train = !a.eval;
    const bool pp = reg && train;  // the p pass enters the loss
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (b < B) {
        const float* x = a.x + (long)b * d;
        const float* mq = a.m + (long)b * d;
        const float* mpp = reg ? a.mp + (long)b * d : nullptr;
        const float* xq = a.xm[0] + (long)b * a.ldxm;
        const float* xp = pp ? a.xm[1] + (long)b * a.ldxm : nullptr;
        const float al = a.alpha;
        // coefficients of the unscaled loss: REG train loss_q + alpha (KL_reg - loss_q + loss_p + NLL_r) (:2086-2093)
        const float c_q = pp ? 1.f - al : 1.f, c_r = pp ? al : 0.f, c_p = pp ? al : 0.f;
        const float gs = a.gscale / a.var;
        for (int k = lane; k < d; k += 64) {
            const float xv = x[k], m = mq[k], rq = xq[k];
            acc[0] += flow_nll(a, xv, rq, m);
            acc[6] += flow_nll(a, xv, rq, 1.f - m);
            float wr = 0.f;
            if (reg) {
                wr = m * (1.f - mpp[k]);
                acc[5] += flow_nll(a, xv, rq, wr);
            }
            if (a.gxm[0]) {
                float gq = (c_q * m + c_r * wr) * (rq - xv) * gs;
                if (a.gated) gq *= rq * (1.f - rq);
                a.gxm[0][(long)b * a.ldg + k] = gq;
                if (a.gxm[1]) {
                    float gp = 0.f;
                    if (pp) {
                        const float rp = xp[k];
                        gp = c_p * mpp[k] * (rp - xv) * gs;
                        if (a.gated) gp *= rp * (1.f - rp);
                    }
                    a.gxm[1][(long)b * a.ldg + k] = gp;
                }
            }
            if (pp) acc[1] += flow_nll(a, xv, xp[k], mpp[k]);
        }
        if (lane < FLOW_L) {
            const long iq = (long)b * FLOW_L + lane;
            const float zq = a.z[0][iq], lq = a.zlp[0][iq];
            acc[2] = lq - (-(zq * zq) / 2.f - FLOW_HALF_LOG_2PI);  // z_log_prob - prior.log_prob(z)
            float sgn = 0.f;
            if (pp) {
                const float zp = a.z[1][iq], lpp = a.zlp[1][iq];
                acc[3] = lpp - (-(zp * zp) / 2.f - FLOW_HALF_LOG_2PI);
                acc[4] = fabsf(lq - lpp);
                sgn = lq > lpp ? 1.f : (lq < lpp ? -1.f : 0.f);
                if (a.gz[1]) {
                    a.gz[1][iq] = a.gscale * c_p * a.beta * zp;
                    a.gzlp[1][iq] = a.gscale * (c_p * a.beta - al * sgn);
                }
            } else if (a.gz[1]) {  // REG evaluate stage: the p pass does not enter the loss
                a.gz[1][iq] = 0.f;
                a.gzlp[1][iq] = 0.f;
            }
            if (a.gz[0]) {
                a.gz[0][iq] = a.gscale * c_q * a.beta * zq;
                a.gzlp[0][iq] = a.gscale * (c_q * a.beta + al * sgn);
            }
        }
#pragma unroll
        for (int c = 0; c < 7; ++c) acc[c] = flow_wave_sum(acc[c]);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 7; ++c) sh[wv][c] = acc[c];
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        double s = 0.0;
        for (int w = 0; w < FLOW_WAVES; ++w) s += (double)sh[w][threadIdx.x];
        a.part[(long)blockIdx.x * 8 + threadIdx.x] = s;
    }
