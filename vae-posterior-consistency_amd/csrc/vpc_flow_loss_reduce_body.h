// The body of flow_loss_reduce_kernel and flow_loss_reduce_multi_kernel (vpc_flow.hip), included as text so that both kernels are one piece of code and
// the stand-alone kernel compiles to the instructions it had with these lines spelled out in it.  blockIdx.x is the workgroup's
// index among ONE member's workgroups in both.  In scope at the point of inclusion: `a` (FlowLossArgs: this member's partials, outputs and coefficients).
// (No include guard: a code fragment.)
    __shared__ double sh[8][33];
    const int c = threadIdx.x >> 5, l = threadIdx.x & 31;
    double s = 0.0;
    if (c < 7)
        for (int i = l; i < a.nblk; i += 32) s += a.part[(long)i * 8 + c];
    sh[c][l] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[7];
        for (int k = 0; k < 7; ++k) {
            double u = 0.0;
            for (int j = 0; j < 32; ++j) u += sh[k][j];
            t[k] = u;
        }
        const double al = a.alpha, be = a.beta;
        const double loss_q = t[0] + be * t[2];
        double loss = loss_q;
        if (a.P == 2 && !a.eval) loss = loss_q + al * (t[4] - loss_q + (t[1] + be * t[3]) + t[5]);
        double* o = a.out8;
        o[0] = loss;   // unscaled; train_loss = loss / B
        o[1] = t[0];   // RE_q (VAEFlow: RE_)
        o[2] = t[1];   // RE_p
        o[3] = t[2];   // KL_q
        o[4] = t[3];   // KL_p
        o[5] = t[4];   // KL_reg
        o[6] = t[5];   // NLL of x * mask * ~mask_p
        o[7] = t[6];   // RE_q_imputed (NLL on ~mask)
        const float tl = (float)(loss / a.B);
        if (a.loss_f32) a.loss_f32[0] = tl;
        if (a.accum) a.accum[0] += tl;
    }
