// Launch 3 of the MIWAE loss (vpc_miw.hip): the BODY of miw_grad_kernel and of its ensemble form miw_grad_multi_kernel,
// included as text so that the stand-alone kernel compiles to the instructions it had with these lines spelled out in it.  In
// scope: `a` (the MiwLossArgs of the launch: the kernel argument, or the base record of the ensemble launch - member 0's) and the
// macros MIW_AT(pointer, field) = that array of this workgroup's member (the pointer itself stand-alone; + mo.field in the
// ensemble form), MIW_OUT(pointer, k) = the member's k-element slot of a result array, MIW_ALPHA = the member's alpha.
// (No include guard: a code fragment, included once per kernel.)
    const int B = a.B, S = a.S, d = a.d, L = a.L;
    const long N = (long)B * S;
    if ((int)blockIdx.x < nblk_elem) {
        const long t = (long)blockIdx.x * 256 + threadIdx.x;
        if (t >= a.P * N * d) return;
        const int p = (int)(t / (N * d));
        const long rem = t - p * N * d;
        const long r = rem / d;
        const int k = (int)(rem - r * d);
        const int b = (int)(r / S);
        const float mq = MIW_AT(a.m, m)[(long)b * d + k];
        const float mv = p == 0 ? mq : MIW_AT(a.mp, mp)[(long)b * d + k];
        float g = MIW_AT(a.gpo[p], scr)[r] * mv;
        if (p == 0 && a.P == 2) g -= MIW_ALPHA / (float)N * mq * (1.f - MIW_AT(a.mp, mp)[(long)b * d + k]);  // - alpha * reg_like
        const MiwHead h = miw_head(MIW_AT(a.y[p], y) + r * a.ldy, d, k, a.raw);
        const float x = MIW_AT(a.x, x)[(long)b * d + k];
        const float y = (x - h.mu) / h.sc;
        const float tt = y * y / h.v, u = 1.f + tt;
        float gmu = g * (h.v + 1.f) * y / (h.v * h.sc * u);
        float gsc = g * (-1.f / h.sc + (h.v + 1.f) * tt / (h.sc * u));
        float gv = g * (miw_half_digamma_diff(h.v) - 0.5f / h.v - 0.5f * log1pf(tt) + (h.v + 1.f) * tt / (2.f * h.v * u));
        if (a.raw) {
            gmu *= miw_sigmoid_d(h.a0);
            gsc *= miw_softplus_d(h.a1);
            gv *= miw_softplus_d(h.a2);
        }
        float* go = MIW_AT(a.gy[p], y) + r * a.ldg;
        go[k] = gmu;
        go[d + k] = gsc;
        go[2 * d + k] = gv;
        return;
    }
    if ((int)blockIdx.x < nblk_elem + nblk_head) {
        const long t = (long)(blockIdx.x - nblk_elem) * 256 + threadIdx.x;
        if (t >= (long)a.P * B * L) return;
        const int p = (int)(t / ((long)B * L));
        const long rem = t - (long)p * B * L;
        const int b = (int)(rem / L), l = (int)(rem - (long)b * L);
        const float* hh = MIW_AT(a.h[p], h) + (long)b * 2 * L;
        const float mu = hh[l], sc = hh[L + l];
        float gm = 0.f, gs = 0.f;
        for (int s = 0; s < S; ++s) {  // d(logpz - logq)/d mean = -z2, d/d scale = -z2 e + 1/scale
            const long r = (long)b * S + s;
            const float e = MIW_AT(a.e[p], e)[r * L + l];
            const float z = mu + sc * e;
            const float w = MIW_AT(a.gw[p], scr)[r];
            gm -= w * z;
            gs += w * (1.f / sc - z * e);
        }
        if (a.P == 2) {  // + alpha * d KL_reg, KL_reg = mean over [B, S, L] (each (b, l) S times)
            const float* hq = MIW_AT(a.h[0], h) + (long)b * 2 * L;
            const float* hp = MIW_AT(a.h[1], h) + (long)b * 2 * L;
            const float mq = hq[l], sq = hq[L + l], mp = hp[l], sp = hp[L + l];
            const float c = MIW_ALPHA / ((float)B * L);
            const float dm = mq - mp, isp2 = 1.f / (sp * sp);
            if (p == 0) {
                gm += c * dm * isp2;
                gs += c * (sq * isp2 - 1.f / sq);
            } else {
                gm -= c * dm * isp2;
                gs += c * (1.f / sp - (sq * sq + dm * dm) * isp2 / sp);
            }
        }
        float* go = MIW_AT(a.gh[p], h) + (long)b * 2 * L;
        go[l] = gm;
        go[L + l] = gs;
        return;
    }
    // the last workgroup: loss partials of the slot launch, summed in block order
    __shared__ double tot[5];
    if (threadIdx.x < 5) {
        double t = 0.0;
        for (int i = 0; i < a.nslot_blocks; ++i) t += MIW_AT(a.part, part)[(long)i * 8 + threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double nb_q = -tot[0] / B;
        const double nb_p = a.P == 2 ? -tot[1] / B : 0.0;
        const double reg_like = tot[2] / (double)N;
        const double kl = tot[3] / ((double)B * L);
        const double al = MIW_ALPHA;
        const double loss = a.P == 2 ? nb_q + al * (kl - nb_q + nb_p - reg_like) : nb_q;  // VAE.py:3250-3251
        double* o = MIW_OUT(a.out8, 8);
        o[0] = loss; o[1] = nb_q; o[2] = nb_p; o[3] = kl; o[4] = reg_like;
        o[5] = tot[4] / ((double)B * 5000.0);  // VAE.py:3099: logpxobsgivenz_imp.sum() / (B * 5000), a literal
        o[6] = tot[0]; o[7] = tot[1];
        if (a.loss_f32) MIW_OUT(a.loss_f32, 1)[0] = (float)loss;
        if (a.accum) MIW_OUT(a.accum, 1)[0] += (float)loss;
    }
