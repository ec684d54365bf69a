// Launch 1 of the MIWAE loss (vpc_miw.hip): the BODY of miw_rows_kernel and of its ensemble form miw_rows_multi_kernel,
// included as text so that the stand-alone kernel compiles to the instructions it had with these lines spelled out in it.  In
// scope: `a` (the MiwLossArgs of the launch: the kernel argument, or the base record of the ensemble launch - member 0's) and the
// macros MIW_AT(pointer, field) = that array of this workgroup's member (the pointer itself stand-alone; + mo.field in the
// ensemble form), MIW_OUT(pointer, k) = the member's k-element slot of a result array, MIW_ALPHA = the member's alpha.
// (No include guard: a code fragment, included once per kernel.)
    const int lane = threadIdx.x & 63;
    const long N = (long)a.B * a.S;
    const long gw = (long)blockIdx.x * MIW_WAVES + (threadIdx.x >> 6);
    if (gw >= a.P * N) return;
    const int p = (int)(gw / N);
    const long r = gw - p * N;
    const int b = (int)(r / a.S), s = (int)(r - (long)b * a.S);
    const int d = a.d, L = a.L;
    const float* x = MIW_AT(a.x, x) + (long)b * d;
    const float* mq = MIW_AT(a.m, m) + (long)b * d;
    const float* mpp = a.mp ? MIW_AT(a.mp, mp) + (long)b * d : nullptr;
    const float* mrow = p == 0 ? mq : mpp;
    const float* y = MIW_AT(a.y[p], y) + r * a.ldy;
    float so = 0.f, sm = 0.f, sr = 0.f;
    for (int k = lane; k < d; k += 64) {
        const MiwHead h = miw_head(y, d, k, a.raw);
        const float lp = miw_student_lp(x[k], h);
        so += lp * mrow[k];
        if (p == 0) {
            sm += lp * (1.f - mq[k]);
            if (mpp) sr += lp * mq[k] * (1.f - mpp[k]);
        }
    }
    // logpz - logq of the fresh draw z2 = mean + scale * e (VAE.py:3087-3091 / :3216-3220, :3237-3240)
    const float* hh = MIW_AT(a.h[p], h) + (long)b * 2 * L;
    const float* e = MIW_AT(a.e[p], e) + r * L;
    float slw = 0.f;
    for (int l = lane; l < L; l += 64) {
        const float mu = hh[l], sc = hh[L + l];
        const float z = mu + sc * e[l];
        const float dz = z - mu;
        const float lpz = -0.5f * z * z - MIW_HALF_LOG_2PI;
        const float lq = -(dz * dz) / (2.f * sc * sc) - logf(sc) - MIW_HALF_LOG_2PI;
        slw += lpz - lq;
    }
    so = miw_wave_sum(so);
    slw = miw_wave_sum(slw);
    if (p == 0) {
        sm = miw_wave_sum(sm);
        sr = miw_wave_sum(sr);
    }
    float skl = 0.f;
    const bool do_kl = p == 0 && a.P == 2 && s == 0;
    if (do_kl) {  // KL(N(mean_q, scale_q) || N(mean_p, scale_p)) summed over l (VAE.py:3249, :3253-3258)
        const float* hp = MIW_AT(a.h[1], h) + (long)b * 2 * L;
        for (int l = lane; l < L; l += 64) {
            const float r1 = hh[L + l] / hp[L + l];
            const float vr = r1 * r1;
            const float t1 = (hh[l] - hp[l]) / hp[L + l];
            skl += 0.5f * (vr + t1 * t1 - 1.f - logf(vr));
        }
        skl = miw_wave_sum(skl);
    }
    if (lane == 0) {
        MIW_AT(a.lpo[p], scr)[r] = so;
        MIW_AT(a.lw[p], scr)[r] = slw;
        if (p == 0) {
            MIW_AT(a.lpm, scr)[r] = sm;
            if (a.P == 2) MIW_AT(a.rl, scr)[r] = sr;
        }
        if (do_kl) MIW_AT(a.kl, scr)[b] = skl;
    }
