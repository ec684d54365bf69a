// Launch 2 of the MIWAE loss (vpc_miw.hip): the BODY of miw_slots_kernel and of its ensemble form miw_slots_multi_kernel,
// included as text so that the stand-alone kernel compiles to the instructions it had with these lines spelled out in it.  In
// scope: `a` (the MiwLossArgs of the launch: the kernel argument, or the base record of the ensemble launch - member 0's) and the
// macros MIW_AT(pointer, field) = that array of this workgroup's member (the pointer itself stand-alone; + mo.field in the
// ensemble form), MIW_OUT(pointer, k) = the member's k-element slot of a result array, MIW_ALPHA = the member's alpha.
// (No include guard: a code fragment, included once per kernel.)
    __shared__ double sh[MIW_WAVES][5];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = blockIdx.x * MIW_WAVES + wv;
    const int B = a.B, S = a.S;
    float lse[2] = {0.f, 0.f}, srl = 0.f, skl = 0.f, slm = 0.f;
    if (j < B) {
        for (int p = 0; p < a.P; ++p) {
            float mx = -INFINITY;
            for (int i = lane; i < S; i += 64)
                mx = fmaxf(mx, MIW_AT(a.lpo[p], scr)[miw_lpo_row(a.pairing, i, j, B, S)] + MIW_AT(a.lw[p], scr)[(long)j * S + i]);
            mx = miw_wave_max(mx);
            float se = 0.f;
            for (int i = lane; i < S; i += 64)
                se += expf(MIW_AT(a.lpo[p], scr)[miw_lpo_row(a.pairing, i, j, B, S)] + MIW_AT(a.lw[p], scr)[(long)j * S + i] - mx);
            se = miw_wave_sum(se);
            lse[p] = mx + logf(se);
            // gradient seed of the slot: d loss / d a[i, j] = coef * softmax_i
            const float coef = a.P == 2 ? (p == 0 ? -(1.f - MIW_ALPHA) : -MIW_ALPHA) / B : -1.f / B;
            if (a.gy[0]) {
                for (int i = lane; i < S; i += 64) {
                    const long ro = miw_lpo_row(a.pairing, i, j, B, S), rw = (long)j * S + i;
                    const float w = expf(MIW_AT(a.lpo[p], scr)[ro] + MIW_AT(a.lw[p], scr)[rw] - lse[p]);
                    MIW_AT(a.gpo[p], scr)[ro] = coef * w;
                    MIW_AT(a.gw[p], scr)[rw] = coef * w;
                }
            }
        }
        // llh_eval: the q-pass weights of slot j applied to the un-mixed x_mean[j, i, :] (VAE.py:3096-3098 / :3267-3269)
        if (a.xm_imp) {
            for (int k = lane; k < a.d; k += 64) {
                float acc = 0.f;
                for (int i = 0; i < S; ++i) {
                    const long rw = (long)j * S + i;
                    const float w = expf(MIW_AT(a.lpo[0], scr)[miw_lpo_row(a.pairing, i, j, B, S)] + MIW_AT(a.lw[0], scr)[rw] - lse[0]);
                    const float* y = MIW_AT(a.y[0], y) + rw * a.ldy;
                    acc += w * (a.raw ? miw_sigmoid(y[k]) : y[k]);
                }
                a.xm_imp[(long)j * a.d + k] = acc;
            }
        }
        // per-row sums of the same workgroup's rows (rows j*S .. j*S + S - 1)
        for (int s = lane; s < S; s += 64) {
            slm += MIW_AT(a.lpm, scr)[(long)j * S + s];
            if (a.P == 2) srl += MIW_AT(a.rl, scr)[(long)j * S + s];
        }
        slm = miw_wave_sum(slm);
        srl = miw_wave_sum(srl);
        if (a.P == 2) skl = MIW_AT(a.kl, scr)[j];
    }
    if (lane == 0) {
        sh[wv][0] = lse[0]; sh[wv][1] = lse[1]; sh[wv][2] = srl; sh[wv][3] = skl; sh[wv][4] = slm;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        double t = 0.0;
        for (int w = 0; w < MIW_WAVES; ++w) t += sh[w][threadIdx.x];
        MIW_AT(a.part, part)[(long)blockIdx.x * 8 + threadIdx.x] = t;
    }
