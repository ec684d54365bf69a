// The BODY of the reward's chain kernels (vpc_reward.hip), included as text into
//   reward_chain_kernel<KIND, MODE>     (a = the RewardArgs kernel argument) and
//   reward_chain_multi_kernel<MODE>     (a = member blockIdx.y's RewardArgs, built in registers; KIND = RK_DENSE) and
//   reward_chain_multi_kind_kernel<FKIND, MODE>  (the same for RK_DENSE_MASK / RK_POINTNET members; KIND = FKIND in MODE 1),
// so that a member's items run the arithmetic and the in-wave summation order of the single-model kernel, and that kernel compiles
// to the instructions it had as a self-contained kernel (vpc_small_body.h says why this is not a shared inline function).
// Items are handed out over blockIdx.x / gridDim.x and a.next_item: per member under the member kernels.
// In scope at the point of inclusion: KIND, MODE, `a`.  (No include guard: a code fragment, included once per kernel.)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    load_image(lds, a.w23, W23_FLOATS);
    const float* W2 = lds;
    const float* W3 = lds + H2P * 128;
    const float* W1F = lds + W23_FLOATS;  // POINTNET: the W1 fragments of the groups g < ceil(K / 16)
    if (KIND == RK_POINTNET) load_image(lds + W23_FLOATS, a.W1T, (a.K + 15) / 16 * PN_FRAG);
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int nch = (a.d - 1 + RW_CH - 1) / RW_CH;  // chunks per row (upper bound)
    const long nitems = MODE == 0 ? a.n : (long)a.n * nch;
    const float invM = 1.f / (float)a.M;

    long item = (long)blockIdx.x * RW_WAVES + w;
    auto next = [&]() {
        if (MODE == 0) { item += (long)gridDim.x * RW_WAVES; return; }
        int v = 0;
        if (lane == 0) v = atomicAdd(a.next_item, 1);
        item = (long)gridDim.x * RW_WAVES + __builtin_amdgcn_readfirstlane(v);  // (the first round is the launch's own grid)
    };
    for (; item < nitems; next()) {
        const int r = MODE == 0 ? (int)item : (int)(item / nch);
        const int ch = MODE == 0 ? 0 : (int)(item % nch);
        int ncand = 0;
        const int* cl = a.cand + (long)r * a.d + 1 + RW_CH * ch;
        if (MODE == 1) {
            ncand = a.cand[(long)r * a.d] - RW_CH * ch;
            if (ncand <= 0) continue;
            if (ncand > RW_CH) ncand = RW_CH;
        }
        const int total = MODE == 0 ? a.Mp : ncand * a.M;  // columns of this item
        float acc[RW_CH];
#pragma unroll
        for (int k = 0; k < RW_CH; ++k) acc[k] = 0.f;
        for (int t0 = 0; t0 < total; t0 += 16) {
            asm volatile("" ::: "memory");
            int cc = c, qq = q;
            launder(cc, qq);
            const int f = t0 + c;
            const bool live = MODE == 0 ? f < a.M : f < total;
            int kk = 0, m = f;
            if (MODE == 1) {
                kk = live ? f / a.M : 0;
                m = live ? f - kk * a.M : 0;
            }
            const int u = MODE == 1 ? cl[kk] : 0;
            const float imu = (MODE == 1 && live) ? a.im[((long)m * a.n + r) * a.d + u] : 0.f;
            const float* pp = a.pre + (((long)r * a.Mp + m) * 2) * H1P + 4 * q;
            f32x4 h1[2][H1T];
            if constexpr (KIND == RK_POINTNET && MODE == 1) {
                // upd = W1 relu(im_u A_u + C_u), shared by both chains: A = W1 fragments (LDS), B = lane (c, q)'s value of
                // k = 16 g + 4 j + q for its column's candidate
                f32x4 upd[H1T];
#pragma unroll
                for (int t = 0; t < H1T; ++t) upd[t] = zero4();
                const float* Au = a.AC + u;
                const float* Cu = a.AC + (long)a.K * a.d + u;
#pragma unroll
                for (int g = 0; g < PN_MAX_K / 16; ++g) {
                    if (16 * g >= a.K) break;  // (uniform)
                    float bv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = 16 * g + 4 * j + q;
                        bv[j] = k < a.K ? fmaxf(fmaf(imu, Au[(long)k * a.d], Cu[(long)k * a.d]), 0.f) : 0.f;
                    }
                    f32x4 af[H1T];
#pragma unroll
                    for (int t = 0; t < H1T; ++t) af[t] = *reinterpret_cast<const f32x4*>(W1F + ((g * H1T + t) * 64 + lane) * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (16 * g + 4 * j < a.K)  // (uniform) k-steps past K multiply zeros
#pragma unroll
                            for (int t = 0; t < H1T; ++t) upd[t] = VPC_MFMA(af[t][j], bv[j], upd[t]);
                }
#pragma unroll
                for (int chn = 0; chn < 2; ++chn)
#pragma unroll
                    for (int t = 0; t < H1T; ++t)
                        h1[chn][t] = relu4(*reinterpret_cast<const f32x4*>(pp + chn * H1P + 16 * t) + upd[t]);
            } else {
#pragma unroll
                for (int chn = 0; chn < 2; ++chn)
#pragma unroll
                    for (int t = 0; t < H1T; ++t) {
                        f32x4 v = *reinterpret_cast<const f32x4*>(pp + chn * H1P + 16 * t);
                        if (MODE == 1) v += *reinterpret_cast<const f32x4*>(a.W1T + (long)u * H1P + 16 * t + 4 * q) * imu;
                        if (MODE == 1 && KIND == RK_DENSE_MASK)  // revealing u also sets its mask input to 1
                            v += *reinterpret_cast<const f32x4*>(a.W1T + ((long)a.d + u) * H1P + 16 * t + 4 * q);
                        h1[chn][t] = relu4(v);
                    }
            }
            f32x4 h2[2][H2T];
#pragma unroll
            for (int t = 0; t < H2T; ++t) {
                f32x4 o[2] = {zero4(), zero4()};
                tile_fwd_nb<H1T, 128, 2, NK1>(W2, t, h1, o, cc, qq);
                h2[0][t] = relu4(o[0]);
                h2[1][t] = relu4(o[1]);
            }
            f32x4 mu[2] = {zero4(), zero4()}, lv[2] = {zero4(), zero4()};
            tile_fwd_nb<H2T, 64, 2, NK2>(W3, 0, h2, mu, cc, qq);
            tile_fwd_nb<H2T, 64, 2, NK2>(W3, 1, h2, lv, cc, qq);
            float* st = a.stat + ((long)r * a.Mp + m) * STAT + 4 * q;
            if (MODE == 0) {
                *reinterpret_cast<f32x4*>(st) = mu[0];
                *reinterpret_cast<f32x4*>(st + 16) = lv[0];
                *reinterpret_cast<f32x4*>(st + 32) = mu[1];
                *reinterpret_cast<f32x4*>(st + 48) = lv[1];
            } else {
                float val = 0.f;
#pragma unroll
                for (int chn = 0; chn < 2; ++chn) {
                    const f32x4 ma = *reinterpret_cast<const f32x4*>(st + 32 * chn);
                    const f32x4 la = *reinterpret_cast<const f32x4*>(st + 32 * chn + 16);
                    float kl = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float dm = mu[chn][j] - ma[j];
                        const float t = dm * dm * expf(-0.5f * la[j]) + expf(lv[chn][j] - la[j]) - 1.f - lv[chn][j] + la[j];
                        kl += (4 * q + j < a.L) ? t : 0.f;
                    }
                    kl = live ? 0.5f * kl : 0.f;
                    val += chn == 0 ? kl : -kl;
                }
#pragma unroll
                for (int k = 0; k < RW_CH; ++k) acc[k] += kk == k ? val : 0.f;
            }
        }
        if (MODE == 1) {
#pragma unroll
            for (int k = 0; k < RW_CH; ++k) {
                const float sacc = wave_sum(acc[k]);
                if (lane == 0 && k < ncand) a.R[(long)r * (a.d - 1) + cl[k]] = sacc * invM;
            }
        }
    }
