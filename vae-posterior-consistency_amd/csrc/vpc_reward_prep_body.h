// The BODY of the reward's prep kernels (vpc_reward.hip), included as text into
//   reward_prep_kernel<KIND, WIDE>   (the kernel's own arguments) and
//   reward_prep_multi_kernel         (member g's operands, built in registers under the same names; KIND = RK_DENSE, WIDE = false)
//   and reward_prep_multi_kind_kernel<KIND> (the same for RK_DENSE_MASK / RK_POINTNET members, WIDE = true),
// so that both run ONE piece of code and the single-model kernel compiles to the instructions it had as a self-contained kernel (a
// shared inline function is simplified before it is inlined and schedules differently: vpc_small_body.h).
// In scope at the point of inclusion: KIND, WIDE, x, mask, im, W1, b1, AC, pre, W1T, cand, R, n, d, M, Mp, K.
// (No include guard: this is a code fragment, included once per kernel.)
    if (blockIdx.x == 0 && threadIdx.x == 0) cand[(long)n * d] = 0;  // work counter of reward_chain_kernel<1>
    const int f = threadIdx.x;  // 0..127: hidden unit (100 = constant, 101..111 = padding), >= 112 idle
    const int pf = f < H1P ? pos1_full(f) : 0;
    const int din = KIND == RK_DENSE_MASK ? 2 * d : d;  // row pitch of a dense W1
    if (blockIdx.x >= (unsigned)n) {
        if constexpr (KIND == RK_POINTNET) {
            // one block: the A fragments of W1 [100][K] for the update MFMAs of reward_chain_kernel,
            //   W1T[((g * 7 + t) * 64 + lane) * 4 + j] = W1[unit at position 16 t + (lane & 15)][16 g + 4 j + (lane >> 4)]
            // (zero for padding units, the constant unit and k >= K)
            if (f < H1P) {
                const int t = pf >> 4, mr = pf & 15;
                for (int k = 0; k < PN_MAX_K; ++k) {
                    const int s = k >> 2, g = s >> 2, j = s & 3, ln = mr + 16 * (k & 3);
                    W1T[((g * H1T + t) * 64 + ln) * 4 + j] = (f < H1 && k < K) ? W1[f * K + k] : 0.f;
                }
            }
        } else {  // trailing blocks: W1T[u][f] = W1[f][u] (and W1T[d + u][f] = W1[f][d + u]), 8 input columns per block
            const int u0 = 8 * ((int)blockIdx.x - n);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int u = u0 + k;
                if (u < d && f < H1P) {
                    W1T[u * H1P + pf] = f < H1 ? W1[f * din + u] : 0.f;
                    if (KIND == RK_DENSE_MASK) W1T[(d + u) * H1P + pf] = f < H1 ? W1[f * din + d + u] : 0.f;
                }
            }
        }
        return;
    }
    const int r = blockIdx.x, T = d - 1;
    // the row's candidates: cand[r][0] = their number, cand[r][1 + k] = the k-th feature u < d - 1 that is not observed yet, in
    // ascending order; observed features get the reference's R = -1e4 here (evaluate.py:424-433)
    if constexpr (!WIDE) {
        __shared__ int cnt0;
        const int u = threadIdx.x;
        const bool isc = u < T && !mask[(long)r * d + u];
        const unsigned long long bal = __ballot(isc);
        if (threadIdx.x == 0) cnt0 = __popcll(bal);
        __syncthreads();
        const int before = __popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull)) + (threadIdx.x >= 64 ? cnt0 : 0);
        int* cr = cand + (long)r * d;
        if (isc) cr[1 + before] = u;
        if (u < T && !isc) R[(long)r * T + u] = -1e4f;
        if (threadIdx.x == 127) cr[0] = before + (isc ? 1 : 0);
        __syncthreads();
    } else {  // the same ballot over 128-feature chunks, `run` candidates before the chunk
        __shared__ int cnt0, tot;
        int* cr = cand + (long)r * d;
        int run = 0;
        for (int c0 = 0; c0 < T; c0 += 128) {
            const int u = c0 + threadIdx.x;
            const bool isc = u < T && !mask[(long)r * d + u];
            const unsigned long long bal = __ballot(isc);
            if (threadIdx.x == 0) cnt0 = __popcll(bal);
            __syncthreads();
            const int before = run + __popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull)) + (threadIdx.x >= 64 ? cnt0 : 0);
            if (isc) cr[1 + before] = u;
            if (u < T && !isc) R[(long)r * T + u] = -1e4f;
            if (threadIdx.x == 127) tot = before + (isc ? 1 : 0);
            __syncthreads();
            run = tot;
        }
        if (threadIdx.x == 0) cr[0] = run;
    }
    if constexpr (KIND == RK_POINTNET) {
        // agg_X[k] = sum_{j < T} mask_j relu(x_j A[k][j] + C[k][j]): each wave takes every second k, lanes over j
        __shared__ float aggx[PN_MAX_K], aT[PN_MAX_K], cT[PN_MAX_K], agg[2][PN_MAX_K];
        {
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
            for (int k = wv; k < K; k += 2) {
                const float* A = AC + (long)k * d;
                const float* Cc = AC + (long)(K + k) * d;
                float s = 0.f;
                for (int j = lane; j < T; j += 64)
                    if (mask[(long)r * d + j]) s += fmaxf(fmaf(x[(long)r * d + j], A[j], Cc[j]), 0.f);
                s = wave_sum_dpp(s);
                if (lane == 0) {
                    aggx[k] = s;
                    aT[k] = A[T];
                    cT[k] = Cc[T];
                }
            }
        }
        float w[PN_MAX_K];
#pragma unroll
        for (int k = 0; k < PN_MAX_K; ++k) w[k] = (f < H1 && k < K) ? W1[f * K + k] : 0.f;
        const float bias = f < H1 ? b1[f] : 0.f;
        const float xT = x[(long)r * d + T], mT = mask[(long)r * d + T] ? 1.f : 0.f;
        __syncthreads();
        for (int m = 0; m < Mp; ++m) {
            if (m < M) {  // (uniform)
                if (f < K) {
                    const float carry = m == 0 ? xT : im[((long)(m - 1) * n + r) * d + T];
                    const float imT = im[((long)m * n + r) * d + T];
                    agg[0][f] = aggx[f] + mT * fmaxf(fmaf(carry, aT[f], cT[f]), 0.f);
                    agg[1][f] = aggx[f] + fmaxf(fmaf(imT, aT[f], cT[f]), 0.f);
                }
                __syncthreads();
            }
            float p1 = 0.f, p2 = 0.f;
            if (m < M && f < H1) {
                p1 = p2 = bias;
#pragma unroll
                for (int k = 0; k < PN_MAX_K; ++k)
                    if (k < K) {
                        p1 = fmaf(w[k], agg[0][k], p1);
                        p2 = fmaf(w[k], agg[1][k], p2);
                    }
            }
            if (f == H1) p1 = p2 = 1.f;
            if (f < H1P) {
                float* o = pre + (((long)r * Mp + m) * 2) * H1P;
                o[pf] = p1;
                o[H1P + pf] = p2;
            }
            if (m < M) __syncthreads();  // agg is rewritten by the next sample
        }
        return;
    } else {
        // base[f] = b1[f] + sum_i W1[f][i] in[r][i], in = x * mask (| mask): each wave takes every second unit, lanes over i (the
        // rows of W1 are read coalesced; one thread per unit walked its row with a stride of d floats: 128 dependent loads,
        // 35 us for this launch)
        __shared__ float base_sh[H1P];
        {
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
            for (int i0 = 0; i0 < (WIDE ? din : 1); i0 += 128) {
                float xm[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int i = i0 + lane + 64 * k;
                    if (KIND == RK_DENSE_MASK && i >= d)
                        xm[k] = i < din ? (mask[(long)r * d + i - d] ? 1.f : 0.f) : 0.f;
                    else
                        xm[k] = i < d ? x[(long)r * d + i] * (mask[(long)r * d + i] ? 1.f : 0.f) : 0.f;
                }
                for (int u = wv; u < H1; u += 2) {
                    float sacc = 0.f;
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int i = i0 + lane + 64 * k;
                        if (i < din) sacc += W1[u * din + i] * xm[k];
                    }
                    sacc = wave_sum_dpp(sacc);
                    if (lane == 0) base_sh[u] = (i0 == 0 ? b1[u] : base_sh[u]) + sacc;
                }
            }
        }
        __syncthreads();
        if (f >= H1P) return;
        float base = 0.f, wT = 0.f, wTm = 0.f;
        if (f < H1) {
            base = base_sh[f];
            wT = W1[f * din + T];
            if (KIND == RK_DENSE_MASK) wTm = W1[f * din + d + T];
        }
        const float xT = x[(long)r * d + T], mT = mask[(long)r * d + T] ? 1.f : 0.f;
        for (int m = 0; m < Mp; ++m) {
            float p1 = 0.f, p2 = 0.f;
            if (m < M) {
                const float carry = m == 0 ? xT : im[((long)(m - 1) * n + r) * d + T];
                p1 = base + wT * mT * (carry - xT);
                p2 = base + wT * (im[((long)m * n + r) * d + T] - xT * mT);
                if (KIND == RK_DENSE_MASK) p2 += wTm * (1.f - mT);
            }
            if (f == H1) p1 = p2 = 1.f;
            if (f > H1) p1 = p2 = 0.f;
            float* o = pre + (((long)r * Mp + m) * 2) * H1P;
            o[pf] = p1;
            o[H1P + pf] = p2;
        }
    }
