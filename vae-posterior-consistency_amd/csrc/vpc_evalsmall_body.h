// The evaluate-stage forward of ONE (member, 16-row tile): the BODY of the kernels of vpc_evalsmall.hip, included as text into
//   eval_small_kernel<DT>            (OUT = OUT_SUMS: the five sums of the tile's record),
//   eval_small_aug_kernel<DTI, DT>   (the same for Reg_VAE_mask / vanilla_VAE_mask members: AUG),
//   eval_small_eddi_kernel<DTI, DT>  (the same for Reg_EDDI / vanilla_EDDI members: PN) and
//   impute_small_kernel<DT, MODE>    (OUT = OUT_XHAT / OUT_SQERR: x_hat, or the target column's squared error, per draw row) with
//   impute_small_aug_kernel<DTI, DT, MODE> and impute_small_eddi_kernel<DTI, DT, MODE> (the same outputs under AUG / PN: the input
//   stage ends at E_X and the output stage starts at the last layer's `pre`, so the two choices meet nowhere),
// so that the arithmetic up to x_hat is ONE piece of code and eval_small_kernel compiles to the instructions it had as a
// self-contained kernel (vpc_small_body.h says why this is not a shared inline function).
// In scope at the point of inclusion: the compile-time tile counts DT (tiles of d: x / mask words, W6, the output tiles) and DTI
// (tiles of the encoder INPUT: W1's k-tiles, the X buffer) and the flags AUG and PN - the parameters of the training twin
// vpc_small_body.h -, `constexpr int OUT`, `a` (EvalArgs), `pnx` (an EvalPointNet: the point-net kernel's own arguments, an empty
// record elsewhere), and for OUT != OUT_SUMS `out` / `sout` (member 0's output and the member stride in floats).  Plain members:
// DTI == DT, AUG and PN false.  AUG (src/models/VAE.py:545-548, 1031-1033): the encoder input is [x*mask | mask] of width
// 2 a.d_real; PN (VAE.py:719-733, 903-917): it is the point-net aggregate [16][pnx.K] of the folded front-end (DTI = dt_for(K)).
// Under both a.d is the row pitch of x and the mask, a.d_real obs_dim.  (No include guard: a code fragment, included once per
// kernel.)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    auto buf = [&](int b) { return lds + b * SBUF; };
    float* red = lds + E_COUNT * SBUF;
    constexpr int S1 = s_for_tiles(DTI);
    const EncImg ei(DTI);
    const DecImg di(DT);
    const unsigned mem = blockIdx.y;
    const long tile_id = a.tile0 + blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    double* rec = a.part + mem * a.spart + tile_id * EVAL_TERMS;
    // (uniform addresses: scalar loads)
    const long long* te = a.tiles + 4 * tile_id;
    const long xrow0 = te[0], nvl = te[1], erow0 = te[2];
    // a tile entry that points outside the arrays reads nothing: its record is zero (the host builds the table; this is the fence)
    if (xrow0 < 0 || nvl < 1 || nvl > 16 || xrow0 + nvl > a.N || erow0 < 0 || erow0 + nvl > a.R) {
        if (OUT == OUT_SUMS && threadIdx.x < EVAL_TERMS) rec[threadIdx.x] = 0.0;
        return;
    }
    const int nv = (int)nvl;
    const float* xg = a.x + mem * a.sx;
    const uint8_t* mg = a.mask + mem * a.sm;
    const float* enc_img = a.enc_img + mem * a.simg;
    const float* dec_img = a.dec_img + mem * a.simg;
    // (re-derived from opaque base pointers per phase, as the tile body does: keeps the fragment loads of all layers from being
    // hoisted to the top of the kernel)
    const float *W1, *b1, *W2, *W3, *W4, *W5, *W6;
    auto weights = [&]() {
        const float* e_ = enc_img;
        const float* d_ = dec_img;
        asm volatile("" : "+s"(e_), "+s"(d_)::"memory");
        W1 = e_ + ei.oW1; b1 = e_ + ei.ob1; W2 = e_ + ei.oW2; W3 = e_ + ei.oW3;
        W4 = d_ + di.oW4; W5 = d_ + di.oW5; W6 = d_ + di.oW6;
    };
    const float inv_s2 = expf(-a.x_logvar), half_lv = 0.5f * a.x_logvar;
    const bool ok = c < nv;
    // ---- this wave's column tile of x and of the mask words (range-checked: rows past the tile's valid rows read 0; the last
    // tile's columns past d read column 0 and are cleared)
    const bool colok = 16 * w + 4 * q + 3 < a.d;
    f32x4 xv = zero4();
    uint32_t mw = 0;
    if (w < DT) {
        const int vo = c * a.d + (colok ? 16 * w + 4 * q : 0);
        xv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rows_rsrc(xg, xrow0, xrow0 + nv, a.d), 4 * vo, 0, 0));
        mw = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(mg) + xrow0 * a.d, 0, (uint32_t)(nv * a.d), 0x00020000), vo, 0, 0);
        if (!colok) { mw = 0; xv = zero4(); }
    }
    int cc = c, qq = q;
    launder(cc, qq);
    if constexpr (PN) {
        // ================================================================ point-net front-end as the input stage (the folded form
        // of vpc_small_body.h; VAE.py:719-733, 903-917).  The workspace lies in E_H1 .. E_G2 (6 x SBUF = 13 824 floats, contiguous),
        // idle until the first encoder stage:
        //   PT  [a.d][64]   folded table: PT[64 j + k] = A_j[k], PT[64 j + 32 + k] = C_j[k], zero for k >= K and j >= d_real
        //   PPR [n_front]   member g's front-end parameters in flat order (E [d_real][K] | t [d_real] | W [K][2+K] | c [K]), read
        //                   from its row of the parameter stack
        //   PXS, PMQ [16][a.d]   the tile's x and mask rows as floats; rows past the valid ones and columns past d_real are 0
        // 4 096 + 3 328 + 1 024 + 1 024 = 9 472 floats at the limits d = 64, K = 32.
        float* const PT = buf(E_H1);
        float* const PPR = PT + 4096;
        float* const PXS = PPR + 3328;
        float* const PMQ = PXS + 1024;
        const int K = pnx.K, dr = a.d_real, dp = a.d;
        const int nfront = dr * K + dr + K * (2 + K) + K;
        const float* front = pnx.front + mem * pnx.sP;
        const int tid = threadIdx.x;
        for (int i = tid; i < nfront; i += THREADS) PPR[i] = front[i];
        for (int i = tid; i < 16 * dp; i += THREADS) {
            const int r = i / dp, j = i - r * dp;
            const bool in = r < nv && j < dr;
            const long g = (xrow0 + r) * dp + j;
            PXS[i] = in ? xg[g] : 0.f;
            PMQ[i] = (in && mg[g]) ? 1.f : 0.f;
        }
        __syncthreads();
        // the fold of eddi_fold_kernel: A_j = w_x + W_E E_j, C_j = w_t t_j + c  (W = [w_x | W_E | w_t], VAE.py:719-727)
        const float *pE = PPR, *ptb = pE + dr * K, *pW = ptb + dr, *pc = pW + K * (2 + K);
        for (int i = tid; i < 32 * dp; i += THREADS) {
            const int k = i & 31, j = i >> 5;
            float A = 0.f, C = 0.f;
            if (k < K && j < dr) {
                const float* wr = pW + k * (2 + K);
                A = wr[0];
#pragma unroll 4
                for (int e = 0; e < K; ++e) A += wr[1 + e] * pE[j * K + e];
                C = wr[1 + K] * ptb[j] + pc[k];
            }
            PT[64 * j + k] = A;
            PT[64 * j + 32 + k] = C;
        }
        __syncthreads();
        // thread (row r, k) sums m[r][j] relu(x[r][j] A_j[k] + C_j[k]) over the features in a fixed order; columns K .. 16 DTI - 1
        // are written as 0
        const int r = tid >> 5, k = tid & 31;
        float sq = 0.f;
#pragma unroll 4
        for (int j = 0; j < dr; ++j) sq += PMQ[r * dp + j] * fmaxf(PXS[r * dp + j] * PT[64 * j + k] + PT[64 * j + 32 + k], 0.f);
        if (k < 16 * DTI) buf(E_X)[r * SP + k] = k < K ? sq : 0.f;
        // (the first encoder stage reads E_X and writes E_H1 behind its barrier: every read of the workspace is done by then)
    }
    // ================================================================ encoder forward (phase E of the tile body, pass 0)
    {
        weights();
        f32x4 fW1[DTI], fW2[H1T], fW3[H2T], bias1 = zero4();
        if (w < H1T) {
            ldW<DTI, S1>(W1, w, cc, qq, fW1);
            bias1 = *reinterpret_cast<const f32x4*>(b1 + 16 * w + 4 * qq);
        }
        if constexpr (PN) {
            // (E_X holds the aggregate already: the input stage above)
        } else if constexpr (!AUG) {
            if (w < DT) st_act(buf(E_X), w, cc, qq, xv * mask_to_f32(mw));  // x.float() * mask  (VAE.py:388)
        } else {
            // [x*mask | mask | 0] exactly as the step body writes it (VAE.py:545-548): element f < d is x_f m_f, d <= f < 2 d is
            // m_{f-d}, 2 d <= f < 16 DTI is 0.  Column d is in general not 4-aligned, so every element is a dword store of its
            // own; each column of the buffer has exactly one writer.  Rows past the valid ones: xv and the mask word are 0.
            const f32x4 mk = mask_to_f32(mw), xm = xv * mk;
            float* xrow = buf(E_X) + cc * SP;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = 16 * w + 4 * qq + j;
                if (w < DT && f < a.d_real) {
                    xrow[f] = xm[j];
                    xrow[a.d_real + f] = mk[j];
                }
                if (w < DTI && f >= 2 * a.d_real) xrow[f] = 0.f;
            }
        }
        if (w < H2T) ldW<H1T, 128>(W2, w, cc, qq, fW2);
        lds_barrier();
        launder(cc, qq);
        if (w < H1T) {
            f32x4 in[DTI];
#pragma unroll
            for (int t = 0; t < DTI; ++t) in[t] = ld_act(buf(E_X), t, cc, qq);
            st_act(buf(E_H1), w, cc, qq, relu4(mmW<DTI>(fW1, in, bias1)));
        }
        if (w < 2) ldW<H2T, 64>(W3, w, cc, qq, fW3);
        lds_barrier();
        launder(cc, qq);
        if (w < H2T) {
            f32x4 in[H1T];
#pragma unroll
            for (int t = 0; t < H1T; ++t) in[t] = ld_act(buf(E_H1), t, cc, qq);
            st_act(buf(E_H2), w, cc, qq, relu4(mmW<H1T, NK1>(fW2, in, zero4())));
        }
        lds_barrier();
        launder(cc, qq);
        if (w < 2) {  // wave 0: mean tile, wave 1: logvar tile
            f32x4 in[H2T];
#pragma unroll
            for (int t = 0; t < H2T; ++t) in[t] = ld_act(buf(E_H2), t, cc, qq);
            f32x4 o = mmW<H2T, NK2>(fW3, in, zero4());
            if (!ok) o = zero4();  // rows past the valid ones: statistics 0
            st_act(buf(E_ML), w, cc, qq, o);
        }
    }
    lds_barrier();
    launder(cc, qq);
    // ================================================================ decoder forward and the five sums
    float S_A = 0.f, S_I = 0.f, SQ = 0.f, CNT = 0.f, KL = 0.f;
    {
        weights();
        f32x4 fW4[1], fW5[H2T], fW6[H1T];
        if (w < H2T) ldW<1, S4>(W4, w, cc, qq, fW4);
        if (w < H1T) ldW<H2T, 64>(W5, w, cc, qq, fW5);
        if (w == 0) {  // z = mean + eps * exp(logvar / 2); z[L] = 1 drives the bias chain; the row's KL to the standard normal
            const f32x4 mu = ld_act(buf(E_ML), 0, cc, qq), lv = ld_act(buf(E_ML), 1, cc, qq);
            f32x4 e;
            if (a.draw) {
                // group q of draw row r has the counter vpc_fill_normal gives float index 16 r + 4 q of a flat [R x 16] array
                e = eps_normal4((uint64_t)((erow0 + cc) * 4 + qq) + a.offset, a.members[mem].seed);
            } else {
                e = ld_rows(rows_rsrc(a.eps + mem * a.seps, erow0, erow0 + nv, 16), cc, 16, 4 * qq);
            }
            f32x4 z;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool lat = 4 * qq + j < a.L;
                z[j] = mu[j] + ((lat && ok) ? e[j] : 0.f) * __expf(0.5f * lv[j]);
                if (4 * qq + j == a.L) z[j] = 1.f;
                if (lat) KL += 0.5f * (__expf(lv[j]) + mu[j] * mu[j] - 1.f - lv[j]);  // (rows past the valid ones: 0)
            }
            st_act(buf(E_Z), 0, cc, qq, z);
        }
        lds_barrier();
        launder(cc, qq);
        if (w < H2T) {
            const f32x4 in[1] = {ld_act(buf(E_Z), 0, cc, qq)};
            st_act(buf(E_G1), w, cc, qq, relu4(mmW<1>(fW4, in, zero4())));
        }
        if (w < DT) ldW<H1T, 128>(W6, w, cc, qq, fW6);
        lds_barrier();
        launder(cc, qq);
        if (w < H1T) {
            f32x4 in[H2T];
#pragma unroll
            for (int t = 0; t < H2T; ++t) in[t] = ld_act(buf(E_G1), t, cc, qq);
            st_act(buf(E_G2), w, cc, qq, relu4(mmW<H2T, NK2>(fW5, in, zero4())));
        }
        lds_barrier();
        launder(cc, qq);
        if (w < DT) {  // output tile w: x_hat = sigmoid(.), the terms on mask and on its complement
            f32x4 in[H1T];
#pragma unroll
            for (int t = 0; t < H1T; ++t) in[t] = ld_act(buf(E_G2), t, cc, qq);
            const f32x4 pre = mmW<H1T, NK1>(fW6, in, zero4());
            const f32x4 mA = mask_to_f32(mw);
            const float hinv_s2 = 0.5f * inv_s2;
            if constexpr (OUT != OUT_SUMS) {
                // draw row erow0 + c, real rows and real columns only: x_hat [R][d_real], or the target column's squared error [R]
                float* o = out + mem * sout;
                const int T = a.d_real - 1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = 16 * w + 4 * qq + j;
                    const float xh = fast_sigmoid(pre[j]);
                    const float diff = xh - xv[j];
                    if (OUT == OUT_XHAT && ok && col < a.d_real) o[(erow0 + cc) * a.d_real + col] = xh;
                    if (OUT == OUT_SQERR && ok && col == T) o[erow0 + cc] = diff * diff;
                }
                return;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = fast_sigmoid(pre[j]);
                const float diff = xh - xv[j];
                const float t = diff * diff * hinv_s2 + half_lv;
                // the complement counts real rows and REAL columns only: a padding column has a zero mask byte too
                const float mI = (ok && 16 * w + 4 * qq + j < a.d_real) ? 1.f - mA[j] : 0.f;
                S_A += mA[j] * t;
                S_I += mI * t;
                SQ += mI * diff * diff;
                CNT += mI;
            }
        }
    }
    if constexpr (OUT != OUT_SUMS) return;
    // ================================================================ the tile's record
    const float s[EVAL_TERMS] = {S_A, S_I, SQ, CNT, KL};
#pragma unroll
    for (int i = 0; i < EVAL_TERMS; ++i) {
        const float v = wave_sum_dpp(s[i]);
        if (lane == 0) red[w * EVAL_TERMS + i] = v;
    }
    lds_barrier();
    if (threadIdx.x < EVAL_TERMS) {
        double t = 0.0;
        for (int k = 0; k < WAVES; ++k) t += (double)red[k * EVAL_TERMS + threadIdx.x];
        rec[threadIdx.x] = t;
    }
