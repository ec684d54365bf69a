// The step of ONE 16-row tile: the BODY of the small-batch whole-step kernels of vpc_small.hip, included as text into
//   step_small_kernel        (a = the SmallArgs kernel argument, tile_id = blockIdx.x),
//   step_small_aug_kernel    (the same for the mask-augmented classes), step_small_eddi_kernel (the point-net classes) and
//   step_small_multi_kernel, step_small_multi_aug_kernel, step_small_multi_eddi_kernel
//                            (a = member g's arguments built in registers, MemberArgs - the same fields -, tile_id = the
//                             member's tile: vpc_small_member.h),
// so that both run ONE piece of code - a member of an ensemble computes bit for bit what its stand-alone step computes - and
// the single-model kernel compiles to the instructions it had as a self-contained kernel (a shared inline function is
// simplified before it is inlined, without knowing that `a` is the kernel-argument segment, and schedules differently).
// In scope at the point of inclusion: the compile-time tile counts DT (tiles of d: x / mask words of the loss, W6, the output
// tiles, dW6) and DTI (tiles of the encoder INPUT: W1's k-tiles, the X buffers, dW1) and the flags AUG and PN, `a`, `pnx` (a
// SmallPointNet: the point-net kernel's own arguments, an empty record elsewhere), `const unsigned tile_id`; everything
// vpc_small.hip declares before its kernels.  Plain models: DTI == DT, AUG and PN false.  PN (Reg_EDDI / vanilla_EDDI,
// src/models/VAE.py:719-733, 903-917): the encoder input is the point-net aggregate agg [16][pnx.K] of the folded front-end
// (DTI = dt_for(K)), the encoder backward goes on to dagg and the front-end's (dA | dC) block of the tile in pnx.partF; a.d is
// the row pitch of x and the masks, a.d_real obs_dim.  AUG (Reg_VAE_mask /
// vanilla_VAE_mask, src/models/VAE.py:545-548, 1031-1033): the encoder input is [x*mask | mask] of width 2 a.d_real, a.d is
// the row pitch of x and the masks.  Partial blocks and loss terms go to slot tile_id of a.partE / a.partD / a.loss_part.
// (No include guard: this is a code fragment, included once per kernel.)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    auto buf = [&](int b) { return lds + b * SBUF; };
    float* red = lds + B_COUNT * SBUF;
    constexpr int S1 = s_for_tiles(DTI);
    const EncImg ei(DTI);
    const DecImg di(DT);
    // (re-derived from opaque base pointers in every tile / pass: the weights never change during the launch, and hipcc
    // otherwise hoists the global fragment loads of ALL layers out of the loops - 900 bytes of scratch per lane)
    const float *W1, *b1, *W2, *W3, *W4, *W5, *W6;
    auto weights = [&]() {
        const float* e_ = a.enc_img;
        const float* d_ = a.dec_img;
        asm volatile("" : "+s"(e_), "+s"(d_)::"memory");
        W1 = e_ + ei.oW1; b1 = e_ + ei.ob1; W2 = e_ + ei.oW2; W3 = e_ + ei.oW3;
        W4 = d_ + di.oW4; W5 = d_ + di.oW5; W6 = d_ + di.oW6;
    };
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const bool two = a.npass == 2;
    const float inv_s2 = expf(-a.x_logvar), half_lv = 0.5f * a.x_logvar;
    constexpr float HL2PI = 0.91893853320467274f;

    // ONE 16-row tile per workgroup (the host launches one workgroup per tile): the decoder-side gradient accumulators live
    // through the decoder phases of both passes, are written out, and only then the encoder-side ones come to life for the
    // encoder backward of both passes - everything those need (x * mask, h1, h2 and the seeds of both passes) is still in LDS.
    // (All 100 accumulators beside two stages' worth of weight fragments do not fit 256 registers.)
    f32x4 acc6[H1T], acc5[H2T], acc4 = zero4();
#pragma unroll
    for (int t = 0; t < H1T; ++t) acc6[t] = zero4();
#pragma unroll
    for (int t = 0; t < H2T; ++t) acc5[t] = zero4();
    float S_A0 = 0.f, S_E0 = 0.f, S_A1 = 0.f, S_kl0q = 0.f, S_kl0p = 0.f, S_klr = 0.f, S_zll = 0.f;

    if (a.draw) {
        // ---- the step's draws for this tile's rows (same Philox counters and values as vpc_draw_step: vpc_rng.h)
        const long row0 = (long)tile_id * 16;
        const long nrow = a.B - row0 < 16 ? a.B - row0 : 16;
        uint64_t off_m = a.off_mask, off_e = a.off_eps;
        if (a.state) { off_m += (uint64_t)a.state[1]; off_e += (uint64_t)a.state[1]; }
        if (a.mask_in) {  // mask_p bytes [row0 d, (row0 + nrow) d): every 8-byte Philox group that touches them (a group on a
                          // tile boundary is written by both neighbours - the same bytes)
            const long lo = row0 * a.d + (a.mask_elem_lo & 7), hi = (row0 + nrow) * a.d + (a.mask_elem_lo & 7);
            const long g0 = lo / MASK_PER_CALL, g1 = (hi + MASK_PER_CALL - 1) / MASK_PER_CALL;
            for (long g = g0 + threadIdx.x; g < g1; g += THREADS)
                draw_mask_body(a.mask_in, const_cast<uint8_t*>(a.m[1]), a.B * (long)a.d, a.keep_prob, a.seed, off_m, g, a.mask_elem_lo);
        }
        const long plane = a.B * 16, nplanes = a.n_eps / plane;
        for (long i = threadIdx.x; i < nplanes * nrow * 4; i += THREADS) {  // 4 groups of 4 normals per row and plane
            const long pl = i / (nrow * 4), rem = i - pl * nrow * 4;
            fill_normal_body(a.eps_out, a.n_eps, a.seed, off_e, (pl * plane + row0 * 16) / 4 + rem, a.shard);
        }
        __syncthreads();  // (a fence: the stores above are visible to the loads below)
    }
    {
        const int tile = tile_id;
        const long row0 = (long)tile * 16;
        const bool ok = row0 + c < a.B;
        // ---- this wave's column tile of x and of the mask words of both passes (range-checked: rows past B read 0; the last
        // tile's columns past d read column 0 and have their mask words cleared)
        const bool colok = 16 * w + 4 * q + 3 < a.d;
        f32x4 xv = zero4();
        uint32_t mwq = 0, mwp = 0;
        if (w < DT) {
            const int vo = c * a.d + (colok ? 16 * w + 4 * q : 0);
            xv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rows_rsrc(a.x, row0, a.B, a.d), 4 * vo, 0, 0));
            const long rem = (a.B - row0) * (long)a.d;
            const uint32_t rec = rem > 0xffffffffL ? 0xffffffffu : (uint32_t)rem;
            mwq = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
                __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.m[0]) + row0 * a.d, 0, rec, 0x00020000), vo, 0, 0);
            if (two)
                mwp = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
                    __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.m[1]) + row0 * a.d, 0, rec, 0x00020000), vo, 0, 0);
            if (!colok) { mwq = 0; mwp = 0; }
        }
        auto ld_lat = [&](const float* base) -> f32x4 {  // [B][16] padded latent-width array; NULL reads 0
            return ld_rows(rows_rsrc(base ? base : a.x, row0, base ? a.B : row0, 16), c, 16, 4 * q);
        };
        int cc = c, qq = q;
        launder(cc, qq);
        // ---- PN: the point-net front-end's workspace.  Buffers B_Z .. B_DG1 (6 x SBUF = 13 824 floats, contiguous) are idle
        // before the encoder forward and again after the encoder backward; both front-end phases stage into them:
        //   PT  [a.d][64]   folded table: PT[64 j + k] = A_j[k], PT[64 j + 32 + k] = C_j[k], zero for k >= K and j >= d_real
        //   PPR [n_front]   the front-end parameters in flat order (E [d_real][K] | t [d_real] | W [K][2+K] | c [K])
        //   PXS, PMQ, PMP [16][a.d]   x and the masks of both passes as floats; rows past B and columns past d_real are 0
        // 4 096 + 3 328 + 3 x 1 024 = 10 496 floats at the limits d = 64, K = 32.
        float* const PT = buf(B_Z);
        float* const PPR = PT + 4096;
        float* const PXS = PPR + 3328;
        float* const PMQ = PXS + 1024;
        float* const PMP = PMQ + 1024;
        auto pn_stage = [&]() {
            const int K = pnx.K, dr = a.d_real, dp = a.d;
            const int nfront = dr * K + dr + K * (2 + K) + K;
            // (opaque thread id: the stage runs twice, and what the two copies share would otherwise be kept in registers
            // across the whole step - launder() in vpc_device.h)
            int tid = threadIdx.x, tid2 = 0;
            launder(tid, tid2);
            for (int i = tid; i < nfront; i += THREADS) PPR[i] = pnx.front[i];
            for (int i = tid; i < 16 * dp; i += THREADS) {
                const int r = i / dp, j = i - r * dp;
                const bool in = row0 + r < a.B && j < dr;
                const long g = (row0 + r) * dp + j;
                PXS[i] = in ? a.x[g] : 0.f;
                PMQ[i] = (in && a.m[0][g]) ? 1.f : 0.f;
                PMP[i] = (two && in && a.m[1][g]) ? 1.f : 0.f;
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
        };
        if constexpr (PN) {
            // ---- input stage of both passes (eddi_front_fwd_kernel; VAE.py:719-733, 903-917): thread (row r, k) sums
            // m[r][j] relu(x[r][j] A_j[k] + C_j[k]) over the features in a fixed order; columns K .. 16 DTI - 1 are written as 0
            pn_stage();
            int tid = threadIdx.x, tid2 = 0;
            launder(tid, tid2);
            const int r = tid >> 5, k = tid & 31, dp = a.d;
            float sq = 0.f, sp = 0.f;
#pragma unroll 4
            for (int j = 0; j < a.d_real; ++j) {
                const float h = fmaxf(PXS[r * dp + j] * PT[64 * j + k] + PT[64 * j + 32 + k], 0.f);
                sq += PMQ[r * dp + j] * h;
                sp += PMP[r * dp + j] * h;
            }
            if (k < 16 * DTI) {
                buf(B_XQ)[r * SP + k] = k < pnx.K ? sq : 0.f;
                if (two) buf(B_XP)[r * SP + k] = k < pnx.K ? sp : 0.f;
            }
        }
        // ================================================================ E: encoder forward of both passes
        // (every stage requests the weight fragments of the NEXT stage before it computes: a stage is ~30 MFMAs, an L2 round
        // trip as long as that; lds_barrier() leaves those loads in flight)
        for (int p = 0; p < a.npass; ++p) {
            weights();
            float* X = buf(p == 0 ? B_XQ : B_XP);
            float* H1b = buf(p == 0 ? B_H1Q : B_H1P);
            float* H2b = buf(p == 0 ? B_H2Q : B_H2P);
            f32x4 fW1[DTI], fW2[H1T], fW3[H2T], bias1 = zero4();
            if (w < H1T) {
                ldW<DTI, S1>(W1, w, cc, qq, fW1);
                bias1 = *reinterpret_cast<const f32x4*>(b1 + 16 * w + 4 * qq);
            }
            if constexpr (PN) {
                // (the X buffers of both passes hold agg already: the input stage above)
            } else if constexpr (!AUG) {
                if (w < DT) st_act(X, w, cc, qq, xv * mask_to_f32(p == 0 ? mwq : mwp));  // x.float() * mask  (VAE.py:388)
            } else {
                // [x*mask | mask | 0] (ld_input<.., true> of vpc_enc.hip; VAE.py:545-548): element f < d is x_f m_f, d <= f < 2 d
                // is m_{f-d}, 2 d <= f < 16 DTI is 0.  Column d is in general not 4-aligned, so every element is a dword store of
                // its own; each column of the buffer has exactly one writer.  Rows past B: xv and the mask words are 0.
                const f32x4 mk = mask_to_f32(p == 0 ? mwq : mwp), xm = xv * mk;
                float* xrow = X + cc * SP;
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
                for (int t = 0; t < DTI; ++t) in[t] = ld_act(X, t, cc, qq);
                st_act(H1b, w, cc, qq, relu4(mmW<DTI>(fW1, in, bias1)));
            }
            if (w < 2) ldW<H2T, 64>(W3, w, cc, qq, fW3);
            lds_barrier();
            launder(cc, qq);
            if (w < H2T) {
                f32x4 in[H1T];
#pragma unroll
                for (int t = 0; t < H1T; ++t) in[t] = ld_act(H1b, t, cc, qq);
                st_act(H2b, w, cc, qq, relu4(mmW<H1T, NK1>(fW2, in, zero4())));
            }
            lds_barrier();
            launder(cc, qq);
            if (w < 2) {  // wave 0: mean tile, wave 1: logvar tile -> ML tiles 2 p, 2 p + 1
                f32x4 in[H2T];
#pragma unroll
                for (int t = 0; t < H2T; ++t) in[t] = ld_act(H2b, t, cc, qq);
                f32x4 o = mmW<H2T, NK2>(fW3, in, zero4());
                if (!ok) o = zero4();  // rows past B: statistics 0
                st_act(buf(B_ML), 2 * p + w, cc, qq, o);
            }
        }
        lds_barrier();
        launder(cc, qq);
        // ================================================================ per pass: decoder, loss, all backward
        for (int p = 0; p < a.npass; ++p) {
            weights();
            const float* X = buf(p == 0 ? B_XQ : B_XP);
            const float* H1b = buf(p == 0 ? B_H1Q : B_H1P);
            const float* H2b = buf(p == 0 ? B_H2Q : B_H2P);
            f32x4 fW4[1], fW5[H2T], fW6[H1T], fT6[DT], fT5[H1T], fT4[H2T];
            float* DML = buf(p == 0 ? B_DMLQ : B_DMLP);
            if (w < H2T) ldW<1, S4>(W4, w, cc, qq, fW4);
            if (w < H1T) ldW<H2T, 64>(W5, w, cc, qq, fW5);
            const f32x4 mu = ld_act(buf(B_ML), 2 * p, cc, qq), lv = ld_act(buf(B_ML), 2 * p + 1, cc, qq);
            const f32x4 e = ld_lat(a.eps[p]);
            if (w == 0) {  // z = mean + eps * exp(logvar / 2); z[L] = 1 drives the bias chain
                f32x4 z;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    z[j] = mu[j] + ((4 * qq + j < a.L) ? e[j] : 0.f) * __expf(0.5f * lv[j]);
                    if (4 * qq + j == a.L) z[j] = 1.f;
                }
                st_act(buf(B_Z), 0, cc, qq, z);
            }
            lds_barrier();
            launder(cc, qq);
            if (w < H2T) {
                const f32x4 in[1] = {ld_act(buf(B_Z), 0, cc, qq)};
                st_act(buf(B_G1), w, cc, qq, relu4(mmW<1>(fW4, in, zero4())));
            }
            if (w < DT) ldW<H1T, 128>(W6, w, cc, qq, fW6);
            lds_barrier();
            launder(cc, qq);
            if (w < H1T) {
                f32x4 in[H2T];
#pragma unroll
                for (int t = 0; t < H2T; ++t) in[t] = ld_act(buf(B_G1), t, cc, qq);
                st_act(buf(B_G2), w, cc, qq, relu4(mmW<H2T, NK2>(fW5, in, zero4())));
            }
            lds_barrier();
            launder(cc, qq);
            if (w < DT) {  // output tile w: forward, loss terms, d / d pre-activation
                f32x4 in[H1T];
#pragma unroll
                for (int t = 0; t < H1T; ++t) in[t] = ld_act(buf(B_G2), t, cc, qq);
                const f32x4 pre = mmW<H1T, NK1>(fW6, in, zero4());
                const uint32_t ua = p == 0 ? mwq : mwp;
                const uint32_t ub = a.mB[p] ? (p == 0 ? mwp : mwq) : ua;  // (host: the second mask is the other pass's)
                const f32x4 mA = mask_to_f32(ua), mE = mask_to_f32(ua & ~ub);
                const float kA = a.cA[p] * inv_s2 * a.inv_B, kE = a.cE[p] * inv_s2 * a.inv_B, hinv_s2 = 0.5f * inv_s2;
                f32x4 dp;
                float sa = 0.f, se = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xh = fast_sigmoid(pre[j]);
                    const float diff = xh - xv[j];
                    const float t = diff * diff * hinv_s2 + half_lv;
                    sa += mA[j] * t;
                    se += mE[j] * t;
                    dp[j] = (kA * mA[j] + kE * mE[j]) * diff * (xh - xh * xh);
                }
                if (p == 0) { S_A0 += sa; S_E0 += se; } else { S_A1 += sa; }
                st_act(buf(B_DP), w, cc, qq, dp);
            }
            if (w < H1T) ldWT<DT, 128>(W6, w, cc, qq, fT6);  // dg2's fragments
            lds_barrier();
            launder(cc, qq);
            // ---- dW6~ (wave w: out tile w, 7 in tiles)  |  dg2 = relu'(g2) * (W6~^T dpre) (waves 0-6: tile w)
            if (w < DT) {
#pragma unroll
                for (int nt = 0; nt < H1T; ++nt) acc6[nt] = wgrad16(buf(B_DP), w, buf(B_G2), nt, acc6[nt], cc, qq);
            }
            if (w < H1T) {
                f32x4 in[DT];
#pragma unroll
                for (int t = 0; t < DT; ++t) in[t] = ld_act(buf(B_DP), t, cc, qq);
                st_act(buf(B_DG2), w, cc, qq, gate4(mmW<DT>(fT6, in, zero4()), ld_act(buf(B_G2), w, cc, qq)));
            }
            if (w < H2T) ldWT<H1T, 64, NK1>(W5, w, cc, qq, fT5);  // dg1's fragments
            lds_barrier();
            launder(cc, qq);
            // ---- dW5~ (wave w: in tile w & 3 of out tiles 4 (w >> 2) .. + 3)  |  dg1 (waves 0-3)
            {
                const int nt5 = w & 3, mt5 = 4 * (w >> 2);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < 3 || w < 4) acc5[i] = wgrad16(buf(B_DG2), mt5 + i, buf(B_G1), nt5, acc5[i], cc, qq);
            }
            if (w < H2T) {
                f32x4 in[H1T];
#pragma unroll
                for (int t = 0; t < H1T; ++t) in[t] = ld_act(buf(B_DG2), t, cc, qq);
                st_act(buf(B_DG1), w, cc, qq, gate4(mmW<H1T, NK1>(fT5, in, zero4()), ld_act(buf(B_G1), w, cc, qq)));
            }
            if (w == 4) ldWT<H2T, S4, NK2>(W4, 0, cc, qq, fT4);  // dz's fragments
            lds_barrier();
            launder(cc, qq);
            // ---- dW4~ (waves 0-3: out tile w)  |  wave 4: dz, KL terms, seeds on (mean | logvar) -> DML
            if (w < H2T) acc4 = wgrad16(buf(B_DG1), w, buf(B_Z), 0, acc4, cc, qq);
            if (w == 4) {
                f32x4 in[H2T];
#pragma unroll
                for (int t = 0; t < H2T; ++t) in[t] = ld_act(buf(B_DG1), t, cc, qq);
                const f32x4 dz = mmW<H2T, NK2>(fT4, in, zero4());
                const f32x4 mo = two ? ld_act(buf(B_ML), 2 * (1 - p), cc, qq) : zero4();
                const f32x4 lo = two ? ld_act(buf(B_ML), 2 * (1 - p) + 1, cc, qq) : zero4();
                f32x4 dmu, dlv;
                const float b0 = (p == 0) ? a.bq : a.bp;
                const float sgn = (p == 0) ? 1.f : -1.f;
                const float crr = two ? a.cr : 0.f;
                float kl0 = 0.f, klr = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float elv = __expf(lv[j]);
                    kl0 += 0.5f * (elv + mu[j] * mu[j] - 1.f - lv[j]);
                    const float mq = (p == 0) ? mu[j] : mo[j], lq = (p == 0) ? lv[j] : lo[j];
                    const float mp = (p == 0) ? mo[j] : mu[j], lp = (p == 0) ? lo[j] : lv[j];
                    const float diff = mq - mp, eip = __expf(-lp), r = __expf(lq - lp);
                    klr += 0.5f * (r + diff * diff * eip - 1.f - (lq - lp));
                    const float dm = b0 * mu[j] + sgn * crr * diff * eip;
                    const float dl = b0 * 0.5f * (elv - 1.f) + crr * 0.5f * ((p == 0) ? (r - 1.f) : (1.f - r - diff * diff * eip));
                    dmu[j] = dm * a.inv_B;
                    dlv[j] = dl * a.inv_B;
                }
                if (p == 0) { S_kl0q += kl0; if (two) S_klr += klr; } else { S_kl0p += kl0; }
                if (two && a.wml != 0.f) {  // ml_reg: extra rsample z' of q scored under p (VAE.py:435-440)
                    const f32x4 e3 = ld_lat(a.eps_ml);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool live = ok && 4 * qq + j < a.L;
                        const float e3j = (4 * qq + j < a.L) ? e3[j] : 0.f;
                        const float mq = (p == 0) ? mu[j] : mo[j], lq = (p == 0) ? lv[j] : lo[j];
                        const float mp = (p == 0) ? mo[j] : mu[j], lp = (p == 0) ? lo[j] : lv[j];
                        const float sq = __expf(0.5f * lq), eip = __expf(-lp);
                        const float dlt = mq + e3j * sq - mp;
                        const float g = a.wml * dlt * eip * a.inv_B;
                        if (p == 0) {
                            if (live) S_zll += -HL2PI - 0.5f * lp - 0.5f * dlt * dlt * eip;
                            dmu[j] += g;
                            dlv[j] += g * e3j * 0.5f * sq;
                        } else {
                            dmu[j] -= g;
                            dlv[j] += live ? a.wml * (0.5f - 0.5f * dlt * dlt * eip) * a.inv_B : 0.f;
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float ef = (4 * qq + j < a.L) ? e[j] * 0.5f * __expf(0.5f * lv[j]) : 0.f;
                    dmu[j] = (4 * qq + j < a.L) ? dmu[j] + dz[j] : 0.f;  // columns >= L carry no gradient (dz's column L is db4)
                    dlv[j] = (4 * qq + j < a.L) ? dlv[j] + dz[j] * ef : 0.f;
                }
                st_act(DML, 0, cc, qq, dmu);
                st_act(DML, 1, cc, qq, dlv);
            }
            lds_barrier();
            launder(cc, qq);
        }
        // ================================================================ decoder partial block and the loss terms
        {
            float* part = a.partD + (long)tile_id * DEC_PART + (long)(w & 3) * DEC_GREGS * 64 + lane;
            const int hi = w >> 2;
#pragma unroll
            for (int nt = 0; nt < H1T; ++nt)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[(28 * hi + 4 * nt + j) * 64] = (w < DT) ? acc6[nt][j] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float* p5 = a.partD + (long)tile_id * DEC_PART + (long)i * DEC_GREGS * 64 + lane;
#pragma unroll
                for (int j = 0; j < 4; ++j) p5[(56 + 16 * hi + 4 * (w & 3) + j) * 64] = (i < 3 || w < 4) ? acc5[i][j] : 0.f;
            }
            if (w < H2T) {
#pragma unroll
                for (int j = 0; j < 4; ++j) part[(88 + j) * 64] = acc4[j];
            }
            const float s[LOSS_TERMS] = {S_A0, S_E0, S_A1, S_kl0q, S_kl0p, S_klr, S_zll, 0.f};
#pragma unroll
            for (int i = 0; i < LOSS_TERMS; ++i) {
                const float v = wave_sum_dpp(s[i]);
                if (lane == 0) red[w * LOSS_TERMS + i] = v;
            }
            lds_barrier();
            if (threadIdx.x < LOSS_TERMS) {
                double t = 0.0;
                for (int k = 0; k < WAVES; ++k) t += (double)red[k * LOSS_TERMS + threadIdx.x];
                a.loss_part[(long)tile_id * LOSS_TERMS + threadIdx.x] = t;
            }
        }
        // ================================================================ encoder backward of both passes
        f32x4 acc1[H1T], acc2[H2T], acc3 = zero4(), dbacc = zero4();
#pragma unroll
        for (int t = 0; t < H1T; ++t) acc1[t] = zero4();
#pragma unroll
        for (int t = 0; t < H2T; ++t) acc2[t] = zero4();
        for (int p = 0; p < a.npass; ++p) {
            weights();
            const float* X = buf(p == 0 ? B_XQ : B_XP);
            const float* H1b = buf(p == 0 ? B_H1Q : B_H1P);
            const float* H2b = buf(p == 0 ? B_H2Q : B_H2P);
            const float* DML = buf(p == 0 ? B_DMLQ : B_DMLP);
            f32x4 fT3[2], fT2[H2T];
            if (w < H2T) ldWT<2, 64>(W3, w, cc, qq, fT3);    // dh2's fragments
            if (w < H1T) ldWT<H2T, 128, NK2>(W2, w, cc, qq, fT2);  // dh1's fragments
            f32x4 fT1[H1T];  // (PN only; never written or read otherwise)
            if constexpr (PN) {
                if (w < DTI) ldWT<H1T, S1, NK1>(W1, w, cc, qq, fT1);  // dagg's fragments
            }
            // ---- dW3~ (wave w: out tile w >> 2, in tile w & 3)  |  dh2 (waves 0-3)
            acc3 = wgrad16(DML, w >> 2, H2b, w & 3, acc3, cc, qq);
            if (w < H2T) {
                const f32x4 in[2] = {ld_act(DML, 0, cc, qq), ld_act(DML, 1, cc, qq)};
                st_act(buf(B_DH2), w, cc, qq, gate4(mmW<2>(fT3, in, zero4()), ld_act(H2b, w, cc, qq)));
            }
            lds_barrier();
            launder(cc, qq);
            // ---- dW2~ (waves 0-6: in tile w, 4 out tiles)  |  dh1 (waves 0-6), db1 += column sums of dh1
            if (w < H1T) {
#pragma unroll
                for (int mt = 0; mt < H2T; ++mt) acc2[mt] = wgrad16(buf(B_DH2), mt, H1b, w, acc2[mt], cc, qq);
                f32x4 in[H2T];
#pragma unroll
                for (int t = 0; t < H2T; ++t) in[t] = ld_act(buf(B_DH2), t, cc, qq);
                const f32x4 dh1 = gate4(mmW<H2T, NK2>(fT2, in, zero4()), ld_act(H1b, w, cc, qq));
                st_act(buf(B_DH1), w, cc, qq, dh1);
                dbacc += dh1;  // per-lane (row c) running sums; the sum over the rows happens once, at the end
            }
            lds_barrier();
            launder(cc, qq);
            // ---- dW1 (wave w < DTI: in tile w, 7 out tiles)
            if (w < DTI) {
#pragma unroll
                for (int mt = 0; mt < H1T; ++mt) acc1[mt] = wgrad16(buf(B_DH1), mt, X, w, acc1[mt], cc, qq);
                if constexpr (PN) {
                    // dagg = dh1 . W1 (the layer-0 dgrad the dense body has no use for: x carries no gradient), tile w of the
                    // pass, into the pass's H2 buffer - dead since the dW3 / dh2 stage
                    f32x4 in[H1T];
#pragma unroll
                    for (int t = 0; t < H1T; ++t) in[t] = ld_act(buf(B_DH1), t, cc, qq);
                    st_act(buf(p == 0 ? B_H2Q : B_H2P), w, cc, qq, mmW<H1T, NK1>(fT1, in, zero4()));
                }
            }
            lds_barrier();
            launder(cc, qq);
        }
        // ================================================================ encoder partial block
        {
            float* part = a.partE + (long)tile_id * ENC_PART + (long)w * GREGS * 64 + lane;
#pragma unroll
            for (int mt = 0; mt < H1T; ++mt)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[(4 * mt + j) * 64] = (w < DTI) ? acc1[mt][j] : 0.f;
#pragma unroll
            for (int mt = 0; mt < H2T; ++mt)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[(28 + 4 * mt + j) * 64] = (w < H1T) ? acc2[mt][j] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) part[(44 + j) * 64] = acc3[j];
            // db1[16 w + 4 q + j] = sum over the 16 rows (lanes c) of dbacc: DPP butterfly inside each 16-lane row
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = dbacc[j];
                v += dpp_mov<0xB1>(v);
                v += dpp_mov<0x4E>(v);
                v += dpp_mov<0x141>(v);
                v += dpp_mov<0x140>(v);
                if (c == 0 && w < H1T) a.partE[(long)tile_id * ENC_PART + WAVES * GREGS * 64 + 16 * w + 4 * q + j] = v;
            }
            if (w == 7 && lane < 16) a.partE[(long)tile_id * ENC_PART + WAVES * GREGS * 64 + 112 + lane] = 0.f;
        }
        if constexpr (PN) {
            // ================================================================ front-end backward (eddi_front_bwd_kernel)
            // dA[k][j] = sum over passes and rows of g x, dC[k][j] = sum of g, g = m 1[x A + C > 0] dagg: gates recomputed from
            // the re-staged table; thread (k, j) walks pass 0's rows, then pass 1's - a fixed order, no atomics.  The tile's
            // block is [dA | dC], each [K][a.d], columns past d_real zero.
            pn_stage();  // (its first barrier is behind the encoder backward's last stage: B_Z .. B_DG1 are idle again)
            const int K = pnx.K, dp = a.d;
            const float *DQ = buf(B_H2Q), *DPp = buf(B_H2P);
            float* pf = pnx.partF + (long)tile_id * 2 * K * dp;
            int tid = threadIdx.x, tid2 = 0;
            launder(tid, tid2);
            for (int i = tid; i < 32 * dp; i += THREADS) {
                const int k = i & 31, j = i >> 5;
                if (k >= K) continue;
                const float A = PT[64 * j + k], C = PT[64 * j + 32 + k];
                float dA = 0.f, dC = 0.f;
                for (int pp = 0; pp < a.npass; ++pp) {
                    const float* M = pp == 0 ? PMQ : PMP;
                    const float* D = pp == 0 ? DQ : DPp;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float xr = PXS[r * dp + j];
                        const float g = (xr * A + C > 0.f) ? M[r * dp + j] * D[r * SP + k] : 0.f;
                        dA += g * xr;
                        dC += g;
                    }
                }
                pf[k * dp + j] = dA;
                pf[(K + k) * dp + j] = dC;
            }
            // the parameters this step's gradients were taken at, for the tail's chain rule: its Adam blocks overwrite them in place
            if (tile_id == 0) {
                const int nfront = a.d_real * K + a.d_real + K * (2 + K) + K;
                for (int i = tid; i < nfront; i += THREADS) pnx.snap[i] = PPR[i];
            }
        }
    }
