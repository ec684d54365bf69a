// The BODY of the encoder forward SWEEP kernels (vpc_enc.hip), included as text into
//   enc_fwd_sweep_kernel<DT, DRAW>   (DRAW = false: both passes fetch their mask; true: pass 1's mask is drawn),
// the form of enc_fwd_kernel<DT, true, false, 8, PREC_F32> / enc_fwd_draw_kernel<DT> (vpc_enc_fwd_body.h) for two passes in one
// workgroup that runs BOTH passes of a 128-row tile in one sweep over the weight image: x and the mask words are read once, the
// layer-1 inputs of both passes are formed at the head of the tile, and every A fragment of W1 / W2 / W3 feeds the pass-0 and
// the pass-1 accumulator alternately (layer_fwd2_b, vpc_device.h): half the LDS reads and waits of two pass loops, two
// independent MFMA chains per wave, the fragment stream requested one ahead and pinned.  Each accumulator sees the k-steps of
// its pass in the order of tile_fwd, so every workspace holds the bytes the pass loop writes.
// In scope at the point of inclusion: DT, DRAW, a (EncFwdArgs; npass == 2, psplit == 0), dr (EncDraw; only read when DRAW).
// (No include guard: this is a code fragment, included once per kernel.)
    constexpr int NW = 8, TILE_ROWS = 16 * NW;  // shadows vpc::TILE_ROWS
    static_assert(DT == 8, "the sweep exists for d in (64, 128]");
    extern __shared__ __attribute__((aligned(16))) float lds[];
#ifdef VPC_ABLATE
    unsigned long long T[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tlast = __builtin_amdgcn_s_memtime();
    const unsigned long long t_begin = tlast, r_begin = __builtin_amdgcn_s_memrealtime();
#endif
    constexpr int S1 = s_for_tiles(DT);
    const EncImg im(DT);
    const float* W1 = lds + im.oW1;
    const float* b1 = lds + im.ob1;
    const float* W2 = lds + im.oW2;
    const float* W3 = lds + im.oW3;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;

    // x is read once per tile, and the mask words of pass 0 (DRAW) or of both passes; the next tile's are requested under this
    // tile's sweep, with branch-free loads (rows past B read 0 and are never stored; columns past d are cleared)
    f32x4 xraw[DT];
    uint32_t mw[2][DT];
    const int cq = (4 * q + 3 < a.d) ? 4 * q : 0;
    const int vo = (w * 16 + c) * a.d + cq;  // element offset of this lane's row / column group inside the tile's rows
    auto fetch_x = [&](long t0) {
        const __amdgpu_buffer_rsrc_t rx = rows_rsrc(a.x, t0, a.B, a.d);
#pragma unroll
        for (int t = 0; t < DT; ++t)
            xraw[t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                rx, 4 * (vo + ((t < DT / 2 || 16 * t + 4 * q + 3 < a.d) ? 16 * t : 0)), 0, 0));
    };
    auto fetch_m = [&](int p, long t0) {
        const long rem = (a.B - t0) * (long)a.d;
        const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(a.mask[p]) + t0 * a.d, 0, rem > 0xffffffffL ? 0xffffffffu : (uint32_t)rem, 0x00020000);
#pragma unroll
        for (int t = 0; t < DT; ++t)
            mw[p][t] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
                rm, vo + ((t < DT / 2 || 16 * t + 4 * q + 3 < a.d) ? 16 * t : 0), 0, 0);
    };
    auto fetch_tile = [&](long t0) {
        fetch_x(t0);
        fetch_m(0, t0);
        if (!DRAW) fetch_m(1, t0);
    };
    uint64_t off_mask = 0;
    if (DRAW) off_mask = dr.off_mask + (dr.state ? (uint64_t)dr.state[1] : 0);
    // the first tile's x / mask words are requested BEFORE the weight image: both latencies overlap
    if ((int)blockIdx.x < a.ntiles) fetch_tile((long)blockIdx.x * TILE_ROWS);
    // DRAW: the keep bits of the mask words this lane holds of the tile at local row `r0` (pass 1's mask = pass 0's & keep):
    // draw_keep of vpc_enc_fwd_body.h - the same counters, lane mapping and 16-lane exchange - at the head of the tile.  Every
    // lane of the wave is active where this is called; rows past B draw too and their stores are dropped by the range check.
    uint32_t keep[DRAW ? DT : 1];
    auto draw_keep = [&](long r0, int qd) {
        const int odd = qd & 1;
        const uint32_t thr = mask_thr(dr.keep_prob);
        const uint64_t g0 = off_mask + (uint64_t)mask_lane_group(dr.elem_lo, r0 + w * 16 + c, a.d, mask_lane_call_tile(0, qd), qd);
#pragma unroll
        for (int u = 0; u < DT / 2; ++u) {
            const U4 r = philox(g0 + 4 * u, 0u, dr.seed);  // tile 2 u + odd: 2 tiles = 4 groups further per pair
            // this lane's own halves are words 2 odd, 2 odd + 1; the other two go to lane q ^ 1
            const uint32_t o0 = odd ? r.z : r.x, o1 = odd ? r.w : r.y, s0 = odd ? r.x : r.z, s1 = odd ? r.y : r.w;
            const uint32_t r0w = (uint32_t)__builtin_amdgcn_ds_swizzle((int)s0, 0x401F);  // lane ^ 16
            const uint32_t r1w = (uint32_t)__builtin_amdgcn_ds_swizzle((int)s1, 0x401F);
            const uint32_t kown = keep_bits4(o0, o1, thr), koth = keep_bits4(r0w, r1w, thr);
            keep[2 * u] = odd ? koth : kown;
            keep[2 * u + 1] = odd ? kown : koth;
        }
#pragma unroll
        for (int t = 0; t < (DRAW ? DT : 1); ++t) asm volatile("" : "+v"(keep[t]));
    };
    load_image<13>(lds, a.img, im.total);
    __syncthreads();
    VPC_STAMP(0);

    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long row = (long)tile * TILE_ROWS + w * 16 + c;
        const bool ok = row < a.B;
        // the weight image never changes after the prologue: without this compiler barrier LICM hoists every LDS weight read
        // out of the tile loop and spills it to scratch
        asm volatile("" ::: "memory");
        int cc = c, qq = q;
        launder(cc, qq);
        // workspace stores go through range-checked buffer descriptors (rows past B are dropped by the hardware)
        const long row0 = (long)tile * TILE_ROWS;
        const int lrow = w * 16 + c;
        f32x4 xin[2][DT];
        if (DRAW) {
            draw_keep(row0, qq);
            const long mrem = (a.B - row0) * (long)a.d;
            const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
                dr.mask_out + row0 * a.d, 0, mrem > 0xffffffffL ? 0xffffffffu : (uint32_t)mrem, 0x00020000);
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                mw[1][t] = mw[0][t] & keep[DRAW ? t : 0];
                asm volatile("" : "+v"(mw[1][t]));
                if (t < DT / 2 || 16 * t + 4 * q + 3 < a.d)  // out-of-range column groups hold a word of tile 0: not stored
                    __builtin_amdgcn_raw_buffer_store_b32((int)mw[1][t], ro, vo + 16 * t, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            const uint32_t vm = opaque_mask(t < DT / 2 || 16 * t + 4 * q + 3 < a.d);
            xin[0][t] = xraw[t] * mask_to_f32(mw[0][t] & vm);  // x.float() * mask  (VAE.py:388)
            xin[1][t] = xraw[t] * mask_to_f32(mw[1][t] & vm);
        }
        if (tile + (int)gridDim.x < a.ntiles) fetch_tile(row0 + (long)gridDim.x * TILE_ROWS);
        VPC_STAMP(1);
        f32x4 h1[2][H1T], h2[2][H2T], ml[2][2];
        {
            const __amdgpu_buffer_rsrc_t r0 = rows_rsrc(a.h1[0], row0, a.B, H1P), r1 = rows_rsrc(a.h1[1], row0, a.B, H1P);
            uint32_t f1[4];
            frag_bases<S1>(f1, W1, cc, qq);
            uint32_t bb = lds_addr(b1) + 16u * (uint32_t)qq;
            asm volatile("" : "+v"(bb));
            layer_fwd2_b<DT, S1, H1T, 4 * DT>(
                f1, xin[0], xin[1], [&](int mt) { return lds_ld128(bb + 64u * mt); },
                [&](int mt, f32x4 acc0, f32x4 acc1) {
                    h1[0][mt] = relu4(acc0);
                    h1[1][mt] = relu4(acc1);
                    st_rows(r0, lrow, H1P, 16 * mt + 4 * q, h1[0][mt]);
                    st_rows(r1, lrow, H1P, 16 * mt + 4 * q, h1[1][mt]);
                });
        }
        VPC_STAMP(2);
        launder(cc, qq);
        {
            const __amdgpu_buffer_rsrc_t r0 = rows_rsrc(a.h2[0], row0, a.B, H2P), r1 = rows_rsrc(a.h2[1], row0, a.B, H2P);
            uint32_t f2[4];
            frag_bases<128>(f2, W2, cc, qq);
            layer_fwd2_b<H1T, 128, H2T, NK1>(
                f2, h1[0], h1[1], [&](int) { return zero4(); },
                [&](int mt, f32x4 acc0, f32x4 acc1) {
                    h2[0][mt] = relu4(acc0);
                    h2[1][mt] = relu4(acc1);
                    st_rows(r0, lrow, H2P, 16 * mt + 4 * q, h2[0][mt]);
                    st_rows(r1, lrow, H2P, 16 * mt + 4 * q, h2[1][mt]);
                });
        }
        VPC_STAMP(3);
        launder(cc, qq);
        {
            uint32_t f3[4];
            frag_bases<64>(f3, W3, cc, qq);
            layer_fwd2_b<H2T, 64, 2, NK2>(
                f3, h2[0], h2[1], [&](int) { return zero4(); },
                [&](int mt, f32x4 acc0, f32x4 acc1) {  // out tile 0: mean, 1: logvar
                    ml[0][mt] = acc0;
                    ml[1][mt] = acc1;
                });
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const f32x4 mu = ml[p][0], lv = ml[p][1];
            if (a.lp == 16) {  // padded workspaces: rows are 16 floats, features >= L are exact zeros
                st_rows(rows_rsrc(a.mean[p], row0, a.B, 16), lrow, 16, 4 * q, mu);
                st_rows(rows_rsrc(a.logvar[p], row0, a.B, 16), lrow, 16, 4 * q, lv);
            } else {
                st_tile<false>(a.mean[p], row, a.L, 4 * q, a.L, ok, mu);
                st_tile<false>(a.logvar[p], row, a.L, 4 * q, a.L, ok, lv);
            }
            if (a.z[p]) {
                f32x4 z = mu;
                if (a.eps[p]) {
                    const f32x4 e = ld_tile<false>(a.eps[p], row, a.L, 4 * q, a.L, ok);
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[j] = mu[j] + e[j] * expf(lv[j] * 0.5f);  // rsample
                }
                st_tile<false>(a.z[p], row, a.L, 4 * q, a.L, ok, z);
            }
        }
        VPC_STAMP(4);
    }
#ifdef VPC_ABLATE
    if ((blockIdx.x == 0 || blockIdx.x == 100) && (threadIdx.x & 63) == 0 && (threadIdx.x >> 6) < 2)
        printf("enc_fwd sweep blk %d wave %d cycles: prologue %llu loadx %llu L1 %llu L2 %llu L3+st %llu | total %llu cycles in %llu x 10 ns\n",
               blockIdx.x, (int)(threadIdx.x >> 6), T[0], T[1], T[2], T[3], T[4],
               (unsigned long long)(__builtin_amdgcn_s_memtime() - t_begin),
               (unsigned long long)(__builtin_amdgcn_s_memrealtime() - r_begin));
#endif
