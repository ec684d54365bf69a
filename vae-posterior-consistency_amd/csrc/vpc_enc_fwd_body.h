// The BODY of the encoder forward kernels (vpc_enc.hip), included as text into
//   enc_fwd_kernel<DT, VEC, AUG, NW, PREC>   (DRAW = false: both passes fetch their mask) and
//   enc_fwd_draw_kernel<DT>                  (VEC = true, AUG = false, NW = 8, PREC = PREC_F32, DRAW = true: pass 1 draws mask_p),
// so that both run ONE piece of code and enc_fwd_kernel compiles to the instructions it had as a self-contained kernel (a shared
// inline function is simplified before it is inlined and schedules differently: vpc_small_body.h).
// In scope at the point of inclusion: DT, VEC, AUG, NW, PREC, DRAW, a (EncFwdArgs), dr (EncDraw; only read when DRAW).
// (No include guard: this is a code fragment, included once per kernel.)
    constexpr int TILE_ROWS = 16 * NW;  // shadows vpc::TILE_ROWS (the 8-wave value)
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

    // PIPE (the vectorised fast path): x is read once per tile (both passes see the same rows, only the mask differs)
    // and the mask words of the next pass - or x and the mask words of the next tile - are requested before this
    // pass's MFMAs, with branch-free loads (rows past B read row 0 and are never stored; columns past d are cleared).
    constexpr bool PIPE = VEC && !AUG;
    static_assert(!DRAW || (PIPE && NW == 8 && PREC == PREC_F32 && DT % 2 == 0), "the drawing form is the 8-wave fp32 fast path");
    f32x4 xraw[DT];
    uint32_t mw[DT];
    const int cq = (4 * q + 3 < a.d) ? 4 * q : 0;
    // range-checked buffer loads relative to a tile's first row t0 (rows past B read 0)
    const int vo = (w * 16 + c) * a.d + cq;  // element offset of this lane's row / column group inside the tile's rows
    auto fetch_x = [&](long t0) {
        const __amdgpu_buffer_rsrc_t rx = rows_rsrc(a.x, t0, a.B, a.d);
#pragma unroll
        for (int t = 0; t < DT; ++t)
            xraw[t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                rx, 4 * (vo + ((t < DT / 2 || 16 * t + 4 * q + 3 < a.d) ? 16 * t : 0)), 0, 0));
    };
    auto fetch_m = [&](const uint8_t* m, long t0) {
        const long rem = (a.B - t0) * (long)a.d;
        const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(m) + t0 * a.d, 0, rem > 0xffffffffL ? 0xffffffffu : (uint32_t)rem, 0x00020000);
#pragma unroll
        for (int t = 0; t < DT; ++t)
            mw[t] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
                rm, vo + ((t < DT / 2 || 16 * t + 4 * q + 3 < a.d) ? 16 * t : 0), 0, 0);
    };
    const int p_lo = a.psplit ? (int)blockIdx.y : 0, p_hi = a.psplit ? p_lo + 1 : a.npass;
    uint64_t off_mask = 0;
    if (DRAW) off_mask = dr.off_mask + (dr.state ? (uint64_t)dr.state[1] : 0);
    // the first tile's x / mask words are requested BEFORE the weight image: both latencies overlap
    if (PIPE && (int)blockIdx.x < a.ntiles) {
        fetch_x((long)blockIdx.x * TILE_ROWS);
        fetch_m(a.mask[p_lo], (long)blockIdx.x * TILE_ROWS);
    }
    // DRAW: the keep bits of the mask words this lane holds of the tile at local row `r0` (pass 1's mask = pass 0's & keep),
    // drawn at the head of pass 1.  Every lane of the wave is active where this is called (the swap needs both lanes of a
    // pair); rows past B draw too and their stores are dropped by the range check.
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
    load_image<(NW == 8 ? 13 : 25)>(lds, a.img, im.total);
    __syncthreads();
    VPC_STAMP(0);

    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long row = (long)tile * TILE_ROWS + w * 16 + c;
        const bool ok = row < a.B;
        for (int p = p_lo; p < p_hi; ++p) {
            // the weight image never changes after the prologue: without this compiler barrier LICM hoists
            // every LDS weight read out of the pass loop and spills ~1 KB/lane of it to scratch
            asm volatile("" ::: "memory");
            int cc = c, qq = q;
            launder(cc, qq);
            // workspace stores go through range-checked buffer descriptors (rows past B are dropped by the hardware)
            const long row0 = (long)tile * TILE_ROWS;
            const int lrow = w * 16 + c;
            const __amdgpu_buffer_rsrc_t rh1 = rows_rsrc(a.h1[p], row0, a.B, H1P), rh2 = rows_rsrc(a.h2[p], row0, a.B, H2P);
            f32x4 xin[DT];
            if (PIPE) {
                if (DRAW && p == 1) {
                    draw_keep(row0, qq);
                    const long mrem = (a.B - row0) * (long)a.d;
                    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
                        dr.mask_out + row0 * a.d, 0, mrem > 0xffffffffL ? 0xffffffffu : (uint32_t)mrem, 0x00020000);
#pragma unroll
                    for (int t = 0; t < DT; ++t) {
                        mw[t] &= keep[DRAW ? t : 0];
                        asm volatile("" : "+v"(mw[t]));
                        if (t < DT / 2 || 16 * t + 4 * q + 3 < a.d)  // out-of-range column groups hold a word of tile 0: not stored
                            __builtin_amdgcn_raw_buffer_store_b32((int)mw[t], ro, vo + 16 * t, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    const uint32_t vm = opaque_mask(t < DT / 2 || 16 * t + 4 * q + 3 < a.d);
                    xin[t] = xraw[t] * mask_to_f32(mw[t] & vm);  // x.float() * mask  (VAE.py:388)
                }
                if (p + 1 < p_hi) {
                    if (!DRAW) fetch_m(a.mask[p + 1], row0);  // (DRAW: pass 1 = these words & the keep bits drawn at its head)
                } else if (tile + (int)gridDim.x < a.ntiles) {
                    const long tn = row0 + (long)gridDim.x * TILE_ROWS;
                    fetch_x(tn);
                    fetch_m(a.mask[p_lo], tn);
                }
            } else {
#pragma unroll
                for (int t = 0; t < DT; ++t) xin[t] = ld_input<VEC, AUG>(a.x, a.mask[p], row, a.d, t, q, ok);
            }
            VPC_STAMP(1);
            f32x4 h1[H1T], h2[H2T], mu, lv;
            if (PREC == PREC_F32) {
#pragma unroll
                for (int mt = 0; mt < H1T; ++mt) {
                    f32x4 acc = *reinterpret_cast<const f32x4*>(b1 + 16 * mt + 4 * q);
                    acc = tile_fwd<DT, S1>(W1, mt, xin, acc, cc, qq);
                    h1[mt] = relu4(acc);
                    st_rows(rh1, lrow, H1P, 16 * mt + 4 * q, h1[mt]);
                }
                VPC_STAMP(2);
                launder(cc, qq);
#pragma unroll
                for (int mt = 0; mt < H2T; ++mt) {
                    h2[mt] = relu4(tile_fwd<H1T, 128, NK1>(W2, mt, h1, zero4(), cc, qq));
                    st_rows(rh2, lrow, H2P, 16 * mt + 4 * q, h2[mt]);
                }
                VPC_STAMP(3);
                mu = tile_fwd<H2T, 64, NK2>(W3, 0, h2, zero4(), cc, qq);
                lv = tile_fwd<H2T, 64, NK2>(W3, 1, h2, zero4(), cc, qq);
            } else {
                constexpr int KB1 = (DT + 1) / 2;
                BfOp xb[KB1];
                bf_acts<PREC, DT>(xin, xb);
                // (fragments of tile mt + 1 in flight during tile mt: vpc_bf16.h, bf_layer_fwd)
                // plain bf16: the h1 / h2 workspaces hold the PACKED operands (what the backward kernel's MFMAs consume
                // anyway): rows of [k-block][q][8 x bf16], 256 / 128 bytes per row inside the same allocation - half the
                // bytes of the fp32 rows in both directions (enc_fwd is HBM-bound in this form)
                constexpr bool HPK = PREC == PREC_BF16;
                bf_layer_fwd<PREC, KB1, S1, H1T, PREC == PREC_BF16 ? KB1 : (KB1 < 2 ? KB1 : 2)>(W1, xb, cc, qq, [&](int mt, f32x4 acc) {
                    h1[mt] = relu4(acc + *reinterpret_cast<const f32x4*>(b1 + 16 * mt + 4 * q));
                    if (!HPK) st_rows(rh1, lrow, H1P, 16 * mt + 4 * q, h1[mt]);
                });
                VPC_STAMP(2);
                launder(cc, qq);
                BfOp h1b[4];
                bf_acts<PREC, H1T>(h1, h1b);
                if (HPK) {
                    const __amdgpu_buffer_rsrc_t rp = rows_rsrc(a.h1[p], row0, a.B, 64);
#pragma unroll
                    for (int kb = 0; kb < 4; ++kb) st_rows(rp, lrow, 64, 16 * kb + 4 * q, __builtin_bit_cast(f32x4, h1b[kb].hi));
                }
                bf_layer_fwd<PREC, 4, 128, H2T, PREC == PREC_BF16 ? 4 : 2>(W2, h1b, cc, qq, [&](int mt, f32x4 acc) {
                    h2[mt] = relu4(acc);
                    if (!HPK) st_rows(rh2, lrow, H2P, 16 * mt + 4 * q, h2[mt]);
                });
                VPC_STAMP(3);
                BfOp h2b[2];
                bf_acts<PREC, H2T>(h2, h2b);
                if (HPK) {
                    const __amdgpu_buffer_rsrc_t rp = rows_rsrc(a.h2[p], row0, a.B, 32);
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) st_rows(rp, lrow, 32, 16 * kb + 4 * q, __builtin_bit_cast(f32x4, h2b[kb].hi));
                }
                mu = bf_tile_fwd<PREC, 2, 64>(W3, 0, h2b, zero4(), cc, qq);
                lv = bf_tile_fwd<PREC, 2, 64>(W3, 1, h2b, zero4(), cc, qq);
            }
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
            VPC_STAMP(4);
        }
    }
#ifdef VPC_ABLATE
    if ((blockIdx.x == 0 || blockIdx.x == 100) && (threadIdx.x & 63) == 0 && (threadIdx.x >> 6) < 2)
        printf("enc_fwd blk %d wave %d cycles: prologue %llu loadx %llu L1 %llu L2 %llu L3+st %llu | total %llu cycles in %llu x 10 ns\n",
               blockIdx.x, (int)(threadIdx.x >> 6), T[0], T[1], T[2], T[3], T[4],
               (unsigned long long)(__builtin_amdgcn_s_memtime() - t_begin),
               (unsigned long long)(__builtin_amdgcn_s_memrealtime() - r_begin));
#endif
