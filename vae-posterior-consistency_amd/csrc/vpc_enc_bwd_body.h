// The BODY of the encoder backward kernels (vpc_enc.hip), included as text into
//   enc_bwd_kernel<DT, VEC, AUG, NW, PREC>   (every shape and engine) and
//   step_f32_kernel<DT>                      (vpc_step_f32.hip: phase B of the one-launch fp32 step; VEC, !AUG, NW = 8, PREC_F32),
// so that both run ONE piece of code and enc_bwd_kernel compiles to the instructions it had as a self-contained kernel (a shared
// inline function is simplified before it is inlined and schedules differently: vpc_small_body.h).
// In scope at the point of inclusion: DT, VEC, AUG, NW, PREC, a (EncBwdArgs).
// (No include guard: this is a code fragment, included once per kernel.)
    extern __shared__ __attribute__((aligned(16))) float lds[];
#ifdef VPC_ABLATE
    unsigned long long T[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tlast = __builtin_amdgcn_s_memtime();
#endif
    // Staging is full width (all batch rows of the workgroup tile at once): ONE write + barrier + read round per
    // wgrad round (two rounds: layer 2, then layers 1 + 3 together), 4 barriers per pass instead of 12 (barriers were 16 %
    // of this kernel, `profiles/r01_notes.md`).  That
    // fits in LDS because the B operand of the layer-1 wgrad - x * mask, the only use of x in this kernel - never
    // goes through LDS: a B fragment wants batch rows along the register index and features along the lanes, which
    // is how row-major x lies in memory, so the tile's owner wave reads it from global memory directly.
    constexpr int TILE_ROWS = 16 * NW, CH = TILE_ROWS, NTHR = 64 * NW, OWN = 8 / NW;
    constexpr bool PIPE = VEC && !AUG;
    const EncImg im(DT);
    const int nW = im.total - im.oW2;  // only W2, W3 are needed (layer 1 has no dgrad)
    float* W2 = lds;
    float* W3 = lds + (im.oW3 - im.oW2);
    float* stA = lds + nW;             // [112][CH]  dY operands (dml, dh2, dh1)
    float* stB = stA + H1P * CH;       // [112][CH]  activations (h2, h1)
    float* db1s = stB + H1P * CH;      // [NW][128]: per-wave bias-gradient sums (no atomics across waves: bit-reproducible)
    // bf16 engine: the same buffers hold the operands as bf16, row-major [batch row][7 tile slots], hi plane + lo plane
    // (vpc_bf16.h, bf_stage_*): written once by the owner of the row, read back with the transposing LDS read
    constexpr bool BF = PREC != PREC_F32;
    constexpr int SKB = CH / 32;
    constexpr bool LB = !BF && NW == 8 && VPC_LANE_BASES;
    constexpr int OFF_B = H1P * CH * 4;  // stB behind stA, bytes (too far for an immediate: the B buffer has bases of its own)
    static_assert(frag_imm(128, H1T - 1, 7) < 65536, "ds_read immediates are 16 bits");
    float* sAh = stA;
    float* sAl = stA + 56 * CH;
    float* sBh = stB;
    float* sBl = stB + 56 * CH;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    // the wave index as a scalar for the ownership tests (threadIdx.x >> 6 is divergent to hipcc: exec-masked regions
    // around the wgrad loops); addresses keep the vector value
    const int ws = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p_lo = a.psplit ? (int)blockIdx.y : 0, p_hi = a.psplit ? p_lo + 1 : a.npass;
    // row-layout operands of one (tile, pass) through range-checked buffer descriptors: rows past B read 0 - zero seeds make
    // dh2, dh1 and every wgrad contribution of such a row exactly zero.  (hipcc turns `ok ? load : 0` into an exec-masked
    // branch with a vmcnt(0) wait at the join.)  The first (tile, pass) of the workgroup is requested before the weight
    // image: in the small-batch shape there is only one, and the two latencies otherwise add up.
    // plain bf16: h1 / h2 arrive as the packed operands enc_fwd stored (4 + 2 k-blocks of 8 bf16 per lane)
    constexpr bool HPK = PREC == PREC_BF16;
    struct RowIn { f32x4 dml[2], h2[HPK ? 1 : H2T], h1[HPK ? 1 : H1T]; BfOp h2p[HPK ? 2 : 1], h1p[HPK ? 4 : 1]; };
    auto fetch_rows = [&](int tile, int p, RowIn& R) {
        const long row0 = (long)tile * TILE_ROWS;
        const int lrow = w * 16 + c;
        if (a.lp == 16) {
            R.dml[0] = ld_rows(rows_rsrc(a.dmean[p], row0, a.B, 16), lrow, 16, 4 * q);
            R.dml[1] = ld_rows(rows_rsrc(a.dlogvar[p], row0, a.B, 16), lrow, 16, 4 * q);
        } else {
            const long row = row0 + lrow;
            R.dml[0] = ld_tile<false>(a.dmean[p], row, a.L, 4 * q, a.L, row < a.B);
            R.dml[1] = ld_tile<false>(a.dlogvar[p], row, a.L, 4 * q, a.L, row < a.B);
        }
        if (HPK) {
            const __amdgpu_buffer_rsrc_t rp2 = rows_rsrc(a.h2[p], row0, a.B, 32), rp1 = rows_rsrc(a.h1[p], row0, a.B, 64);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                R.h2p[kb].hi = __builtin_bit_cast(bf16x8, ld_rows(rp2, lrow, 32, 16 * kb + 4 * q));
                R.h2p[kb].lo = R.h2p[kb].hi;
            }
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                R.h1p[kb].hi = __builtin_bit_cast(bf16x8, ld_rows(rp1, lrow, 64, 16 * kb + 4 * q));
                R.h1p[kb].lo = R.h1p[kb].hi;
            }
            return;
        }
        const __amdgpu_buffer_rsrc_t rh2 = rows_rsrc(a.h2[p], row0, a.B, H2P), rh1 = rows_rsrc(a.h1[p], row0, a.B, H1P);
#pragma unroll
        for (int t = 0; t < H2T; ++t) R.h2[t] = ld_rows(rh2, lrow, H2P, 16 * t + 4 * q);
#pragma unroll
        for (int t = 0; t < H1T; ++t) R.h1[t] = ld_rows(rh1, lrow, H1P, 16 * t + 4 * q);
    };
    // (small-batch shape only: the 8-wave kernel sits at its 256-register limit and would spill the extra copy)
    constexpr bool HOIST = NW == 4;
    RowIn Rpre;
    bool have_pre = false;
    if (HOIST && (int)blockIdx.x < a.ntiles) {
        fetch_rows(blockIdx.x, p_lo, Rpre);
        have_pre = true;
    }
    load_image<(NW == 8 ? 5 : 10)>(lds, a.img + im.oW2, nW);
    for (int i = threadIdx.x; i < NW * 128; i += NTHR) db1s[i] = 0.f;
    __syncthreads();
    int sb[4];  // per-lane element offsets of the staging writes (tile 0); tiles add a compile-time constant
    stage_bases<CH>(sb, 16 * w, c, q);

    f32x4 acc1[OWN][H1T], acc2[OWN][H2T], acc3[OWN], dbacc[H1T];
#pragma unroll
    for (int i = 0; i < H1T; ++i) dbacc[i] = zero4();
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
        acc3[o] = zero4();
#pragma unroll
        for (int i = 0; i < H1T; ++i) acc1[o][i] = zero4();
#pragma unroll
        for (int i = 0; i < H2T; ++i) acc2[o][i] = zero4();
    }

    // layer-1 input features of this lane as B-fragment columns (owned in tiles w + NW o)
    const int din = AUG ? 2 * a.d : a.d;
    bool fx[OWN], fm[OWN];
    int colB[OWN];
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
        const int fB = 16 * (w + NW * o) + c;
        fx[o] = fB < a.d; fm[o] = AUG && fB >= a.d && fB < din;  // x * mask column / appended mask column
        colB[o] = fx[o] ? fB : (fm[o] ? fB - a.d : 0);
    }

    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long row0 = (long)tile * TILE_ROWS;
        for (int p = p_lo; p < p_hi; ++p) {
            int cc = c, qq = q;
            launder(cc, qq);
            VPC_STAMP(0);
            // B fragments of slice s (batch rows row0 + 16 s + 4 q + j): raw x and mask bytes; rows past B read row 0
            // (their dh1 is exactly zero), columns past the input width are cleared when the fragment is formed
            // range-checked buffer loads relative to the tile's first row: a row past B is out of range and reads 0 (x and
            // mask byte), so no clamp; per load one 32-bit add of the slice offset to a per-lane base (the range check
            // covers voffset only, so the slice offset must not go into soffset).  Formed from the laundered lane id:
            // hipcc otherwise precomputes all 32 addresses per tile and spills them.
            const __amdgpu_buffer_rsrc_t rx = rows_rsrc(a.x, row0, a.B, a.d);
            const long mrem = (a.B - row0) * (long)a.d;
            const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t*>(a.mask[p]) + row0 * a.d, 0, mrem > 0xffffffffL ? 0xffffffffu : (uint32_t)mrem, 0x00020000);
            auto ld_xb = [&](int o, int sl, f32x4& xv, uint32_t& mb) {
                const int vo0 = 4 * qq * a.d + colB[o];  // element offset of (row 4 q, this lane's column)
                mb = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int off = vo0 + (16 * sl + j) * a.d;
                    xv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, 4 * off, 0, 0));
                    mb |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rm, off, 0, 0) << (8 * j);
                }
            };
            // fp32 engine: the four mask bytes stay in their own registers until the fragment is formed.  Packing them into
            // one word where they are requested (ld_xb) is VALU on the loaded values in front of the MFMAs the loads are
            // meant to run under (hipcc waits for every slice's mask bytes right behind their request), and five
            // instructions per slice where the unpacked form needs four.
            auto ld_xr = [&](int o, int sl, f32x4& xv, uint32_t (&mr)[4]) {
                const int vo0 = 4 * qq * a.d + colB[o];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int off = vo0 + (16 * sl + j) * a.d;
                    xv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, 4 * off, 0, 0));
                    mr[j] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rm, off, 0, 0);
                }
            };
            auto mk_fr = [&](int o, const f32x4& xv, const uint32_t (&mr)[4]) -> f32x4 {
                const uint32_t k = (AUG || fx[o]) ? 0xffu : 0u;  // columns past the input width: mask 0
                const f32x4 m = {(float)(mr[0] & k), (float)(mr[1] & k), (float)(mr[2] & k), (float)(mr[3] & k)};
                if (!AUG) return xv * m;
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fx[o] ? xv[j] * m[j] : (fm[o] ? m[j] : 0.f);
                return v;
            };
            auto mk_fb = [&](int o, const f32x4& xv, uint32_t mb) -> f32x4 {
                if (!AUG) return xv * mask_to_f32(mb & (fx[o] ? 0xffffffffu : 0u));  // columns past the input width: mask 0
                const f32x4 m = mask_to_f32(mb);
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fx[o] ? xv[j] * m[j] : (fm[o] ? m[j] : 0.f);
                return v;
            };
            RowIn R;
            if (HOIST && have_pre) R = Rpre; else fetch_rows(tile, p, R);
            have_pre = false;
            f32x4 (&dml)[2] = R.dml;
            auto& h2 = R.h2;
            auto& h1 = R.h1;
            // ReLU gate of tile mt from the fp32 tile or, packed form, from the bf16 halves of its operand (relu output >= +0:
            // positive <=> the 16 bits are not zero)
            auto gate_h2 = [&](int mt, f32x4 acc) { return HPK ? bf_gate(acc, R.h2p[HPK ? mt >> 1 : 0], mt & 1) : gate4(acc, h2[HPK ? 0 : mt]); };
            auto gate_h1 = [&](int mt, f32x4 acc) { return HPK ? bf_gate(acc, R.h1p[HPK ? mt >> 1 : 0], mt & 1) : gate4(acc, h1[HPK ? 0 : mt]); };
            // (dW3~ += dml * h2^T is staged and computed together with the layer-1 wgrad below: the B staging buffer is
            // free in that round because x never goes through LDS - 4 instead of 6 barriers per pass)
            VPC_STAMP(1);
            // ---- dh2 = relu'(h2) * (W3~^T dml)
            launder(cc, qq);
            f32x4 dh2[H2T];
            BfOp dmlb[1], dh2b[2];  // bf16 engine: packed once, used by the dgrad MFMAs AND the wgrad staging writes
            if (BF) dmlb[0] = bf_pack<PREC>(dml[0], dml[1]);
            uint32_t tj[4], tv[4];
            if (LB) fragT_bases<64>(tj, tv, W3, cc, qq);
#pragma unroll
            for (int mt = 0; mt < H2T; ++mt) {
                if (LB) dh2[mt] = gate4(tile_T_b<2, 64>(tj, tv, mt, dml, zero4()), h2[mt]);
                else if (PREC == PREC_F32) dh2[mt] = gate4(tile_T<2, 64>(W3, mt, dml, zero4(), cc, qq), h2[mt]);
                else dh2[mt] = gate_h2(mt, bf_tile_T<PREC, 1, 64>(W3, mt, dmlb, zero4(), 16 * qq + cc));
            }
            if (BF) bf_acts<PREC, H2T>(dh2, dh2b);
            VPC_STAMP(2);
            // ---- dW2~ += dh2 * h1^T   (owner: wave w -> in tiles w + NW o < 7, all 4 out tiles)
            launder(cc, qq);
            // staging fragments: bases of tile 0 of the A buffer and of this wave's own tile of the B buffer
            uint32_t sf[4], sfw[4];
            if (LB) {
                frag_bases<CH>(sf, stA, cc, qq);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    sfw[v] = sf[v] + (uint32_t)(OFF_B + ws * frag_imm(CH, 1, 0));
                    asm volatile("" : "+v"(sfw[v]));
                }
            }
            if (!ABLE(2)) lds_barrier();
            if (BF && !ABLE(1)) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) bf_stage_write_op<PREC, 7, H2T>(sAh, sAl, 16 * w + cc, kb, qq, dh2b[kb]);
                if (HPK) {
#pragma unroll
                    for (int kb = 0; kb < 4; ++kb) bf_stage_write_op<PREC, 7, H1T>(sBh, sBl, 16 * w + cc, kb, qq, R.h1p[kb]);
                } else {
#pragma unroll
                    for (int t = 0; t < H1T; ++t) bf_stage_write<PREC, 7>(sBh, sBl, 16 * w + cc, t, qq, h1[HPK ? 0 : t]);
                }
            } else if (!ABLE(1)) {
#pragma unroll
                for (int t = 0; t < H2T; ++t) stage_write_b<CH>(stA, t, dh2[t], sb);
#pragma unroll
                for (int t = 0; t < H1T; ++t) stage_write_b<CH>(stB, t, h1[t], sb);
            }
            if (!ABLE(2)) lds_barrier();
#pragma unroll
            for (int o = 0; o < OWN; ++o) {
                if (PREC != PREC_F32) {
                    if (ws + NW * o < H1T && !ABLE(4)) {
#pragma unroll
                        for (int kb = 0; kb < SKB; ++kb) {
                            asm volatile("" ::: "memory");
                            const BfOp fb = bf_stage_frag<PREC, 7>(sBh, sBl, w + NW * o, kb, 16 * qq + cc);
#pragma unroll
                            for (int mt = 0; mt < H2T; ++mt) {
                                const BfOp fa = bf_stage_frag<PREC, 7>(sAh, sAl, mt, kb, 16 * qq + cc);
                                acc2[o][mt] = bf_mma<PREC>(fa, fb, acc2[o][mt]);
                            }
                        }
                    }
                } else if (ws + NW * o < H1T && !ABLE(4)) {
#pragma unroll
                    for (int s = 0; s < CH / 16; ++s) {
                        asm volatile("" ::: "memory");
                        const f32x4 fb = LB ? frag_ld<CH>(sfw, 0, s) : stage_frag<CH>(stB, w + NW * o, s, cc, qq);
                        // A fragments double-buffered by hand (hipcc sinks each LDS read to its first use: one exposed
                        // LDS latency per 4 MFMAs); the sched_barrier pins the read of mt+1 above the MFMAs of mt
                        f32x4 fa = LB ? frag_ld<CH>(sf, 0, s) : stage_frag<CH>(stA, 0, s, cc, qq);
#pragma unroll
                        for (int mt = 0; mt < H2T; ++mt) {
                            const f32x4 fn = LB ? frag_ld<CH>(sf, mt + 1 < H2T ? mt + 1 : mt, s)
                                                : stage_frag<CH>(stA, mt + 1 < H2T ? mt + 1 : mt, s, cc, qq);
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc2[o][mt] = VPC_MFMA(fa[j], fb[j], acc2[o][mt]);
                            fa = fn;
                        }
                    }
                }
            }
            VPC_STAMP(3);
            // the first two B slices of the layer-1 wgrad come in under the dh1 MFMAs
            constexpr int NS = CH / 16;
            f32x4 xb[OWN][3];  // rotating: slices s, s + 1, s + 2
            uint32_t mbb[OWN][3];
            uint32_t mrr[OWN][3][4];  // fp32 engine: unpacked
#pragma unroll
            for (int o = 0; o < OWN; ++o)
                if (NW * (o + 1) <= DT || ws + NW * o < DT) {
                    if (PREC == PREC_F32) {
                        ld_xr(o, 0, xb[o][0], mrr[o][0]);
                        ld_xr(o, 1, xb[o][1], mrr[o][1]);
                    } else {
                        ld_xb(o, 0, xb[o][0], mbb[o][0]);
                        ld_xb(o, 1, xb[o][1], mbb[o][1]);
                        ld_xb(o, 2, xb[o][2], mbb[o][2]);  // bf16: slices are consumed in pairs
                    }
                }
            // ---- dh1 = relu'(h1) * (W2~^T dh2);  db1 += dh1
            launder(cc, qq);
            f32x4 dh1[H1T];
            // db1: per-lane running sums over all tile-passes; the cross-lane reduction happens ONCE, after the
            // loops (it used to be 4 DPP adds + a predicated ds_add per value and pass: ~170 VALU and 28 exec-masked
            // basic blocks in the middle of the dgrad MFMA stream)
            if (BF) {
                bf_layer_T<PREC, 2, 128, H1T, 4, 2>(W2, dh2b, 16 * qq + cc, [&](int mt, f32x4 acc) {
                    dh1[mt] = gate_h1(mt, acc);
                    dbacc[mt] += dh1[mt];
                });
            } else {
                // (not on lane bases: this phase is the kernel's register peak, and the 4 + 4 bases spill 116 B / lane)
#pragma unroll
                for (int mt = 0; mt < H1T; ++mt) {
                    dh1[mt] = gate4(tile_T<H2T, 128, NK2>(W2, mt, dh2, zero4(), cc, qq), h1[mt]);
                    dbacc[mt] += dh1[mt];
                }
            }
            VPC_STAMP(4);
            // ---- dW1 += dh1 * (x*mask)^T   (owner: wave w -> in tiles w + NW o < DT, all 7 out tiles; B straight from global)
            launder(cc, qq);
            // bases of tile 0 of the A buffer (dW1) and of this wave's two operand tiles of dW3 in the B buffer
            uint32_t s1[4], s3a[4], s3b[4];
            if (LB) {
                frag_bases<CH>(s1, stA, cc, qq);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    s3a[v] = s1[v] + (uint32_t)(OFF_B + (H2T + (ws >> 2)) * frag_imm(CH, 1, 0));
                    s3b[v] = s1[v] + (uint32_t)(OFF_B + (ws & 3) * frag_imm(CH, 1, 0));
                    asm volatile("" : "+v"(s3a[v]), "+v"(s3b[v]));
                }
            }
            if (!ABLE(2)) lds_barrier();
            if (BF && !ABLE(1)) {
#pragma unroll
                for (int t = 0; t < H1T; ++t) bf_stage_write<PREC, 7>(sAh, sAl, 16 * w + cc, t, qq, dh1[t]);
                if (HPK) {
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) bf_stage_write_op<PREC, 7, H2T>(sBh, sBl, 16 * w + cc, kb, qq, R.h2p[kb]);
                } else {
#pragma unroll
                    for (int t = 0; t < H2T; ++t) bf_stage_write<PREC, 7>(sBh, sBl, 16 * w + cc, t, qq, h2[HPK ? 0 : t]);
                }
                bf_stage_write_op<PREC, 7, 6>(sBh, sBl, 16 * w + cc, H2T / 2, qq, dmlb[0]);  // tiles 4, 5
            } else if (!ABLE(1)) {
#pragma unroll
                for (int t = 0; t < H1T; ++t) stage_write_b<CH>(stA, t, dh1[t], sb);
                // operands of dW3~ (tile t8 = w + NW o -> out tile t8 >> 2, in tile t8 & 3): h2 -> stB tiles 0..3, dml -> stB tiles 4, 5
#pragma unroll
                for (int t = 0; t < H2T; ++t) stage_write_b<CH>(stB, t, h2[t], sb);
                stage_write_b<CH>(stB, H2T, dml[0], sb);
                stage_write_b<CH>(stB, H2T + 1, dml[1], sb);
            }
            if (!ABLE(2)) lds_barrier();
#pragma unroll
            for (int o = 0; o < OWN; ++o) {
                const int t8 = w + NW * o;
                if (PREC == PREC_F32) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const f32x4 fa = LB ? frag_ld<CH>(s3a, 0, s) : stage_frag<CH>(stB, H2T + (t8 >> 2), s, cc, qq);
                        const f32x4 fb = LB ? frag_ld<CH>(s3b, 0, s) : stage_frag<CH>(stB, t8 & 3, s, cc, qq);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc3[o] = VPC_MFMA(fa[j], fb[j], acc3[o]);
                    }
                } else {
#pragma unroll
                    for (int kb = 0; kb < SKB; ++kb) {
                        const BfOp fa = bf_stage_frag<PREC, 7>(sBh, sBl, H2T + (t8 >> 2), kb, 16 * qq + cc);
                        const BfOp fb = bf_stage_frag<PREC, 7>(sBh, sBl, t8 & 3, kb, 16 * qq + cc);
                        acc3[o] = bf_mma<PREC>(fa, fb, acc3[o]);
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < OWN; ++o) {
                if (PREC != PREC_F32) {
                    if (NW * (o + 1) <= DT || ws + NW * o < DT) {
                        // slices in pairs (one 32-row k-block per MFMA); ring of 4 slices: block sb2 + 1 in flight
                        f32x4 xq[4] = {xb[o][0], xb[o][1], xb[o][2], zero4()};
                        uint32_t mq[4] = {mbb[o][0], mbb[o][1], mbb[o][2], 0u};
                        if (3 < NS) ld_xb(o, 3, xq[3], mq[3]);
#pragma unroll
                        for (int sb2 = 0; sb2 < NS / 2; ++sb2) {
                            asm volatile("" ::: "memory");
                            const BfOp fb = bf_pack<PREC>(mk_fb(o, xq[(2 * sb2) & 3], mq[(2 * sb2) & 3]),
                                                          mk_fb(o, xq[(2 * sb2 + 1) & 3], mq[(2 * sb2 + 1) & 3]));
                            if (2 * sb2 + 4 < NS) ld_xb(o, 2 * sb2 + 4, xq[(2 * sb2) & 3], mq[(2 * sb2) & 3]);
                            if (2 * sb2 + 5 < NS) ld_xb(o, 2 * sb2 + 5, xq[(2 * sb2 + 1) & 3], mq[(2 * sb2 + 1) & 3]);
#pragma unroll
                            for (int mt = 0; mt < H1T; ++mt) {
                                const BfOp fa = bf_stage_frag<PREC, 7>(sAh, sAl, mt, sb2, 16 * qq + cc);
                                acc1[o][mt] = bf_mma<PREC>(fa, fb, acc1[o][mt]);
                            }
                        }
                    }
                } else if ((NW * (o + 1) <= DT || ws + NW * o < DT) && !ABLE(4)) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        asm volatile("" ::: "memory");  // keep each slice's loads in its slice (hipcc hoists all 8 otherwise)
                        if (s + 2 < NS) ld_xr(o, s + 2, xb[o][(s + 2) % 3], mrr[o][(s + 2) % 3]);
                        const f32x4 fb = mk_fr(o, xb[o][s % 3], mrr[o][s % 3]);
                        f32x4 fa = LB ? frag_ld<CH>(s1, 0, s) : stage_frag<CH>(stA, 0, s, cc, qq);
#pragma unroll
                        for (int mt = 0; mt < H1T; ++mt) {
                            const f32x4 fn = LB ? frag_ld<CH>(s1, mt + 1 < H1T ? mt + 1 : mt, s)
                                                : stage_frag<CH>(stA, mt + 1 < H1T ? mt + 1 : mt, s, cc, qq);
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc1[o][mt] = VPC_MFMA(fa[j], fb[j], acc1[o][mt]);
                            fa = fn;
                        }
                    }
                }
            }
            VPC_STAMP(5);
        }
    }
    // ---- db1 = sum of dh1 over this wave's 16 rows (lanes c): DPP butterfly inside each 16-lane row, then the c == 0
    // lanes own one (wave, feature) slot each - plain stores, fixed order, bit-reproducible
#pragma unroll
    for (int mt = 0; mt < H1T; ++mt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = dbacc[mt][j];
            v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
            v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
            v += dpp_mov<0x141>(v);  // row_half_mirror
            v += dpp_mov<0x140>(v);  // row_mirror: every lane of the 16-lane row holds the row sum
            if (c == 0) db1s[w * 128 + 16 * mt + 4 * q + j] = v;
        }
    // ---- write this workgroup's gradient partial block (8-wave slot layout: owned slice o is "wave" w + NW o)
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
        float* part = a.part + blk * ENC_PART + (long)(w + NW * o) * GREGS * 64 + lane;
#pragma unroll
        for (int mt = 0; mt < H1T; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[(4 * mt + j) * 64] = acc1[o][mt][j];
#pragma unroll
        for (int mt = 0; mt < H2T; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[(28 + 4 * mt + j) * 64] = acc2[o][mt][j];
#pragma unroll
        for (int j = 0; j < 4; ++j) part[(44 + j) * 64] = acc3[o][j];
    }
    __syncthreads();  // every wave's db1s row is complete
    if (threadIdx.x < 128) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < NW; ++k) t += db1s[k * 128 + threadIdx.x];
        a.part[blk * ENC_PART + WAVES * GREGS * 64 + threadIdx.x] = t;
    }
#ifdef VPC_ABLATE
    VPC_STAMP(6);
    if (ABLE(64) && blockIdx.x == 100 && (threadIdx.x & 63) == 0 && (threadIdx.x >> 6) % 3 == 0)
        printf("enc_bwd blk %d wave %d cycles: top %llu loads %llu dh2 %llu dW2 %llu dh1 %llu dW1+dW3 %llu epilogue %llu\n",
               blockIdx.x, (int)(threadIdx.x >> 6), T[0], T[1], T[2], T[3], T[4], T[5], T[6]);
#endif
