// The backward kernel of the small-batch MIWAE step (vpc_miw_small.hip): the BODY of miw_small_bwd_kernel<YT, LT> and of its
// ensemble form miw_small_bwd_multi_kernel<YT, LT>, included as text (see vpc_miw_small_fwd_body.h).  In scope: `a` (a
// MiwSmallArgs), YT, LT and the macros MIW_BLK / MIW_NBLK: workgroup MIW_BLK of MIW_NBLK walks the row blocks MIW_BLK,
// MIW_BLK + MIW_NBLK, .. and writes partial block MIW_BLK of a.part.
// (No include guard: a code fragment, included once per kernel.)
    constexpr int DT = YT <= 3 ? 1 : 2;
    __shared__ __attribute__((aligned(16))) float lds[K_COUNT * SBUF];
    auto buf = [&](int b) { return lds + b * SBUF; };
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int tid = threadIdx.x;
    const int d = a.d, L = a.L, S = a.S;
    const MiwOff o(d, L);
    const float* P = a.prm;
    float* part = a.part + (long)MIW_BLK * o.n;
    int cc = c, qq = q;
    // ================================================================ first loop: decoder side
    // wave w: dWx in-tile w x YT out tiles, dWd2 in-tile w x 8 out tiles, dWd1 out tile w; thread t: one bias column
    // (t < 128: bd2, 128 <= t < 256: bd1, 256 <= t < 256 + 3 d: bx)
    {
        f32x4 accX[YT], acc2[8], acc1 = zero4();
#pragma unroll
        for (int t = 0; t < YT; ++t) accX[t] = zero4();
#pragma unroll
        for (int t = 0; t < 8; ++t) acc2[t] = zero4();
        float db = 0.f;
        for (int u = MIW_BLK; u < a.units; u += MIW_NBLK) {
            const long r0 = (long)u * a.RB;
            const int nr = a.R - r0 < a.RB ? (int)(a.R - r0) : a.RB;
            const int nrows = nr * S;
            const long drow0 = r0 * S;
            // thread (rb, l) of wave 0: the row's encoder-head gradient, from the loss's own term on (miw_sample_bwd_kernel)
            const int rb = tid >> 4, hl = tid & 15;
            const bool hown = rb < nr && hl < L;
            float gm = hown ? a.gh[(r0 + rb) * 2 * L + hl] : 0.f;
            float gs = hown ? a.gh[(r0 + rb) * 2 * L + L + hl] : 0.f;
            // the operands of a tile are requested one tile ahead (registers pG / p2 / p1 / pz / pe) and written to LDS at the top
            // of their tile: G [16][16 YT], g2, g1 [16][128]; z and the sampling eps as tiles 0 and 3 of K_Z (dz is tile 2)
            constexpr int NG = (256 * YT + THREADS - 1) / THREADS;
            float pG[NG], pz = 0.f, pe = 0.f;
            f32x4 p2 = zero4(), p1 = zero4();
            const int sr = tid >> 5, sf = 4 * (tid & 31), zr = tid >> 4;
            auto fetch = [&](int t0) {
                const int nl = nrows - t0 < 16 ? nrows - t0 : 16;
                const long row0 = drow0 + t0;
#pragma unroll
                for (int k = 0; k < NG; ++k) {
                    const int i = tid + k * THREADS, r = i / (16 * YT), f = i - r * 16 * YT;
                    pG[k] = (i < 256 * YT && r < nl && f < 3 * d) ? a.G[(row0 + r) * 3 * d + f] : 0.f;
                }
                p2 = sr < nl ? *reinterpret_cast<const f32x4*>(a.g2 + (row0 + sr) * MIW_HID + sf) : zero4();
                p1 = sr < nl ? *reinterpret_cast<const f32x4*>(a.g1 + (row0 + sr) * MIW_HID + sf) : zero4();
                const bool zok = tid < 256 && zr < nl && hl < L;
                pz = zok ? a.z[(row0 + zr) * L + hl] : 0.f;
                pe = zok ? a.eps[(row0 + zr) * L + hl] : 0.f;
            };
            auto commit = [&]() {
#pragma unroll
                for (int k = 0; k < NG; ++k) {
                    const int i = tid + k * THREADS, r = i / (16 * YT), f = i - r * 16 * YT;
                    if (i < 256 * YT) buf(K_DP)[r * SP + f] = pG[k];
                }
                *reinterpret_cast<f32x4*>(buf(K_A2) + sr * SP + sf) = p2;
                *reinterpret_cast<f32x4*>(buf(K_A1) + sr * SP + sf) = p1;
                if (tid < 256) {
                    buf(K_Z)[zr * SP + hl] = pz;
                    buf(K_Z)[zr * SP + 48 + hl] = pe;
                }
            };
            fetch(0);
            f32x4 fT6[YT];  // (the first stage's fragments: requested behind their last use, for the next tile)
            miw_ldAT<YT>(P + o.Wx, 3 * d, MIW_HID, w, cc, qq, fT6);
            for (int t0 = 0; t0 < nrows; t0 += 16) {
                const int nl = nrows - t0 < 16 ? nrows - t0 : 16;
                f32x4 fT5[8], fT4[8];
                commit();
                lds_barrier();
                launder(cc, qq);
                if (t0 + 16 < nrows) fetch(t0 + 16);
                // ---- dWx | dg2 = relu'(g2) (Wx^T G) | bx
                miw_ldAT<8>(P + o.Wd2, MIW_HID, MIW_HID, w, cc, qq, fT5);
#pragma unroll
                for (int mt = 0; mt < YT; ++mt) accX[mt] = wgrad16(buf(K_DP), mt, buf(K_A2), w, accX[mt], cc, qq);
                st_act(buf(K_DA2), w, cc, qq, gate4(miw_mm<YT>(fT6, buf(K_DP), cc, qq, zero4()), ld_act(buf(K_A2), w, cc, qq)));
                if (tid >= 256 && tid < 256 + 3 * d) db += miw_colsum(buf(K_DP), tid - 256);
                lds_barrier();
                launder(cc, qq);
                // ---- dWd2 | dg1 | bd2
                if (w == 0) miw_ldAT<8>(P + o.Wd1, MIW_HID, L, 0, cc, qq, fT4);
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) acc2[mt] = wgrad16(buf(K_DA2), mt, buf(K_A1), w, acc2[mt], cc, qq);
                st_act(buf(K_DA1), w, cc, qq, gate4(miw_mm<8>(fT5, buf(K_DA2), cc, qq, zero4()), ld_act(buf(K_A1), w, cc, qq)));
                if (tid < 128) db += miw_colsum(buf(K_DA2), tid);
                lds_barrier();
                launder(cc, qq);
                // ---- dWd1 | dz (wave 0, into tile 2 of K_Z) | bd1
                if (t0 + 16 < nrows) miw_ldAT<YT>(P + o.Wx, 3 * d, MIW_HID, w, cc, qq, fT6);
                acc1 = wgrad16(buf(K_DA1), w, buf(K_Z), 0, acc1, cc, qq);
                if (w == 0) st_act(buf(K_Z), 2, cc, qq, miw_mm<8>(fT4, buf(K_DA1), cc, qq, zero4()));
                if (tid >= 128 && tid < 256) db += miw_colsum(buf(K_DA1), tid - 128);
                lds_barrier();
                launder(cc, qq);
                // ---- sum over the row's samples, in sample order: rows [lo, hi) of the tile are samples of data row rb
                if (hown) {
                    const int lo = rb * S - t0 > 0 ? rb * S - t0 : 0, hi = (rb + 1) * S - t0 < nl ? (rb + 1) * S - t0 : nl;
                    for (int r = lo; r < hi; ++r) {
                        const float dzv = buf(K_Z)[r * SP + 32 + hl];
                        gm += dzv;
                        gs += dzv * buf(K_Z)[r * SP + 48 + hl];
                    }
                }
                lds_barrier();  // the next tile's operands overwrite what this stage and the last one read
                launder(cc, qq);
            }
            if (hown) {
                a.dht[(r0 + rb) * 2 * L + hl] = gm;
                a.dht[(r0 + rb) * 2 * L + L + hl] = gs * miw_softplus_d(a.heads[(r0 + rb) * 2 * L + L + hl]);
            }
        }
#pragma unroll
        for (int mt = 0; mt < YT; ++mt) miw_put(part + o.Wx, 3 * d, MIW_HID, mt, w, c, q, accX[mt]);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) miw_put(part + o.Wd2, MIW_HID, MIW_HID, mt, w, c, q, acc2[mt]);
        miw_put(part + o.Wd1, MIW_HID, L, w, 0, c, q, acc1);
        if (tid < 128) part[o.bd2 + tid] = db;
        else if (tid < 256) part[o.bd1 + tid - 128] = db;
        else if (tid < 256 + 3 * d) part[o.bx + tid - 256] = db;
    }
    __syncthreads();  // dht of this workgroup's rows is in memory; every LDS buffer is free
    launder(cc, qq);
    // ================================================================ second loop: encoder side, the same row blocks
    // wave w: dWh in-tile w x LT out tiles, dWe2 in-tile w x 8 out tiles, dWe1 out tile w x DT in tiles; thread t: one bias
    // column (t < 128: be2, 128 <= t < 256: be1, 256 <= t < 256 + 2 L: bh)
    {
        f32x4 accH[LT], acc2[8], acc1[DT];
#pragma unroll
        for (int t = 0; t < LT; ++t) accH[t] = zero4();
#pragma unroll
        for (int t = 0; t < 8; ++t) acc2[t] = zero4();
#pragma unroll
        for (int t = 0; t < DT; ++t) acc1[t] = zero4();
        float db = 0.f;
        for (int u = MIW_BLK; u < a.units; u += MIW_NBLK) {
            const long r0 = (long)u * a.RB;
            const int nr = a.R - r0 < a.RB ? (int)(a.R - r0) : a.RB;
            f32x4 fT3[LT], fT2[8];
            miw_ldAT<LT>(P + o.Wh, 2 * L, MIW_HID, w, cc, qq, fT3);
            miw_stage(buf(K_DP), a.dht, r0, nr, 2 * L, LT);
            miw_stage128(buf(K_A2), a.h2, r0, nr);
            miw_stage128(buf(K_A1), a.h1, r0, nr);
            miw_stage(buf(K_Z), a.xin, r0, nr, d, DT);
            lds_barrier();
            launder(cc, qq);
            // ---- dWh | dh2 | bh
            miw_ldAT<8>(P + o.We2, MIW_HID, MIW_HID, w, cc, qq, fT2);
#pragma unroll
            for (int mt = 0; mt < LT; ++mt) accH[mt] = wgrad16(buf(K_DP), mt, buf(K_A2), w, accH[mt], cc, qq);
            st_act(buf(K_DA2), w, cc, qq, gate4(miw_mm<LT>(fT3, buf(K_DP), cc, qq, zero4()), ld_act(buf(K_A2), w, cc, qq)));
            if (tid >= 256 && tid < 256 + 2 * L) db += miw_colsum(buf(K_DP), tid - 256);
            lds_barrier();
            launder(cc, qq);
            // ---- dWe2 | dh1 | be2
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) acc2[mt] = wgrad16(buf(K_DA2), mt, buf(K_A1), w, acc2[mt], cc, qq);
            st_act(buf(K_DA1), w, cc, qq, gate4(miw_mm<8>(fT2, buf(K_DA2), cc, qq, zero4()), ld_act(buf(K_A1), w, cc, qq)));
            if (tid < 128) db += miw_colsum(buf(K_DA2), tid);
            lds_barrier();
            launder(cc, qq);
            // ---- dWe1 | be1
#pragma unroll
            for (int t = 0; t < DT; ++t) acc1[t] = wgrad16(buf(K_DA1), w, buf(K_Z), t, acc1[t], cc, qq);
            if (tid >= 128 && tid < 256) db += miw_colsum(buf(K_DA1), tid - 128);
            lds_barrier();  // the next row block stages into the buffers read above
            launder(cc, qq);
        }
#pragma unroll
        for (int mt = 0; mt < LT; ++mt) miw_put(part + o.Wh, 2 * L, MIW_HID, mt, w, c, q, accH[mt]);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) miw_put(part + o.We2, MIW_HID, MIW_HID, mt, w, c, q, acc2[mt]);
#pragma unroll
        for (int t = 0; t < DT; ++t) miw_put(part + o.We1, MIW_HID, d, w, t, c, q, acc1[t]);
        if (tid < 128) part[o.be2 + tid] = db;
        else if (tid < 256) part[o.be1 + tid - 128] = db;
        else if (tid < 256 + 2 * L) part[o.bh + tid - 256] = db;
    }
