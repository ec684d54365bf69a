// The forward kernel of the small-batch MIWAE step (vpc_miw_small.hip): the BODY of miw_small_fwd_kernel<YT, LT> and of its
// ensemble form miw_small_fwd_multi_kernel<YT, LT>, included as text so that the stand-alone kernel compiles to the
// instructions it had with these lines spelled out in it.  In scope at the point of inclusion: `a` (a MiwSmallArgs: the kernel
// argument, or member g's record built in registers), YT, LT and the macro MIW_BLK = the row block of this workgroup.
// (No include guard: a code fragment, included once per kernel.)
    constexpr int DT = YT <= 3 ? 1 : 2;
    __shared__ __attribute__((aligned(16))) float lds[F_COUNT * SBUF];
    auto buf = [&](int b) { return lds + b * SBUF; };
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int d = a.d, L = a.L, S = a.S;
    const MiwOff o(d, L);
    const float* P = a.prm;
    const long r0 = (long)MIW_BLK * a.RB;
    const int nr = a.R - r0 < a.RB ? (int)(a.R - r0) : a.RB;
    int cc = c, qq = q;
    // ================================================================ encoder: one tile, rows past nr dead
    f32x4 fW1[DT], fW2[8], fW3[8];
    miw_ldA<DT>(P + o.We1, MIW_HID, d, w, cc, qq, fW1);
    miw_stage(buf(F_X), a.xin, r0, nr, d, DT);
    miw_ldA<8>(P + o.We2, MIW_HID, MIW_HID, w, cc, qq, fW2);
    lds_barrier();
    launder(cc, qq);
    {
        const f32x4 v = relu4(miw_mm<DT>(fW1, buf(F_X), cc, qq, miw_bias(P + o.be1, MIW_HID, w, qq)));
        st_act(buf(F_H1), w, cc, qq, v);
        if (cc < nr) *reinterpret_cast<f32x4*>(a.h1 + (r0 + cc) * MIW_HID + 16 * w + 4 * qq) = v;
    }
    if (w < LT) miw_ldA<8>(P + o.Wh, 2 * L, MIW_HID, w, cc, qq, fW3);
    lds_barrier();
    launder(cc, qq);
    {
        const f32x4 v = relu4(miw_mm<8>(fW2, buf(F_H1), cc, qq, miw_bias(P + o.be2, MIW_HID, w, qq)));
        st_act(buf(F_H2), w, cc, qq, v);
        if (cc < nr) *reinterpret_cast<f32x4*>(a.h2 + (r0 + cc) * MIW_HID + 16 * w + 4 * qq) = v;
    }
    // the decoder's fragments do not change from tile to tile: requested once, here
    f32x4 fW4[1], fW5[8], fW6[8];
    miw_ldA<1>(P + o.Wd1, MIW_HID, L, w, cc, qq, fW4);
    miw_ldA<8>(P + o.Wd2, MIW_HID, MIW_HID, w, cc, qq, fW5);
    if (w < YT) miw_ldA<8>(P + o.Wx, 3 * d, MIW_HID, w, cc, qq, fW6);
    const f32x4 bias4 = miw_bias(P + o.bd1, MIW_HID, w, qq), bias5 = miw_bias(P + o.bd2, MIW_HID, w, qq);
    const f32x4 bias6 = miw_bias(P + o.bx, 3 * d, w < YT ? w : 0, qq);
    lds_barrier();
    launder(cc, qq);
    if (w < LT) {  // heads: raw to the workspace, (mean | softplus(raw)) to the workspace and to LDS for the sampler
        const f32x4 v = miw_mm<8>(fW3, buf(F_H2), cc, qq, miw_bias(P + o.bh, 2 * L, w, qq));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = 16 * w + 4 * qq + j;
            const float act = f < L ? v[j] : miw_softplus(v[j]);
            buf(F_HD)[cc * SP + f] = act;
            if (cc < nr && f < 2 * L) {
                a.heads[(r0 + cc) * 2 * L + f] = v[j];
                a.hact[(r0 + cc) * 2 * L + f] = act;
            }
        }
    }
    lds_barrier();
    launder(cc, qq);
    // ================================================================ decoder: the nr S rows r0 S .. in tiles of 16
    const int nrows = nr * S;
    const long drow0 = r0 * S;
    const int zr = threadIdx.x >> 4, zl = threadIdx.x & 15;
    auto eps_of = [&](int t0) {  // this thread's draw of the tile at t0: requested one tile ahead
        return (threadIdx.x < 256 && t0 + zr < nrows && zl < L) ? a.eps[(drow0 + t0 + zr) * L + zl] : 0.f;
    };
    float e_next = eps_of(0);
    for (int t0 = 0; t0 < nrows; t0 += 16) {
        if (threadIdx.x < 256) {  // z = mean + eps * scale (miw_sample_kernel), columns past L and dead rows 0
            const int row = t0 + zr;
            float zv = 0.f;
            if (row < nrows && zl < L) {
                const int b = row / S;
                const float mu = buf(F_HD)[b * SP + zl], sc = buf(F_HD)[b * SP + L + zl];
                zv = mu + e_next * sc;
                a.z[(drow0 + row) * L + zl] = zv;
            }
            buf(F_Z)[zr * SP + zl] = zv;
        }
        lds_barrier();
        launder(cc, qq);
        e_next = eps_of(t0 + 16);
        const bool live = t0 + cc < nrows;
        const long grow = drow0 + t0 + cc;
        {
            const f32x4 v = relu4(miw_mm<1>(fW4, buf(F_Z), cc, qq, bias4));
            st_act(buf(F_G1), w, cc, qq, v);
            if (live) *reinterpret_cast<f32x4*>(a.g1 + grow * MIW_HID + 16 * w + 4 * qq) = v;
        }
        lds_barrier();
        launder(cc, qq);
        {
            const f32x4 v = relu4(miw_mm<8>(fW5, buf(F_G1), cc, qq, bias5));
            st_act(buf(F_G2), w, cc, qq, v);
            if (live) *reinterpret_cast<f32x4*>(a.g2 + grow * MIW_HID + 16 * w + 4 * qq) = v;
        }
        lds_barrier();
        launder(cc, qq);
        if (w < YT) {
            const f32x4 v = miw_mm<8>(fW6, buf(F_G2), cc, qq, bias6);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = 16 * w + 4 * qq + j;
                if (live && f < 3 * d) a.Y[grow * 3 * d + f] = v[j];
            }
        }
        // (no barrier: the next tile's first write to a buffer lies behind a barrier every reader of this tile has passed)
    }
