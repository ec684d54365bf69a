// The body of rows_bwd_kernel and rows_bwd_multi_kernel (vpc_rows.hip), included as text for the reason given in
// vpc_rows_fwd_body.h.  In scope: `a` (RowsBwdArgs), the template flags VN / VK, and the macro ROWS_BX = the workgroup's index
// in the layer's 1-D grid (weight-gradient workgroups first, then the data-gradient slabs).  (No include guard.)
    __shared__ f32x4 red[ROWS_WAVES][ROWS_RT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    if ((int)ROWS_BX < a.wg_blocks) {  // ---- weight gradient: unit = (slab of 16 features, group of 64 columns) per wave
        const int unit = ROWS_WG_UNITS * ROWS_BX + wave;
        if (wave >= ROWS_WG_UNITS || unit >= a.wg_units) return;
        const int ng = (a.K + 63) / 64;
        rows_wgrad_unit<VK>(a, unit / ng, unit % ng, c, q);
        return;
    }
    // ---- data gradient: slab of 16 input features x 32 rows, the waves split the contraction over N
    const int b = ROWS_BX - a.wg_blocks, nsk = (a.K + 15) / 16;
    const int kf0 = 16 * (b % nsk), m0 = 16 * ROWS_RT * (b / nsk);
    const int nrt = min(ROWS_RT, (a.M - m0 + 15) / 16);
    const int nchunk = (a.N + 15) / 16;
    const int kf = kf0 + c;
    const bool kf_ok = kf < a.K;
    f32x4 acc[ROWS_RT];
#pragma unroll
    for (int rt = 0; rt < ROWS_RT; ++rt) acc[rt] = zero4();
    // lane (c, q): A = W[16 ch + 4 q + j][kf0 + c], B = dY~[m0 + 16 rt + c][16 ch + 4 q + j] in k-step j of chunk ch
    act_dispatch(a.gate, [&](auto gc) {
        constexpr int G = decltype(gc)::value;
        rows_slab<(G == ACT_NONE ? ROWS_GROUP : ROWS_GROUP / 2)>(nrt, nchunk, wave,
                  [&](int ch) { return rows_ld4_col(a.w, a.K, 16 * ch + 4 * q, a.N, kf, kf_ok); },
                  [&](int ch, int rt) {
                      const int n = 16 * ch + 4 * q, row = m0 + 16 * rt + c;
                      const int nv = row < a.M ? a.N - n : 0;
                      f32x4 d = rows_ld4<VN>(a.dy, (long)row * a.lddy + n, nv);
                      if (G != ACT_NONE) {
                          const f32x4 y = rows_ld4<VN>(a.yg, (long)row * a.ldyg + n, nv);
#pragma unroll
                          for (int j = 0; j < 4; ++j) d[j] *= act_grad<G>(y[j], n + j >= a.gate_split);
                      }
                      return d;
                  }, acc);
    });
#pragma unroll
    for (int rt = 0; rt < ROWS_RT; ++rt) red[wave][rt][lane] = acc[rt];
    __syncthreads();
    // wave rt: s[e] = (dY~ W)[m0 + 16 rt + c][kf0 + 4 q + e]
    if (wave >= nrt) return;
    f32x4 v = rows_sum(red, min(ROWS_WAVES, nchunk), wave, lane);
    const int f = kf0 + 4 * q, row = m0 + 16 * wave + c;
    if (f >= a.K || row >= a.M) return;
    const bool full4 = f + 3 < a.K;
    if (a.xo) {
        const float* px = a.xo + (long)row * a.ldxo + f;
        f32x4 xo = zero4();
        if (a.vecXo && full4) {
            xo = *reinterpret_cast<const f32x4*>(px);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (f + e < a.K) xo[e] = px[e];
        }
        act_dispatch(a.act_prev, [&](auto actc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= act_grad<decltype(actc)::value>(xo[e], false);
        });
    }
    float* pd = a.dx + (long)row * a.lddx + f;
    if (a.vecDx && full4) {
        *reinterpret_cast<f32x4*>(pd) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (f + e < a.K) pd[e] = v[e];
    }
