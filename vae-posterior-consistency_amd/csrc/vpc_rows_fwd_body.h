// The body of rows_fwd_kernel and rows_fwd_multi_kernel (vpc_rows.hip), included as text so that both kernels are one piece of
// code and the stand-alone kernel compiles to the instructions it had with these lines spelled out in it.
// In scope at the point of inclusion: `a` (RowsFwdArgs: this workgroup's operands), the template flag VEC, and the macros
// ROWS_BX / ROWS_BY = the workgroup's 16-feature slab and 32-row block.  (No include guard: a code fragment.)
    __shared__ f32x4 red[ROWS_WAVES][ROWS_RT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int f0 = ROWS_BX * 16, m0 = ROWS_BY * 16 * ROWS_RT;
    const int nrt = min(ROWS_RT, (a.M - m0 + 15) / 16);
    const int nchunk = (a.K + 15) / 16;
    const int fw = f0 + c;
    const bool fw_ok = fw < a.N;
    f32x4 acc[ROWS_RT];
#pragma unroll
    for (int rt = 0; rt < ROWS_RT; ++rt) acc[rt] = zero4();
    // lane (c, q): A = W[f0 + c][16 ch + 4 q + j], B = X[m0 + 16 rt + c][16 ch + 4 q + j] in k-step j of chunk ch
    rows_slab<ROWS_GROUP>(nrt, nchunk, wave,
              [&](int ch) {
                  const int k = 16 * ch + 4 * q;
                  return rows_ld4<VEC>(a.w, (long)fw * a.K + k, fw_ok ? a.K - k : 0);
              },
              [&](int ch, int rt) {
                  const int k = 16 * ch + 4 * q, row = m0 + 16 * rt + c;
                  return rows_ld4<VEC>(a.x, (long)row * a.ldx + k, row < a.M ? a.K - k : 0);
              }, acc);
#pragma unroll
    for (int rt = 0; rt < ROWS_RT; ++rt) red[wave][rt][lane] = acc[rt];
    __syncthreads();
    // waves 0, 1: the epilogue of row tile `wave`.  s[e] = Y[m0 + 16 wave + c][f0 + 4 q + e] before bias and activation
    if (wave >= nrt) return;
    const f32x4 s = rows_sum(red, min(ROWS_WAVES, nchunk), wave, lane);
    const int f = f0 + 4 * q, row = m0 + 16 * wave + c;
    if (f >= a.N || row >= a.M) return;
    f32x4 bv = zero4();
    if (a.bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (f + e < a.N) bv[e] = a.bias[f + e];
    }
    act_dispatch(a.act, [&](auto actc) {
        constexpr int ACT = decltype(actc)::value;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = act_fwd<ACT>(s[e] + bv[e], f + e >= a.split);
        float* py = a.y + (long)row * a.ldy + f;
        if (a.vecY && f + 3 < a.N) {
            *reinterpret_cast<f32x4*>(py) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (f + e < a.N) py[e] = v[e];
        }
    });
