// The body of flow_prep_kernel and flow_prep_multi_kernel (vpc_flow.hip), included as text so that both kernels are one piece of code and
// the stand-alone kernel compiles to the instructions it had with these lines spelled out in it.  blockIdx.x is the workgroup's
// index among ONE member's workgroups in both.  In scope at the point of inclusion: `x`, `m`, `mp_in`, `mp_out`, `xin`, `eps` (this member's arrays), `B`, `d`, `n_eps`, `gm`, `offset`, `offset_eps` and this member's `keep_prob` and `seed`.
// (No include guard: a code fragment.)
    if (blockIdx.x >= gm) {
        fill_normal_body(eps, n_eps, seed, offset_eps, (long)(blockIdx.x - gm) * blockDim.x + threadIdx.x,
                         EpsShard{0, 0, 0, 4});
        return;
    }
    const long n = B * d;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i0 = g * 4;
    if (i0 >= n) return;
    const bool two = mp_in || mp_out;
    U4 r{0, 0, 0, 0};
    if (mp_out && !mp_in) r = philox((uint64_t)g + offset, 0u, seed);  // the counters of vpc_nm_prep's mask_p draw
    const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
    for (int j = 0; j < 4 && i0 + j < n; ++j) {
        const long e = i0 + j;
        const long b = e / d;
        const int k = (int)(e - b * d);
        const float xv = x[e], mv = m[e];
        float* q = xin + b * 2 * d;
        q[k] = xv * mv;
        q[d + k] = mv;
        if (two) {
            const float pv = mp_in ? mp_in[e] : (u01(rr[j]) < keep_prob ? mv : 0.f);
            if (mp_out) mp_out[e] = pv;
            float* pp = xin + (B + b) * 2 * d;
            pp[k] = xv * pv;
            pp[d + k] = pv;
        }
    }
