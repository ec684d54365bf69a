// The BODY of nm_prep_kernel (vpc_misc.hip) and of its ensemble form nm_prep_multi_kernel, included as text so that the
// stand-alone kernel compiles to the instructions it had with these lines spelled out in it.  In scope: the parameters of
// nm_prep_kernel as local names, and the macros NM_PREP_DRAWS_MP (whether mask_p is drawn here), NM_PREP_MP(drawn) (the mask_p
// value of element i0 + j: the drawn one, or the injected one read from mp) and NM_PREP_KEEP_MP (a prefix of the store of a
// drawn value: empty, or a condition).  (No include guard: a code fragment, included once per kernel.)
    if (state) { offset += (uint64_t)state[1]; offset_eps += (uint64_t)state[1]; }
    if (blockIdx.x >= gm) {
        fill_normal_body(eps, n_eps, seed, offset_eps, (long)(blockIdx.x - gm) * blockDim.x + threadIdx.x, sh);
        return;
    }
    offset += (uint64_t)(elem_lo >> 2);  // counter of a mask group = its index in the GLOBAL [B_global][d] array
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i0 = g * 4;
    if (i0 >= n) return;
    U4 r{0, 0, 0, 0};
    if (NM_PREP_DRAWS_MP) r = philox((uint64_t)g + offset, 0u, seed);
    const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
    for (int j = 0; j < 4 && i0 + j < n; ++j) {
        const float xv = x[i0 + j], mv = m[i0 + j];
        xin[i0 + j] = xv * mv;
        if (mp) {
            const float pv = NM_PREP_MP(u01(rr[j]) < keep_prob ? mv : 0.f);
            NM_PREP_KEEP_MP mp[i0 + j] = pv;
            xin[n + i0 + j] = xv * pv;
        }
    }
