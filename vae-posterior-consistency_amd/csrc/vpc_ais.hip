// Annealed importance sampling with adaptive-step HMC (reference src/utils/AIS.py:94-304) as ONE persistent kernel per block
// of temperatures.
//
// Chains never interact, so a wave owns one 16-chain tile for the whole launch: z, v, the step size, the accept history,
// logw and the x tile of its chains stay in registers across the temperature loop, the fp32 decoder image (DecImg of
// vpc_layout.h, as vpc_pack_weights writes it) sits in LDS, and HBM is touched at launch start (chain state, x) and end
// (chain state) only - plus the draws when the caller injects them instead of letting the kernel generate them.
//
// One gradient pass = decoder forward L -> 50 -> 100 -> d (ReLU, ReLU, sigmoid), the row sum of the squared error, and
// dgrad back to z (no wgrad): activations chain through registers in the MFMA C/D layout (vpc_device.h), lane (c, q) of a
// wave holding features 4q..4q+3 of every 16-feature tile of chain c.  A temperature costs leapfrog_steps + 1 passes
// (11 forwards + 11 dgrads against the reference's 15 + 11): NLL(z_current) of the first pass serves both log f terms
// of the weight update and U(z_current), the last pass's NLL is U(z_proposed).  The state's nll_current field is
// informational: NLL at the final z for the caller; the next launch recomputes it in the forward its first dgrad needs anyway.
//
// The annealed density is log f(z, t) = -|z|^2 / 2 + t * sign * NLL(x; decoder(z)) with NLL = the sum over all d columns
// of MINUS the Gaussian log-density: sign = +1 is the reference as written (AIS.py:125 passes neg_gaussian_log_likelihood
// as the "log likelihood"), sign = -1 the corrected target p(z) p(x|z)^t.
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_rng.h"

namespace vpc {

constexpr int AIS_WAVES = 8, AIS_THREADS = AIS_WAVES * 64;
constexpr int AIS_ZP = 16;                 // row pitch of z inside the state
constexpr int AIS_STATE = AIS_ZP + 4;      // floats per chain: z[16], epsilon, accept_hist, logw, nll_current
// the draw counters and the Box-Muller draws (ais_ctr, ais_normal4, ais_uniform, AIS_KIND_*): vpc_rng.h, shared with
// the GEMM-backed engine of vpc_aisg.hip

struct AisArgs {
    const float* x;         // [nb][d]
    const float* img;       // decoder image
    const float* sched;     // [T] temperatures
    float* state;           // z [B][16] | epsilon [B] | accept_hist [B] | logw [B] | nll_current [B]
    const float* z0;        // [B][L] or NULL (generated); read when init != 0
    const float* v;         // [T-1][B][L] or NULL
    const float* u;         // [T-1][B] or NULL
    uint64_t seed;
    long B, nb;
    int d, L, j0, nsteps, init, leapfrog;
    float sign, init_step, grad_clip, x_logvar;
};

// sum over the four lanes (c, q = 0..3) of a chain; every one of them gets the same bits (a + b == b + a)
__device__ __forceinline__ float chain_sum(float s) {
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    return s;
}
__device__ __forceinline__ float sq4(f32x4 a) { return (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]); }

template <int DT>
__global__ __launch_bounds__(AIS_THREADS) void ais_kernel(AisArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const DecImg im(DT);
    load_image<13>(lds, a.img, im.total);
    const float* W4 = lds + im.oW4;
    const float* W5 = lds + im.oW5;
    const float* W6 = lds + im.oW6;
    __syncthreads();  // the only workgroup barrier: from here on the waves run on their own
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const long chain = ((long)blockIdx.x * AIS_WAVES + w) * 16 + c;
    if (((long)blockIdx.x * AIS_WAVES + w) * 16 >= a.B) return;  // wave without a tile
    const bool ok = chain < a.B;   // lanes of absent chains compute on zeros and store nothing
    const int L = a.L, d = a.d;
    const float inv_s2 = expf(-a.x_logvar);
    const float nll0 = (float)d * (0.5f * a.x_logvar + 0.91893853320467274f);  // sum_d log(scale) + log(2 pi) / 2
    uint32_t lat_ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) lat_ok[j] = (ok && 4 * q + j < L) ? 0xffffffffu : 0u;
    auto lat_mask = [&](f32x4 t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = __uint_as_float(__float_as_uint(t[j]) & lat_ok[j]);
        return t;
    };

    // ---- x tile of the wave's chains (chain c belongs to data row c % nb, AIS.py:28-29, 160): read once per launch
    f32x4 xv[DT];
    uint32_t col_ok = 0;  // bit 4 mt + j: column 16 mt + 4 q + j exists
    {
        const float* xr = a.x + (ok ? chain % a.nb : 0) * (long)d;
#pragma unroll
        for (int mt = 0; mt < DT; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = 16 * mt + 4 * q + j;
                const bool in = ok && f < d;
                xv[mt][j] = in ? xr[in ? f : 0] : 0.f;
                col_ok |= (in ? 1u : 0u) << (4 * mt + j);
            }
    }

    // ---- chain state
    float* sz = a.state;
    float* s_eps = a.state + a.B * AIS_ZP;
    float* s_hist = s_eps + a.B;
    float* s_logw = s_hist + a.B;
    float* s_nll = s_logw + a.B;
    f32x4 z = zero4();
    float eps = a.init_step, hist = 0.f, logw = 0.f, nll_cur = 0.f;
    if (a.init) {
        if (a.z0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ok && 4 * q + j < L) z[j] = a.z0[chain * L + 4 * q + j];
        } else {
            z = lat_mask(ais_normal4(chain, q, 0, AIS_KIND_Z0, a.seed));
        }
    } else if (ok) {
        z = lat_mask(*reinterpret_cast<const f32x4*>(sz + chain * AIS_ZP + 4 * q));
        eps = s_eps[chain]; hist = s_hist[chain]; logw = s_logw[chain]; nll_cur = s_nll[chain];
    }

    // ---- one gradient pass: NLL(x; decoder(zz)) and d NLL / d zz
    int cc = c, qq = q;
    auto nll_grad = [&](const f32x4& zz, float& nll, f32x4& dz) {
        launder(cc, qq);
        f32x4 zin[1] = {zz};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * q + j == L) zin[0][j] = 1.f;  // constant feature that drives the bias chain
        f32x4 g1[H2T], g2[H1T];
#pragma unroll
        for (int mt = 0; mt < H2T; ++mt) g1[mt] = relu4(tile_fwd<1, S4>(W4, mt, zin, zero4(), cc, qq));
        launder(cc, qq);
#pragma unroll
        for (int mt = 0; mt < H1T; ++mt) {
            __builtin_amdgcn_sched_barrier(0);
            g2[mt] = relu4(tile_fwd_p2<H2T, 64, NK2>(W5, mt, g1, cc, qq));
        }
        const uint32_t gm1 = relu_bits<H2T>(g1);
        launder(cc, qq);
        f32x4 dpre[DT];
        float ss = 0.f;
#pragma unroll
        for (int mt = 0; mt < DT; ++mt) {
            const f32x4 pre = tile_fwd_p2<H1T, 128, NK1>(W6, mt, g2, cc, qq);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = fast_sigmoid(pre[j]);
                // absent columns (ragged d) and absent chains: no error term, no gradient
                const float diff = __uint_as_float(__float_as_uint(xh - xv[mt][j]) &
                                                   (uint32_t)__builtin_amdgcn_sbfe((int)col_ok, 4 * mt + j, 1));
                ss = fmaf(diff, diff, ss);
                dpre[mt][j] = diff * (xh - xh * xh);
            }
            asm volatile("" : "+v"(dpre[mt][0]), "+v"(dpre[mt][1]), "+v"(dpre[mt][2]), "+v"(dpre[mt][3]), "+v"(ss));
        }
        const uint32_t gm2 = relu_bits<H1T>(g2);
        launder(cc, qq);
        f32x4 dg2[H1T];
#pragma unroll
        for (int mt = 0; mt < H1T; ++mt) {
            __builtin_amdgcn_sched_barrier(0);
            dg2[mt] = gate_bits(tile_T_p2<DT, 128>(W6, mt, dpre, cc, qq), gm2, mt);
        }
        launder(cc, qq);
        f32x4 dg1[H2T];
#pragma unroll
        for (int mt = 0; mt < H2T; ++mt) {
            __builtin_amdgcn_sched_barrier(0);
            dg1[mt] = gate_bits(tile_T_p2<H1T, 64, NK1>(W5, mt, dg2, cc, qq), gm1, mt);
        }
        launder(cc, qq);
        const f32x4 t = tile_T<H2T, S4, NK2>(W4, 0, dg1, zero4(), cc, qq);
        dz = lat_mask(t * inv_s2);
        nll = nll0 + 0.5f * inv_s2 * chain_sum(ss);
    };

    const int Lf = a.leapfrog;
#pragma unroll 1
    for (int j = a.j0; j < a.j0 + a.nsteps; ++j) {
        const float t0 = a.sched[j - 1], t1 = a.sched[j];
        const float ts = t1 * a.sign;
        // ---- momentum (AIS.py:185) and the uniform of accept_reject (AIS.py:289)
        f32x4 v0;
        if (a.v) {
            v0 = zero4();
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                if (ok && 4 * q + jj < L) v0[jj] = a.v[((long)(j - 1) * a.B + chain) * L + 4 * q + jj];
        } else {
            v0 = lat_mask(ais_normal4(chain, q, j, AIS_KIND_V, a.seed));
        }
        const float un = a.u ? (ok ? a.u[(long)(j - 1) * a.B + chain] : 1.f) : ais_uniform(chain, j, a.seed);
        // ---- leapfrog (AIS.py:237-262): half step, L position steps, half step; U = -log f(., t1)
        f32x4 zz = z, vv = v0;
        float h_cur = 0.f, nll_prop = 0.f;
#pragma unroll 1
        for (int s = 0; s <= Lf; ++s) {
            float nll;
            f32x4 dn;
            nll_grad(zz, nll, dn);
            f32x4 g = zz - dn * ts;  // grad U = z - t1 * sign * d NLL / d z, clamped (AIS.py:194-196)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) g[jj] = fminf(fmaxf(g[jj], -a.grad_clip), a.grad_clip);
            if (s == 0) {
                nll_cur = nll;
                logw += (t1 - t0) * a.sign * nll;  // log f(z, t1) - log f(z, t0) (AIS.py:180-182)
                h_cur = 0.5f * chain_sum(sq4(v0)) + (0.5f * chain_sum(sq4(z)) - ts * nll);
            }
            if (s == 0 || s == Lf) vv = vv - (g * eps) * 0.5f;
            else vv = vv - g * eps;
            if (s < Lf) zz = zz + vv * eps;
            else nll_prop = nll;
        }
        // ---- accept / reject and step-size adaptation (AIS.py:265-304)
        const float h_prop = 0.5f * chain_sum(sq4(vv)) + (0.5f * chain_sum(sq4(zz)) - ts * nll_prop);
        const bool acc = expf(h_cur - h_prop) > un;
        if (acc) { z = zz; nll_cur = nll_prop; }
        hist += acc ? 1.f : 0.f;
        eps = fminf(fmaxf(eps * (hist / (float)j > 0.65f ? 1.02f : 0.98f), 1e-4f), 0.5f);
    }

    if (ok) {
        *reinterpret_cast<f32x4*>(sz + chain * AIS_ZP + 4 * q) = z;
        if (q == 0) { s_eps[chain] = eps; s_hist[chain] = hist; s_logw[chain] = logw; s_nll[chain] = nll_cur; }
    }
}

// the draws of ais_kernel as dense arrays (any of them may be NULL): z0 [B][L], v [T-1][B][L], u [T-1][B]
__global__ __launch_bounds__(256) void ais_draws_kernel(float* z0, float* v, float* u, long B, int L, int T, uint64_t seed) {
    const int G = (L + 3) / 4;
    const long total = (long)T * B * G;  // (j, chain, group); j = 0: z0
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int group = (int)(e % G);
        const long chain = (e / G) % B;
        const int j = (int)((e / G) / B);
        float* out = j == 0 ? z0 : v;
        if (out) {
            const f32x4 n = ais_normal4(chain, group, j, j == 0 ? AIS_KIND_Z0 : AIS_KIND_V, seed);
            float* row = out + ((long)(j == 0 ? 0 : j - 1) * B + chain) * L;
            for (int jj = 0; jj < 4; ++jj)
                if (4 * group + jj < L) row[4 * group + jj] = n[jj];
        }
        if (u && j > 0 && group == 0) u[(long)(j - 1) * B + chain] = ais_uniform(chain, j, seed);
    }
}

static bool ais_shape_ok(long B, int d, int L) {
    return B >= 1 && B < (1L << 30) && d >= 1 && d <= MAX_D && L >= 1 && L <= MAX_L;
}

template <int DT>
static int ais_launch(const AisArgs& a, hipStream_t s) {
    const size_t lds = sizeof(float) * DecImg(DT).total;
    auto kern = ais_kernel<DT>;
    if (!lds_attr_done(reinterpret_cast<const void*>(kern), lds)) return VPC_ERR_HIP;
    const long tiles = (a.B + 15) / 16;
    hipLaunchKernelGGL(kern, dim3((unsigned)((tiles + AIS_WAVES - 1) / AIS_WAVES)), dim3(AIS_THREADS), lds, s, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // namespace vpc

using namespace vpc;

extern "C" {

int vpc_ais_applicable(long B, int d, int L) { return ais_shape_ok(B, d, L) ? 1 : 0; }

long vpc_ais_state_floats(long B) { return B > 0 ? B * AIS_STATE : 0; }

int vpc_ais_run(const float* x, const float* dec_img, const float* schedule, int T, int j0, int nsteps, int init,
                float* state, const float* z0, const float* v, const float* u, unsigned long long seed, float sign,
                int leapfrog_steps, float init_step_size, float grad_clip, float x_logvar, long B, long nb, int d, int L,
                void* stream) {
    if (!x || !dec_img || !schedule || !state || !aligned16(dec_img) || !aligned16(state)) return VPC_ERR_ARG;
    if (B < 1 || nb < 1 || nb > B || T < 2 || j0 < 1 || nsteps < 1 || (long)j0 + nsteps > T || leapfrog_steps < 1)
        return VPC_ERR_ARG;
    if (sign != 1.f && sign != -1.f) return VPC_ERR_ARG;
    if (!ais_shape_ok(B, d, L)) return VPC_ERR_SHAPE;
    AisArgs a{};
    a.x = x; a.img = dec_img; a.sched = schedule; a.state = state; a.z0 = z0; a.v = v; a.u = u; a.seed = seed;
    a.B = B; a.nb = nb; a.d = d; a.L = L; a.j0 = j0; a.nsteps = nsteps; a.init = init; a.leapfrog = leapfrog_steps;
    a.sign = sign; a.init_step = init_step_size; a.grad_clip = grad_clip; a.x_logvar = x_logvar;
    switch (dt_for(d)) {
        case 1: return ais_launch<1>(a, (hipStream_t)stream);
        case 2: return ais_launch<2>(a, (hipStream_t)stream);
        case 4: return ais_launch<4>(a, (hipStream_t)stream);
        case 8: return ais_launch<8>(a, (hipStream_t)stream);
    }
    return VPC_ERR_SHAPE;
}

int vpc_ais_draws(float* z0, float* v, float* u, long B, int L, int T, unsigned long long seed, void* stream) {
    if (B < 1 || T < 1 || (!z0 && !v && !u)) return VPC_ERR_ARG;
    if (B >= (1L << 30) || L < 1 || L > AIS_DRAW_MAX_L || T >= (1 << 24)) return VPC_ERR_SHAPE;
    const long total = (long)T * B * ((L + 3) / 4);
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(ais_draws_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                       (hipStream_t)stream, z0, v, u, B, L, T, (uint64_t)seed);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
