// Annealed importance sampling with adaptive-step HMC (reference src/utils/AIS.py:94-304) around the generic fp32 MFMA GEMM
// layer ops of vpc_gemm.hip: the engine for every decoder that returns a Gaussian (mean, logvar) and does not fit the
// persistent kernel of vpc_ais.hip (its fp32 weights in LDS): the MNAR decoders with their learned log-variance head, the
// flow decoders (4 ELU layers of hid_dim), the image-width EDDI decoder, and the 50-100 chain past obs_dim 128 / latent 15.
//
// The chain state lives in a caller-owned workspace; a gradient pass is
//     n_layers x vpc_linear_fwd -> aisg_energy_kernel -> n_layers x vpc_linear_dgrad -> aisg_leapfrog_kernel
// and a temperature is leapfrog_steps + 1 passes between two launches of aisg_temp_kernel (the end of temperature j and the
// begin of j + 1 share one launch).  NLL(z_current) of the first pass serves both log f terms of the weight update and
// U(z_current); the last pass's NLL is U(z_proposed).  Every kernel is a pure function of the workspace, the draws depend
// on (chain, j, kind, seed) only, and no reduction uses atomics: results are bit-equal however the schedule is split.
//
// log f(z, t) = -|z|^2 / 2 + t * sign * NLL(x; decoder(z)), NLL = the sum over the columns of MINUS the Gaussian
// log-density (utils.py:149-151), each term times the 0/1 mask when one is given; sign as in vpc_ais.hip.
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_rng.h"
#include "../../include/vpc.h"

namespace vpc {

constexpr int AISG_MAX_LAYERS = 8, AISG_MAX_D = 1024, AISG_MAX_HID = 512, AISG_MAX_L = AIS_DRAW_MAX_L;
constexpr int AISG_THREADS = 256;

static long r4(long n) { return (n + 3) & ~3L; }

// the workspace: [z | epsilon | accept_hist | logw | nll_current] first (the caller reads these), then the engine's own
struct AisgWs {
    float *z, *eps, *hist, *logw, *nll_cur;     // chain state proper
    float *zz, *vv, *dz, *nll, *kin, *pot, *un;  // trajectory: proposed z (= the decoder's input), momentum, dNLL/dz, ..
    float* act[AISG_MAX_LAYERS];                 // act[i]: output of layer i  [B][N_i]
    float* dact[AISG_MAX_LAYERS];                // dact[i]: d NLL / d act[i]  [B][N_i]
    long total;
};
static AisgWs aisg_carve(float* base, long B, int L, int nl, const int* N) {
    AisgWs w{};
    long o = 0;
    auto take = [&](long n) { float* p = base ? base + o : nullptr; o += r4(n); return p; };
    w.z = take(B * L); w.eps = take(B); w.hist = take(B); w.logw = take(B); w.nll_cur = take(B);
    w.zz = take(B * L); w.vv = take(B * L); w.dz = take(B * L);
    w.nll = take(B); w.kin = take(B); w.pot = take(B); w.un = take(B);
    for (int i = 0; i < nl; ++i) w.act[i] = take(B * (long)N[i]);
    for (int i = 0; i < nl; ++i) w.dact[i] = take(B * (long)N[i]);
    w.total = o;
    return w;
}

// ---- energy and seed: per-chain NLL and d NLL / d (decoder output), one wave per chain
// out [B][ldo]: post-activation [mean d | logvar d] (learned != 0) or mean d with the scalar x_logvar.  dout: same layout.
template <bool LEARNED, bool MASKED>
__global__ __launch_bounds__(AISG_THREADS) void aisg_energy_kernel(const float* __restrict__ out, float* __restrict__ dout,
                                                                    const float* __restrict__ x,
                                                                    const float* __restrict__ mask, float* __restrict__ nll,
                                                                    long B, long nb, int d, float x_logvar) {
    const int lane = threadIdx.x & 63;
    const long chain = (long)blockIdx.x * (AISG_THREADS / 64) + (threadIdx.x >> 6);
    if (chain >= B) return;  // whole waves only: no divergence inside the reduction below
    const long row = chain % nb;  // safe_repeat order (AIS.py:28-29, 160)
    const long ldo = LEARNED ? 2L * d : d;
    const float* o = out + chain * ldo;
    float* g = dout + chain * ldo;
    const float* xr = x + row * d;
    const float* mr = MASKED ? mask + row * d : nullptr;
    const float inv_c = expf(-x_logvar), half_log2pi = 0.91893853320467274f;
    float s = 0.f;
    for (int f = lane; f < d; f += 64) {  // a lane's columns in ascending order, then the fixed DPP tree
        const float m = MASKED ? mr[f] : 1.f;
        const float diff = o[f] - xr[f];
        if (LEARNED) {
            const float lv = o[d + f];
            const float inv = expf(-lv);
            const float q = 0.5f * diff * diff * inv;
            s += m * (q + (0.5f * lv + half_log2pi));
            g[f] = m * (diff * inv);
            g[d + f] = m * (0.5f - q);
        } else {
            s += m * (0.5f * diff * diff * inv_c + (0.5f * x_logvar + half_log2pi));
            g[f] = m * (diff * inv_c);
        }
    }
    s = wave_sum_dpp(s);
    if (lane == 0) nll[chain] = s;
}

struct AisgStep {
    const float* sched;
    float *z, *eps, *hist, *logw, *nll_cur, *zz, *vv, *dz, *nll, *kin, *pot, *un;
    const float *z0, *v, *u;  // injected draws or NULL
    uint64_t seed;
    long B;
    int L;
    float sign, init_step, grad_clip;
};

// ---- leapfrog update after pass s of temperature j (AIS.py:252-260): one thread per chain
__global__ __launch_bounds__(AISG_THREADS) void aisg_leapfrog_kernel(AisgStep a, int j, int s, int Lf) {
    const long c = (long)blockIdx.x * AISG_THREADS + threadIdx.x;
    if (c >= a.B) return;
    const float t0 = a.sched[j - 1], t1 = a.sched[j];
    const float ts = t1 * a.sign, e = a.eps[c], n = a.nll[c];
    float* zz = a.zz + c * a.L;
    float* vv = a.vv + c * a.L;
    const float* dz = a.dz + c * a.L;
    for (int l = 0; l < a.L; ++l) {
        float g = zz[l] - dz[l] * ts;  // grad U = z - t1 * sign * d NLL / d z, clamped (AIS.py:194-196)
        g = fminf(fmaxf(g, -a.grad_clip), a.grad_clip);
        float v = vv[l];
        if (s == 0 || s == Lf) v = v - (g * e) * 0.5f;
        else v = v - g * e;
        vv[l] = v;
        if (s < Lf) zz[l] = zz[l] + v * e;
    }
    if (s == 0) {
        a.nll_cur[c] = n;
        a.logw[c] += (t1 - t0) * a.sign * n;  // log f(z, t1) - log f(z, t0) (AIS.py:180-182)
        a.pot[c] = a.pot[c] - ts * n;          // -log f(z_current, t1) = |z|^2 / 2 - t1 * sign * NLL
    }
}

// ---- temperature end (accept / reject and step adaptation of j_end, AIS.py:265-304) and begin (the draws of j_beg and
// the start of its trajectory); j_end / j_beg = 0: that half is not run.  init: chain state from z0 / the seed first.
__global__ __launch_bounds__(AISG_THREADS) void aisg_temp_kernel(AisgStep a, int j_end, int j_beg, int init) {
    const long c = (long)blockIdx.x * AISG_THREADS + threadIdx.x;
    if (c >= a.B) return;
    const int L = a.L, G = (L + 3) >> 2;
    float* z = a.z + c * L;
    float* zz = a.zz + c * L;
    float* vv = a.vv + c * L;
    if (init) {
        for (int g = 0; g < G; ++g) {
            f32x4 n = zero4();
            if (!a.z0) n = ais_normal4(c, g, 0, AIS_KIND_Z0, a.seed);
            for (int i = 0; i < 4 && 4 * g + i < L; ++i) z[4 * g + i] = a.z0 ? a.z0[c * L + 4 * g + i] : n[i];
        }
        a.eps[c] = a.init_step; a.hist[c] = 0.f; a.logw[c] = 0.f; a.nll_cur[c] = 0.f;
    }
    if (j_end) {
        const float ts = a.sched[j_end] * a.sign, n = a.nll[c];
        float sv = 0.f, sz = 0.f;
        for (int l = 0; l < L; ++l) { sv = fmaf(vv[l], vv[l], sv); sz = fmaf(zz[l], zz[l], sz); }
        const float h_cur = a.kin[c] + a.pot[c];
        const float h_prop = 0.5f * sv + (0.5f * sz - ts * n);
        const bool acc = expf(h_cur - h_prop) > a.un[c];
        if (acc) {
            for (int l = 0; l < L; ++l) z[l] = zz[l];
            a.nll_cur[c] = n;
        }
        const float hist = a.hist[c] + (acc ? 1.f : 0.f);
        a.hist[c] = hist;
        a.eps[c] = fminf(fmaxf(a.eps[c] * (hist / (float)j_end > 0.65f ? 1.02f : 0.98f), 1e-4f), 0.5f);
    }
    if (j_beg) {
        float sv = 0.f, sz = 0.f;
        for (int g = 0; g < G; ++g) {
            f32x4 n = zero4();
            if (!a.v) n = ais_normal4(c, g, j_beg, AIS_KIND_V, a.seed);  // momentum (AIS.py:185)
            for (int i = 0; i < 4 && 4 * g + i < L; ++i) {
                const int l = 4 * g + i;
                const float v0 = a.v ? a.v[((long)(j_beg - 1) * a.B + c) * L + l] : n[i];
                const float zc = z[l];
                vv[l] = v0; zz[l] = zc;
                sv = fmaf(v0, v0, sv); sz = fmaf(zc, zc, sz);
            }
        }
        a.kin[c] = 0.5f * sv; a.pot[c] = 0.5f * sz;
        a.un[c] = a.u ? a.u[(long)(j_beg - 1) * a.B + c] : ais_uniform(c, j_beg, a.seed);  // accept_reject's (AIS.py:289)
    }
}

static bool aisg_chain_ok(int nl, const int* K, const int* N, const int* act, int split, int d, int L, bool* learned) {
    if (nl < 1 || nl > AISG_MAX_LAYERS || !K || !N || !act) return false;
    if (K[0] != L) return false;
    for (int i = 0; i < nl; ++i) {
        if (act[i] < 0 || act[i] > 3 || N[i] < 1 || K[i] < 1) return false;
        if (i + 1 < nl && K[i + 1] != N[i]) return false;
    }
    if (N[nl - 1] == d) *learned = false;
    else if (N[nl - 1] == 2 * d && split == d) *learned = true;
    else return false;
    return true;
}

}  // namespace vpc

using namespace vpc;

extern "C" {

long vpc_aisg_workspace_floats(long B, int L, int n_layers, const int* N) {
    if (B < 1 || L < 1 || n_layers < 1 || n_layers > AISG_MAX_LAYERS || !N) return 0;
    return aisg_carve(nullptr, B, L, n_layers, N).total;
}

int vpc_aisg_run(const float* x, const float* mask, const float* const* w, const float* const* b, const int* K,
                 const int* N, const int* act, int n_layers, int last_split, float x_logvar, const float* schedule, int T,
                 int j0, int nsteps, int init, float* workspace, long workspace_floats, const float* z0, const float* v,
                 const float* u, unsigned long long seed, float sign, int leapfrog_steps, float init_step_size,
                 float grad_clip, long B, long nb, int d, int L, void* stream) {
    if (!x || !w || !b || !schedule || !workspace || !aligned16(workspace)) return VPC_ERR_ARG;
    if (B < 1 || nb < 1 || nb > B || T < 2 || j0 < 1 || nsteps < 1 || (long)j0 + nsteps > T || leapfrog_steps < 1)
        return VPC_ERR_ARG;
    if (sign != 1.f && sign != -1.f) return VPC_ERR_ARG;
    if (n_layers < 1 || n_layers > AISG_MAX_LAYERS || !K || !N || !act) return VPC_ERR_ARG;
    if (B >= (1L << 30) || d < 1 || d > AISG_MAX_D || L < 1 || L > AISG_MAX_L || T >= (1 << 24)) return VPC_ERR_SHAPE;
    for (int i = 0; i + 1 < n_layers; ++i)
        if (N[i] > AISG_MAX_HID) return VPC_ERR_SHAPE;
    bool learned = false;
    if (!aisg_chain_ok(n_layers, K, N, act, last_split, d, L, &learned)) return VPC_ERR_ARG;
    for (int i = 0; i < n_layers; ++i)
        if (!w[i]) return VPC_ERR_ARG;
    const AisgWs ws = aisg_carve(workspace, B, L, n_layers, N);
    if (workspace_floats < ws.total) return VPC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;

    AisgStep a{};
    a.sched = schedule;
    a.z = ws.z; a.eps = ws.eps; a.hist = ws.hist; a.logw = ws.logw; a.nll_cur = ws.nll_cur;
    a.zz = ws.zz; a.vv = ws.vv; a.dz = ws.dz; a.nll = ws.nll; a.kin = ws.kin; a.pot = ws.pot; a.un = ws.un;
    a.z0 = z0; a.v = v; a.u = u; a.seed = seed; a.B = B; a.L = L;
    a.sign = sign; a.init_step = init_step_size; a.grad_clip = grad_clip;
    const dim3 per_chain((unsigned)((B + AISG_THREADS - 1) / AISG_THREADS)), blk(AISG_THREADS);
    const dim3 per_wave((unsigned)((B + AISG_THREADS / 64 - 1) / (AISG_THREADS / 64)));
    const int nl = n_layers, last = n_layers - 1;

    for (int j = j0; j < j0 + nsteps; ++j) {
        // the end of the temperature before (inside this block of temperatures) and the begin of this one
        hipLaunchKernelGGL(aisg_temp_kernel, per_chain, blk, 0, st, a, j > j0 ? j - 1 : 0, j, (init && j == j0) ? 1 : 0);
        for (int s = 0; s <= leapfrog_steps; ++s) {
            for (int i = 0; i < nl; ++i) {
                const int rc = vpc_linear_fwd(i ? ws.act[i - 1] : ws.zz, K[i], w[i], b[i], ws.act[i], N[i], B, N[i], K[i],
                                              act[i], i == last ? last_split : 0, 0, stream);
                if (rc != VPC_OK) return rc;
            }
            if (learned) {
                if (mask) hipLaunchKernelGGL((aisg_energy_kernel<true, true>), per_wave, blk, 0, st, ws.act[last], ws.dact[last], x, mask, ws.nll, B, nb, d, x_logvar);
                else hipLaunchKernelGGL((aisg_energy_kernel<true, false>), per_wave, blk, 0, st, ws.act[last], ws.dact[last], x, mask, ws.nll, B, nb, d, x_logvar);
            } else {
                if (mask) hipLaunchKernelGGL((aisg_energy_kernel<false, true>), per_wave, blk, 0, st, ws.act[last], ws.dact[last], x, mask, ws.nll, B, nb, d, x_logvar);
                else hipLaunchKernelGGL((aisg_energy_kernel<false, false>), per_wave, blk, 0, st, ws.act[last], ws.dact[last], x, mask, ws.nll, B, nb, d, x_logvar);
            }
            for (int i = last; i >= 0; --i) {
                // gated by the layer's own activation at the output (the energy kernel's gradient is with respect to the
                // post-activation heads) and by the activation of the layer below through that layer's outputs
                const int rc = vpc_linear_dgrad(ws.dact[i], N[i], i == last ? ws.act[i] : nullptr, N[i], i == last ? act[i] : 0,
                                                i == last ? last_split : 0, w[i], i ? ws.act[i - 1] : nullptr, K[i],
                                                i ? act[i - 1] : 0, i ? ws.dact[i - 1] : ws.dz, K[i], B, N[i], K[i], 0, stream);
                if (rc != VPC_OK) return rc;
            }
            hipLaunchKernelGGL(aisg_leapfrog_kernel, per_chain, blk, 0, st, a, j, s, leapfrog_steps);
        }
    }
    hipLaunchKernelGGL(aisg_temp_kernel, per_chain, blk, 0, st, a, j0 + nsteps - 1, 0, 0);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
