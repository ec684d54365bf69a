// Config 5 reward for the flow models (reference src/experiment_main/evaluate.py: R_lindley_chain_ratio_version :637-665,
// chaini_I_ratio_version :669-684, chaini_II_ratio_version :688-708, called per candidate from active_learning_func
// :416-422; the encoder is VAEFlow.encoder, src/models/VAE.py:1924-1931, Flow.forward :1816-1831).
//
// For row n, candidate u < d-1 with mask[n][u] == 0, target T = d-1:
//     R[n][u] = 1/M sum_m ( sum_l |lp_Ia - lp_Ib| - sum_l |lp_IIa - lp_IIb| )
// each lp one encoder call's z_log_prob with its own draw.  Only the first encoder layer sees the candidate:
//     a-calls (Ia, IIa):  pre_a[chain][m][n] = b1 + W1 [x' * mask' | mask']            2 n M trunk rows, independent of u
//     b-calls (Ib, IIb):  pre_a + W1[:, u] * im[m][n][u] + W1[:, d + u]                  2 n (d-1) M trunk rows
// so the b-rows' first-layer output h1 = ELU(pre_b) is GENERATED into the layer-2 GEMM's LDS operand tile and never
// exists in memory.  Candidates are processed in chunks; a chunk's layer-2 output goes through a caller-owned workspace
// to the generic layer-3 GEMM (vpc_linear_fwd), then one elementwise launch evaluates the four flows of every
// (n, u, m) and a last one sums over m in a fixed order.
//
//   fr_prep     the a-calls' encoder inputs [chain][m][n][2d] (with the reference's carry-over of the imputed target,
//               evaluate.py:653-658) and the transposed first-layer table w1t[u] = (W1[:, u], W1[:, d + u])
//   fr_draws    eps ~ N(0, 1) for a slab of candidates; the Philox counter of a value is its index in the dense
//               [d-1][M][4][n][10] tensor, so it does not depend on the chunking
//   fr_flags    torch.any(|eps| <= 1) (VAE.py:1698) over loc(u) x 10 for each (u, m, call): one wave per group
//   fr_trunk    layer 2 of the b-rows: fp32 MFMA, 8 waves, 128 x 128 tile, 64-wide contraction chunks through
//               XOR-swizzled LDS tiles (the forward of vpc_gemm.hip's linear_kernel with a generated X tile)
//   fr_ratio    per (u, m, n): the a and b flows of both chains, |lp_a - lp_b| summed over the latents in latent order
//   fr_reduce   R[n][u] = (sum over m in m order) / M, -1e4 where observed
// No atomics; every sum has a fixed order, and a row's GEMM accumulation order does not depend on its tile, so R is
// bit-reproducible and independent of the chunk size.
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_flow_device.h"
#include "vpc_rng.h"

namespace vpc {

constexpr int FR_THREADS = 512;   // trunk: 8 waves, 4 (feature) x 2 (row); a wave owns 32 features x 64 rows
constexpr int FR_TILE = 8192;     // floats per LDS tile ([128][64])
constexpr int FR_MAX_HID = 512;
constexpr int FR_GROUPS = 25;     // fr_ratio: (u, m, n) groups of ten latent threads per 256-thread workgroup

__device__ __forceinline__ float fr_elu(float v) { return v > 0.f ? v : __expf(v) - 1.f; }  // = vpc_gemm.hip's ACT_ELU

// ------------------------------------------------------------------------------------------------ prep
__global__ void __launch_bounds__(256) fr_prep_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                      const float* __restrict__ im, const float* __restrict__ W1,
                                                      float* __restrict__ xin, float* __restrict__ w1t, int n, int d,
                                                      int M, int H, int Hp, unsigned gm) {
    const int T = d - 1;
    if (blockIdx.x < gm) {
        const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
        if (e >= 2L * M * n * d) return;
        const int k = (int)(e % d);
        const long r = e / d;
        const int i = (int)(r % n);
        const int t = (int)(r / n);
        const int m = t % M, ch = t / M;
        float mv = mask[(long)i * d + k] != 0.f ? 1.f : 0.f;
        float xv = x[(long)i * d + k];
        if (k == T) {
            if (ch == 0) {  // calls Ia / Ib see the target the previous sample left in temp_x (evaluate.py:653-658)
                if (m > 0) xv = im[((long)(m - 1) * n + i) * d + T];
            } else {        // calls IIa / IIb: target imputed and marked observed
                xv = im[((long)m * n + i) * d + T];
                mv = 1.f;
            }
        }
        float* q = xin + r * 2 * d;
        q[k] = xv * mv;
        q[d + k] = mv;
        return;
    }
    const long e = (long)(blockIdx.x - gm) * blockDim.x + threadIdx.x;
    if (e >= (long)T * 2 * Hp) return;
    const int h = (int)(e % Hp);
    const int s = (int)((e / Hp) & 1);
    const int u = (int)(e / (2 * Hp));
    w1t[e] = h < H ? W1[(long)h * 2 * d + s * d + u] : 0.f;
}

// ------------------------------------------------------------------------------------------------ draws and flags
__global__ void __launch_bounds__(256) fr_draws_kernel(float* __restrict__ out, long n_out, uint64_t seed, uint64_t group0) {
    fill_normal_body(out, n_out, seed, group0, (long)blockIdx.x * blockDim.x + threadIdx.x, EpsShard{0, 0, 0, 4});
}

// group g = ((u - u0) M + m) 4 + call; eps = the slab of the candidates [u0, u0 + uc)
__global__ void __launch_bounds__(64) fr_flags_kernel(const float* __restrict__ eps, const float* __restrict__ mask,
                                                      int* __restrict__ flags, int n, int d, int M, int u0) {
    const int g = blockIdx.x;
    const int u = u0 + g / (4 * M);
    const float* e = eps + (long)g * n * FLOW_L;
    int any = 0;
    for (int i = threadIdx.x; i < n; i += 64) {
        if (mask[(long)i * d + u] != 0.f) continue;  // not in loc(u): the row is not part of the encoder call
#pragma unroll
        for (int l = 0; l < FLOW_L; ++l) any |= fabsf(e[(long)i * FLOW_L + l]) <= 1.f ? 1 : 0;
    }
    const int v = __any(any) ? 1 : 0;
    if (threadIdx.x == 0) flags[g] = v;
}

// ------------------------------------------------------------------------------------------------ b-row trunk, layer 2
struct FrTrunkArgs {
    const float* W2; const float* b2;  // seq_encoder.2: [H][H], [H]
    const float* preA;                 // [2][M][n][Hp], pad columns zero
    const float* w1t;                  // [d-1][2][Hp], pad columns zero
    const float* im;                   // [M][n][d]
    float* h2;                         // [rows][Hp]
    int n, d, M, H, Hp, u0, rows, vecW;
};

// global -> registers: a 128 x 64 tile of W2 (4 float4 per thread), zero outside [0, H) x [0, H)
__device__ __forceinline__ f32x4 fr_wload(const float* __restrict__ W, int H, int row, int col, bool interior, int vec) {
    const float* p = W + (long)row * H + col;
    if (interior) return *reinterpret_cast<const f32x4*>(p);
    f32x4 v = zero4();
    if (row < H && col < H) {
        if (vec && col + 3 < H) {
            v = *reinterpret_cast<const f32x4*>(p);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (col + e < H) v[e] = p[e];
        }
    }
    return v;
}
__device__ __forceinline__ void fr_sstore(float* __restrict__ s, const f32x4 (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (threadIdx.x >> 4) + 32 * i, sl = threadIdx.x & 15;
        *reinterpret_cast<f32x4*>(s + row * 64 + ((sl ^ (row & 15)) << 2)) = r[i];
    }
}
__device__ __forceinline__ f32x4 fr_frag(const float* __restrict__ s, int ob, int kk, int c, int q) {
    return *reinterpret_cast<const f32x4*>(s + (16 * ob + c) * 64 + (((4 * kk + q) ^ c) << 2));
}

// Row r of a chunk = (((u - u0) M + m) 2 + chain) n + i.  Thread t generates the 16-byte slot (t & 15) of the tile rows
// (t >> 4) + 32 i, i < 4, in every contraction chunk, so the row decode happens once.
__global__ __launch_bounds__(FR_THREADS, 2) void fr_trunk_kernel(FrTrunkArgs a) {
    extern __shared__ __align__(16) float lds[];
    float* sA = lds;
    float* sB = lds + FR_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int wr = wave >> 1, wc = wave & 1;
    const int j0 = blockIdx.x * 128, i0 = blockIdx.y * 128;
    const int H = a.H, Hp = a.Hp;
    const int n_it = min(2, max(0, (H - i0 - 32 * wr + 15) / 16));
    const int n_jt = min(4, max(0, (a.rows - j0 - 64 * wc + 15) / 16));

    const float* pa[4];
    const float* pw[4];
    float iv[4];
    const int col4 = 4 * (threadIdx.x & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = j0 + (threadIdx.x >> 4) + 32 * i;
        pa[i] = nullptr;
        pw[i] = a.w1t;
        iv[i] = 0.f;
        if (row < a.rows) {
            const int in = row % a.n;
            int t = row / a.n;
            const int ch = t & 1;
            t >>= 1;
            const int m = t % a.M, u = a.u0 + t / a.M;
            pa[i] = a.preA + ((long)(ch * a.M + m) * a.n + in) * Hp;
            pw[i] = a.w1t + (long)u * 2 * Hp;
            iv[i] = a.im[((long)m * a.n + in) * a.d + u];
        }
    }

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = zero4();

    f32x4 ra[4], rb[4];
    auto load_chunk = [&](int k0) {
        const bool interior = a.vecW && i0 + 128 <= H && k0 + 64 <= H;  // workgroup-uniform
#pragma unroll
        for (int i = 0; i < 4; ++i)
            ra[i] = fr_wload(a.W2, H, i0 + (threadIdx.x >> 4) + 32 * i, k0 + col4, interior, a.vecW);
#pragma unroll
        for (int i = 0; i < 4; ++i)  // the rows' a pre-activations: requested a chunk ahead, under the MFMAs
            rb[i] = (pa[i] && k0 + col4 < Hp) ? *reinterpret_cast<const f32x4*>(pa[i] + k0 + col4) : zero4();
    };
    // h1 = ELU(pre_a + W1[:, u] im + W1[:, d + u]) for this thread's 16 tile elements (the table is cache-resident)
    auto generate = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!(pa[i] && k0 + col4 < Hp)) continue;  // rb[i] is zero
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(pw[i] + k0 + col4);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(pw[i] + Hp + k0 + col4);
#pragma unroll
            for (int e = 0; e < 4; ++e) rb[i][e] = fr_elu(fmaf(w0[e], iv[i], rb[i][e]) + w1[e]);
        }
    };

    load_chunk(0);
    for (int k0 = 0; k0 < H; k0 += 64) {
        generate(k0);
        __syncthreads();
        fr_sstore(sA, ra);
        fr_sstore(sB, rb);
        __syncthreads();
        if (k0 + 64 < H) load_chunk(k0 + 64);
        const int n_kk = min(4, (H - k0 + 15) / 16);
        if (n_it == 0 || n_jt == 0) continue;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (kk >= n_kk) break;
            f32x4 fa[2], fb[4];
#pragma unroll
            for (int t = 0; t < 2; ++t) fa[t] = t < n_it ? fr_frag(sA, 2 * wr + t, kk, c, q) : zero4();
#pragma unroll
            for (int t = 0; t < 4; ++t) fb[t] = t < n_jt ? fr_frag(sB, 4 * wc + t, kk, c, q) : zero4();
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                if (it >= n_it) break;
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) {
                    if (jt >= n_jt) break;
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[it][jt] = VPC_MFMA(fa[it][j], fb[jt][j], acc[it][jt]);
                }
            }
        }
    }

    // acc[it][jt][e] = D[feature i0 + 32 wr + 16 it + 4 q + e][row j0 + 64 wc + 16 jt + c]
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int f = i0 + 32 * wr + 16 * it + 4 * q;
        if (f >= H) continue;
        f32x4 bv = zero4();
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (f + e < H) bv[e] = a.b2[f + e];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const int row = j0 + 64 * wc + 16 * jt + c;
            if (row >= a.rows) continue;
            f32x4 v = acc[it][jt];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fr_elu(v[e] + bv[e]);
            float* pc = a.h2 + (long)row * Hp + f;
            if (f + 3 < H) {
                *reinterpret_cast<f32x4*>(pc) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (f + e < H) pc[e] = v[e];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ flow + ratio
// z_log_prob of latent l of one row (flow_fwd_kernel's arithmetic); `inside` = the call's torch.any flag
__device__ __forceinline__ float fr_zlp(const float* __restrict__ t, const float* __restrict__ e, int l, bool inside) {
    const float ev = e[l];
    const float lp = -(ev * ev) / 2.f - FLOW_HALF_LOG_2PI;
    if (!inside) return lp;
    float m[FLOW_L];
    flow_mask(e, m);
    FlowPdf s;
    flow_pdf(t + l * FLOW_L, m, s);
    float in = fabsf(ev) <= 1.f ? ev : 0.f;
    float ld = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const FlowStep st = flow_step(s, in);
        in = flow_out(st);
        ld += flow_lad(st);
    }
    return lp - ld;
}

struct FrRatioArgs {
    const float* ta;    // [2][M][n][100]  contexts of the a-calls
    const float* tb;    // [uc][M][2][n][100]
    const float* eps;   // [uc][M][4][n][10]
    const int* flags;   // [uc][M][4]
    const float* mask;  // [n][d]
    float* part;        // [uc][M][n]
    int n, d, M, u0, uc;
};

__global__ void __launch_bounds__(256) fr_ratio_kernel(FrRatioArgs a) {
    __shared__ float sh[2][256];
    const int tid = threadIdx.x;
    const long g = (long)blockIdx.x * FR_GROUPS + tid / FLOW_L;
    const int l = tid % FLOW_L;
    const long G = (long)a.uc * a.M * a.n;
    const bool live = tid < FR_GROUPS * FLOW_L && g < G;
    float dI = 0.f, dII = 0.f;
    bool in_loc = false;
    if (live) {
        const int i = (int)(g % a.n);
        const long um = g / a.n;  // (u - u0) M + m
        const int m = (int)(um % a.M), u = a.u0 + (int)(um / a.M);
        in_loc = a.mask[(long)i * a.d + u] == 0.f;
        if (in_loc) {
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const float* ea = a.eps + ((um * 4 + 2 * ch) * a.n + i) * FLOW_L;
                const float* eb = ea + (long)a.n * FLOW_L;
                const float* tA = a.ta + ((long)(ch * a.M + m) * a.n + i) * FLOW_CTX;
                const float* tB = a.tb + ((um * 2 + ch) * a.n + i) * FLOW_CTX;
                const float v = fabsf(fr_zlp(tA, ea, l, a.flags[um * 4 + 2 * ch] != 0) -
                                      fr_zlp(tB, eb, l, a.flags[um * 4 + 2 * ch + 1] != 0));
                if (ch == 0) dI = v; else dII = v;
            }
        }
    }
    sh[0][tid] = dI;
    sh[1][tid] = dII;
    __syncthreads();
    if (live && l == 0) {
        float sI = 0.f, sII = 0.f;
#pragma unroll
        for (int j = 0; j < FLOW_L; ++j) {
            sI += sh[0][tid + j];
            sII += sh[1][tid + j];
        }
        a.part[g] = sI - sII;  // KL_I - KL_II of sample m (evaluate.py:656-661)
    }
}

__global__ void __launch_bounds__(256) fr_reduce_kernel(const float* __restrict__ part, const float* __restrict__ mask,
                                                        float* __restrict__ R, int n, int d, int M, int u0, int uc) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)uc * n) return;
    const int i = (int)(e % n), ul = (int)(e / n), u = u0 + ul;
    float r = -1e4f;
    if (mask[(long)i * d + u] == 0.f) {
        float s = 0.f;
        for (int m = 0; m < M; ++m) s += part[((long)ul * M + m) * n + i];
        r = s / (float)M;
    }
    R[(long)i * (d - 1) + u] = r;
}

// ---- workspace layout (floats; every segment a multiple of 4 floats)
struct FrLayout {
    long xin, preA, h1a, h2a, ta, w1t, h2b, tb, eps, part, flags, total;
    int Hp;
};
static inline long fr_up4(long v) { return (v + 3) & ~3L; }
static bool fr_layout(int n, int d, int hid, int M, int chunk, FrLayout& l) {
    if (n < 1 || d < 2 || hid < 1 || hid > FR_MAX_HID || M < 1 || chunk < 1) return false;
    const long U = d - 1, uc = chunk < U ? chunk : U;
    const long ra = 2L * M * n, rb = uc * ra;
    if (rb > (1L << 30) || (long)n * d > (1L << 30) || U * M * 4 * n * FLOW_L > (1L << 40)) return false;
    l.Hp = (int)fr_up4(hid);
    long o = 0;
    auto seg = [&](long& field, long floats) { field = o; o += fr_up4(floats); };
    seg(l.xin, ra * 2 * d);
    seg(l.preA, ra * l.Hp);
    seg(l.h1a, ra * l.Hp);
    seg(l.h2a, ra * l.Hp);
    seg(l.ta, ra * FLOW_CTX);
    seg(l.w1t, U * 2 * l.Hp);
    seg(l.h2b, rb * l.Hp);
    seg(l.tb, rb * FLOW_CTX);
    seg(l.eps, uc * M * 4 * n * FLOW_L);
    seg(l.part, uc * M * n);
    seg(l.flags, uc * M * 4);
    l.total = o;
    return true;
}

static inline bool fr_ok() { return hipGetLastError() == hipSuccess; }

}  // namespace vpc

using namespace vpc;

extern "C" {

int vpc_flow_reward_scratch(int n, int d, int hid, int M, int chunk, long* scratch_floats) {
    FrLayout l;
    if (!scratch_floats || !fr_layout(n, d, hid, M, chunk, l)) return VPC_ERR_ARG;
    *scratch_floats = l.total;
    return VPC_OK;
}

int vpc_flow_reward_draws(float* eps, int n, int d, int M, unsigned long long seed, void* stream) {
    if (!eps || n < 1 || d < 2 || M < 1 || !aligned16(eps)) return VPC_ERR_ARG;
    const long total = (long)(d - 1) * M * 4 * n * FLOW_L;
    if (total > (1L << 40)) return VPC_ERR_ARG;
    const long groups = total / 4;  // the factor 4 (calls) makes the count a multiple of 4
    hipLaunchKernelGGL(fr_draws_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, eps,
                       total, (uint64_t)seed, (uint64_t)0);
    return fr_ok() ? VPC_OK : VPC_ERR_HIP;
}

int vpc_flow_reward_matrix(const float* x, const float* mask, const float* im, const float* We1, const float* be1,
                           const float* We2, const float* be2, const float* We3, const float* be3, const float* eps,
                           unsigned long long seed, float* scratch, long scratch_floats, float* R, int n, int d, int hid,
                           int M, int chunk, void* stream) {
    FrLayout l;
    if (!x || !mask || !im || !We1 || !be1 || !We2 || !be2 || !We3 || !be3 || !scratch || !R) return VPC_ERR_ARG;
    if (!fr_layout(n, d, hid, M, chunk, l) || scratch_floats < l.total || !aligned16(scratch)) return VPC_ERR_ARG;
    if (eps && !aligned16(eps)) return VPC_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int U = d - 1, H = hid, Hp = l.Hp;
    const long ra = 2L * M * n;
    float* S = scratch;
    // ---- the a-calls: inputs, first-layer pre-activations (kept for the b-rows) and contexts
    {
        const long e1 = ra * d, e2 = (long)U * 2 * Hp;
        const unsigned gm = (unsigned)((e1 + 255) / 256), gw = (unsigned)((e2 + 255) / 256);
        hipLaunchKernelGGL(fr_prep_kernel, dim3(gm + gw), dim3(256), 0, st, x, mask, im, We1, S + l.xin, S + l.w1t, n, d,
                           M, H, Hp, gm);
        if (!fr_ok()) return VPC_ERR_HIP;
    }
    if (Hp != H && hipMemsetAsync(S + l.preA, 0, (size_t)ra * Hp * sizeof(float), st) != hipSuccess) return VPC_ERR_HIP;
    int rc;
    if ((rc = vpc_linear_fwd(S + l.xin, 2 * d, We1, be1, S + l.preA, Hp, ra, H, 2 * d, 0, 0, 0, stream))) return rc;
    if ((rc = vpc_linear_fwd(S + l.xin, 2 * d, We1, be1, S + l.h1a, Hp, ra, H, 2 * d, 1, 0, 0, stream))) return rc;
    if ((rc = vpc_linear_fwd(S + l.h1a, Hp, We2, be2, S + l.h2a, Hp, ra, H, H, 1, 0, 0, stream))) return rc;
    if ((rc = vpc_linear_fwd(S + l.h2a, Hp, We3, be3, S + l.ta, FLOW_CTX, ra, FLOW_CTX, H, 0, 0, 0, stream))) return rc;

    constexpr size_t LDS = 2 * FR_TILE * sizeof(float);
    if (!lds_attr_done(reinterpret_cast<const void*>(&fr_trunk_kernel), LDS)) return VPC_ERR_HIP;
    const long per_u = (long)M * 4 * n * FLOW_L;  // draws of one candidate
    for (int u0 = 0; u0 < U; u0 += chunk) {
        const int uc = U - u0 < chunk ? U - u0 : chunk;
        const long rows = (long)uc * ra;
        const float* e = eps ? eps + u0 * per_u : S + l.eps;
        if (!eps) {
            const long cnt = uc * per_u;
            hipLaunchKernelGGL(fr_draws_kernel, dim3((unsigned)((cnt / 4 + 255) / 256)), dim3(256), 0, st, S + l.eps, cnt,
                               (uint64_t)seed, (uint64_t)(u0 * per_u / 4));
        }
        int* flags = reinterpret_cast<int*>(S + l.flags);
        hipLaunchKernelGGL(fr_flags_kernel, dim3((unsigned)(uc * M * 4)), dim3(64), 0, st, e, mask, flags, n, d, M, u0);
        FrTrunkArgs t{};
        t.W2 = We2; t.b2 = be2; t.preA = S + l.preA; t.w1t = S + l.w1t; t.im = im; t.h2 = S + l.h2b;
        t.n = n; t.d = d; t.M = M; t.H = H; t.Hp = Hp; t.u0 = u0; t.rows = (int)rows;
        t.vecW = aligned16(We2) && (H % 4) == 0;
        hipLaunchKernelGGL(fr_trunk_kernel, dim3((unsigned)((rows + 127) / 128), (unsigned)((H + 127) / 128)),
                           dim3(FR_THREADS), LDS, st, t);
        if (!fr_ok()) return VPC_ERR_HIP;
        if ((rc = vpc_linear_fwd(S + l.h2b, Hp, We3, be3, S + l.tb, FLOW_CTX, rows, FLOW_CTX, H, 0, 0, 0, stream)))
            return rc;
        FrRatioArgs r{};
        r.ta = S + l.ta; r.tb = S + l.tb; r.eps = e; r.flags = flags; r.mask = mask; r.part = S + l.part;
        r.n = n; r.d = d; r.M = M; r.u0 = u0; r.uc = uc;
        const long G = (long)uc * M * n;
        hipLaunchKernelGGL(fr_ratio_kernel, dim3((unsigned)((G + FR_GROUPS - 1) / FR_GROUPS)), dim3(256), 0, st, r);
        hipLaunchKernelGGL(fr_reduce_kernel, dim3((unsigned)(((long)uc * n + 255) / 256)), dim3(256), 0, st, S + l.part,
                           mask, R, n, d, M, u0, uc);
        if (!fr_ok()) return VPC_ERR_HIP;
    }
    return VPC_OK;
}

}  // extern "C"
