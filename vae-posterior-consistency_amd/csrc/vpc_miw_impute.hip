// Streaming importance-weighted imputation of the MIWAE path (the llh_eval branch of MIWAE.loss / Reg_MIWAE.loss,
// src/models/VAE.py:3078-3099 / :3204-3258, as src/experiment_main/evaluate.py:89-113 calls it once per data row), fp32
// (gfx950): encoder, sampler, decoder, the per-sample log-weight and the self-normalised weighted mean of the decoder's
// mean head in ONE kernel in the N-split shape of vpc_miw_small.hip - one workgroup of 8 waves, v_mfma_f32_16x16x4_f32,
// the 8 output tiles of a 128-wide layer one per wave, activations handed from layer to layer through LDS as
// [16 rows][SP] fp32, weights read from the flat parameter buffer (row-major nn.Linear [out][in], state_dict order) with
// range-checked fragment reads.  No decoder row is ever written to memory.
//
//   miw_impute_kernel        workgroup (row, chunk) owns data row `row` and the samples [chunk sc, min(S, (chunk + 1) sc)) of
//                            it.  Encoder once on the row (xin = x * mask -> h1 -> h2 -> heads, hact = (mean | softplus) stays in
//                            LDS), then per 16-sample tile z = mean + eps_a * scale (draw requested a tile ahead) -> g1 -> g2 ->
//                            raw heads Y in LDS; per sample the log-weight of the per-row pairing as vpc_miw_loss (raw = 1,
//                            VPC_MIW_PAIR_PER_ROW) forms it, with the prior / posterior term on z' = mean + eps_b * scale, a
//                            second, independent draw (the reference's fresh rsample() of VAE.py:3087 / :3216); and an online
//                            softmax over the chunk, sample after sample: running max m, running sum l, acc[k] += w * sigmoid(Y_k),
//                            rescaled on a new max (wave 7, one tile behind the GEMMs: it has no out tile in the Y stage).
//                            (m, l, acc[0 .. d)) go to the partial slot (row, chunk).
//   miw_impute_merge_kernel  per row the chunks' partials combined in chunk order: xm = acc / l, lse = m + log l.
//   miw_impute_draws_kernel  the draws of a seeded call as [2][B][S][L] (a | b): same function, same values.
//
// No float atomics, fixed orders: bit-reproducible for a given chunk length.  Only the q side enters (VAE.py:3255-3257: the
// imputation of Reg_MIWAE uses the q pass's weights and the q pass's x_mean), so mask_p is no argument.
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_small_device.h"
#include "vpc_miw_device.h"
#include "vpc_miw_chain.h"
#include "vpc_rng.h"

#include <cmath>

namespace vpc {

struct MiwImputeArgs {
    const float* prm;   // flat parameters
    const float* x;     // [B][d]
    const float* mask;  // [B][d] 0 / 1 floats
    const float* eps;   // [2][B][S][L] injected draws (a | b) or nullptr: Philox
    float* part;        // [B][nchunk][2 + d]  (m, l, acc)
    uint64_t seed, offset;
    long row0;          // global index of row 0 (the draw counters' row)
    int B, S, d, L, sc, nchunk, cpl;  // sc: chunk length (a multiple of 16); 1 << cpl >= max(d, L): lanes per sample
};

// eps[plane][row][s][l]: the injected tensor or the counter rule of vpc_rng.h - one path for both
__device__ __forceinline__ float miw_imp_draw(const MiwImputeArgs& a, int plane, int row, int s, int l) {
    if (a.eps) return a.eps[(((long)plane * a.B + row) * a.S + s) * a.L + l];
    return miw_imp_normal(a.seed, a.offset, plane, a.row0 + row, s, l);
}

// LDS: five activation buffers - A: xin, then z; B: h1, then g1; C: h2, then g2; HD: hact (row 0 is the data row); Y: raw
// decoder heads - and behind them the tile's 16 log-weights and its [16][32] sigmoid(mean head)
enum { I_A = 0, I_B, I_C, I_HD, I_Y, I_COUNT };
constexpr int I_TAIL = 16 + 16 * 32;
static_assert((I_COUNT * SBUF + I_TAIL) * 4 <= 65536, "static LDS");

// running (m, l, acc) of wave 7, lane k: the nl samples of the tile in LDS, one after another
__device__ __forceinline__ void miw_imp_online(const float* lw, const float* sg, int nl, int k, float& m, float& l, float& acc) {
    for (int s = 0; s < nl; ++s) {
        const float v = lw[s];
        if (v > m) {  // (wave-uniform) a new max: rescale what has been summed
            const float r = expf(m - v);
            l *= r;
            acc *= r;
            m = v;
        }
        const float wgt = expf(v - m);
        l += wgt;
        acc += wgt * sg[s * 32 + k];
    }
}

// YT = tiles of the 3 d decoder heads (1 .. 6), LT = tiles of the 2 L encoder heads (1, 2); DT = tiles of d
template <int YT, int LT>
__global__ __launch_bounds__(THREADS) void miw_impute_kernel(MiwImputeArgs a) {
    constexpr int DT = YT <= 3 ? 1 : 2;
    __shared__ __attribute__((aligned(16))) float lds[I_COUNT * SBUF + I_TAIL];
    auto buf = [&](int b) { return lds + b * SBUF; };
    float* lw_t = lds + I_COUNT * SBUF;
    float* sg_t = lw_t + 16;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, q = lane >> 4;
    const int d = a.d, L = a.L;
    const MiwOff o(d, L);
    const float* P = a.prm;
    const int row = blockIdx.x / a.nchunk, chunk = blockIdx.x - row * a.nchunk;
    const int s0 = chunk * a.sc;
    const int ns = a.S - s0 < a.sc ? a.S - s0 : a.sc;  // >= 1: nchunk = ceil(S / sc)
    const float* xr = a.x + (long)row * d;
    const float* mr = a.mask + (long)row * d;
    int cc = c, qq = q;
    // ================================================================ encoder: one tile, row 0 live
    f32x4 fW1[DT], fW2[8], fW3[8];
    miw_ldA<DT>(P + o.We1, MIW_HID, d, w, cc, qq, fW1);
    for (int i = tid; i < 256 * DT; i += THREADS) {
        const int r = i / (16 * DT), f = i - r * 16 * DT;
        buf(I_A)[r * SP + f] = (r == 0 && f < d) ? xr[f] * mr[f] : 0.f;
    }
    miw_ldA<8>(P + o.We2, MIW_HID, MIW_HID, w, cc, qq, fW2);
    lds_barrier();
    launder(cc, qq);
    st_act(buf(I_B), w, cc, qq, relu4(miw_mm<DT>(fW1, buf(I_A), cc, qq, miw_bias(P + o.be1, MIW_HID, w, qq))));
    if (w < LT) miw_ldA<8>(P + o.Wh, 2 * L, MIW_HID, w, cc, qq, fW3);
    lds_barrier();
    launder(cc, qq);
    st_act(buf(I_C), w, cc, qq, relu4(miw_mm<8>(fW2, buf(I_B), cc, qq, miw_bias(P + o.be2, MIW_HID, w, qq))));
    // the decoder's fragments do not change from tile to tile: requested once, here
    f32x4 fW4[1], fW5[8], fW6[8];
    miw_ldA<1>(P + o.Wd1, MIW_HID, L, w, cc, qq, fW4);
    miw_ldA<8>(P + o.Wd2, MIW_HID, MIW_HID, w, cc, qq, fW5);
    if (w < YT) miw_ldA<8>(P + o.Wx, 3 * d, MIW_HID, w, cc, qq, fW6);
    const f32x4 bias4 = miw_bias(P + o.bd1, MIW_HID, w, qq), bias5 = miw_bias(P + o.bd2, MIW_HID, w, qq);
    const f32x4 bias6 = miw_bias(P + o.bx, 3 * d, w < YT ? w : 0, qq);
    lds_barrier();
    launder(cc, qq);
    if (w < LT) {  // heads -> (mean | softplus(raw)) in LDS
        const f32x4 v = miw_mm<8>(fW3, buf(I_C), cc, qq, miw_bias(P + o.bh, 2 * L, w, qq));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = 16 * w + 4 * qq + j;
            buf(I_HD)[cc * SP + f] = f < L ? v[j] : miw_softplus(v[j]);
        }
    }
    lds_barrier();
    launder(cc, qq);
    // ================================================================ the chunk's ns samples in tiles of 16
    // sampler: thread (zr, zl) of waves 0 .. 3.  Log-weight: thread (lr, lk), 1 << cpl lanes per sample, of the first 16 << cpl
    // threads: column lk of x / mask / the decoder heads and latent lk of the fresh draw
    const int zr = tid >> 4, zl = tid & 15;
    const bool zown = tid < 256 && zl < L;
    const float zmu = zown ? buf(I_HD)[zl] : 0.f, zsc = zown ? buf(I_HD)[L + zl] : 0.f;
    const int cp = 1 << a.cpl, lr = tid >> a.cpl, lk = tid & (cp - 1);
    const bool lwave = 64 * w < 16 * cp;  // this wave holds log-weight lanes (wave-uniform)
    const bool lown = tid < 16 * cp;
    const bool kd = lown && lk < d, kl = lown && lk < L;
    const float xk = kd ? xr[lk] : 0.f, mk = kd ? mr[lk] : 0.f;
    const float lmu = kl ? buf(I_HD)[lk] : 0.f, lsc = kl ? buf(I_HD)[L + lk] : 1.f;
    auto eps_a = [&](int t0) { return (zown && t0 + zr < ns) ? miw_imp_draw(a, 0, row, s0 + t0 + zr, zl) : 0.f; };
    auto eps_b = [&](int t0) { return (kl && t0 + lr < ns) ? miw_imp_draw(a, 1, row, s0 + t0 + lr, lk) : 0.f; };
    float m_run = -INFINITY, l_run = 0.f, acc = 0.f;  // wave 7, lane k < 32: column k
    float e_next = eps_a(0);
    for (int t0 = 0; t0 < ns; t0 += 16) {
        if (tid < 256) buf(I_A)[zr * SP + zl] = (zown && t0 + zr < ns) ? zmu + e_next * zsc : 0.f;
        lds_barrier();
        launder(cc, qq);
        e_next = eps_a(t0 + 16);
        const float eb = eps_b(t0);
        st_act(buf(I_B), w, cc, qq, relu4(miw_mm<1>(fW4, buf(I_A), cc, qq, bias4)));
        lds_barrier();
        launder(cc, qq);
        st_act(buf(I_C), w, cc, qq, relu4(miw_mm<8>(fW5, buf(I_B), cc, qq, bias5)));
        lds_barrier();
        launder(cc, qq);
        if (w < YT) {
            st_act(buf(I_Y), w, cc, qq, miw_mm<8>(fW6, buf(I_C), cc, qq, bias6));
        } else if (w == 7 && t0 > 0) {  // the tile before this one (full: it has a successor)
            if (lane < 32) miw_imp_online(lw_t, sg_t, 16, lane, m_run, l_run, acc);
        }
        lds_barrier();
        launder(cc, qq);
        if (lwave) {
            // sum_k mask[k] * StudentT(x[k]; heads of sample lr) and sum_l (log N(z'; 0, 1) - log N(z'; mean, scale)): the
            // expressions of miw_rows_kernel
            float so = 0.f, slw = 0.f;
            if (kd) {
                const MiwHead h = miw_head(buf(I_Y) + lr * SP, d, lk, 1);
                so = miw_student_lp(xk, h) * mk;
                sg_t[lr * 32 + lk] = h.mu;
            }
            if (kl) {
                const float z = lmu + lsc * eb;
                const float dz = z - lmu;
                const float lpz = -0.5f * z * z - MIW_HALF_LOG_2PI;
                const float lq = -(dz * dz) / (2.f * lsc * lsc) - logf(lsc) - MIW_HALF_LOG_2PI;
                slw = lpz - lq;
            }
            for (int of = cp >> 1; of > 0; of >>= 1) {
                so += __shfl_xor(so, of, 64);
                slw += __shfl_xor(slw, of, 64);
            }
            if (lown && lk == 0) lw_t[lr] = so + slw;
        }
        // (no barrier: the next tile's first write to a buffer lies behind a barrier every reader of this tile has passed;
        // lw_t / sg_t are read by wave 7 in the next Y stage and written again behind that stage's barrier)
    }
    lds_barrier();
    if (w == 7 && lane < 32) {
        const int tl = (ns - 1) & ~15;  // the last tile: ns - tl live samples, dead ones contribute nothing
        miw_imp_online(lw_t, sg_t, ns - tl, lane, m_run, l_run, acc);
        float* p = a.part + ((long)row * a.nchunk + chunk) * (2 + d);
        if (lane == 0) {
            p[0] = m_run;
            p[1] = l_run;
        }
        if (lane < d) p[2 + lane] = acc;
    }
}

// one 64-thread workgroup per row, thread k: column k.  The chunks' (m, l, acc) in chunk order.
__global__ __launch_bounds__(64) void miw_impute_merge_kernel(const float* __restrict__ part, int nchunk, int d,
                                                              float* __restrict__ xm, float* __restrict__ lse) {
    const long row = blockIdx.x;
    const int k = threadIdx.x;
    const bool kd = k < d;
    const float* p = part + row * nchunk * (2 + d);
    float m = p[0], l = p[1], acc = kd ? p[2 + k] : 0.f;
    for (int ch = 1; ch < nchunk; ++ch) {
        const float* pc = p + (long)ch * (2 + d);
        const float mc = pc[0], lc = pc[1], ac = kd ? pc[2 + k] : 0.f;
        const float mx = fmaxf(m, mc);
        const float f0 = expf(m - mx), f1 = expf(mc - mx);
        l = l * f0 + lc * f1;
        acc = acc * f0 + ac * f1;
        m = mx;
    }
    if (kd) xm[row * d + k] = acc / l;
    if (k == 0 && lse) lse[row] = m + logf(l);
}

// out[plane][row][s][l], n = 2 B S L elements: one thread per element
__global__ void miw_impute_draws_kernel(float* __restrict__ out, long n, long B, int S, int L, uint64_t seed, uint64_t offset,
                                        long row0) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int l = (int)(i % L);
    const long r = i / L;
    const int s = (int)(r % S);
    const long pr = r / S;
    const int plane = (int)(pr / B);
    out[i] = miw_imp_normal(seed, offset, plane, row0 + (pr - plane * B), s, l);
}

}  // namespace vpc

using namespace vpc;

namespace {

typedef void (*MiwImputeKernel)(MiwImputeArgs);
template <int LT>
MiwImputeKernel miw_impute_pick_y(int yt) {
    switch (yt) {
        case 1: return miw_impute_kernel<1, LT>;
        case 2: return miw_impute_kernel<2, LT>;
        case 3: return miw_impute_kernel<3, LT>;
        case 4: return miw_impute_kernel<4, LT>;
        case 5: return miw_impute_kernel<5, LT>;
        default: return miw_impute_kernel<6, LT>;
    }
}
MiwImputeKernel miw_impute_pick(int d, int L) {
    const int yt = (3 * d + 15) / 16;
    return 2 * L <= 16 ? miw_impute_pick_y<1>(yt) : miw_impute_pick_y<2>(yt);
}

constexpr int MIW_IMP_MAX_S = 1 << 28;  // 4 s + group stays inside the low counter word with room to spare

// chunk length in samples (a multiple of 16) and chunks per row; false outside the limits
bool miw_impute_plan(long B, int S, int d, int L, int s_chunk, int* sc, long* nchunk) {
    if (B < 1 || S < 1 || S > MIW_IMP_MAX_S || d < 1 || d > MIW_SMALL_MAX_D || L < 1 || L > MIW_SMALL_MAX_L || s_chunk < 1)
        return false;
    const int c = s_chunk < S ? s_chunk : S;
    *sc = (c + 15) / 16 * 16;
    *nchunk = (S + *sc - 1) / *sc;
    return B * *nchunk <= 0x7fffffffL;
}
bool miw_impute_counters_ok(uint64_t offset, long row0, long B) {
    return row0 >= 0 && offset <= 0xffffffffull && offset + (uint64_t)row0 + (uint64_t)B <= 0x100000000ull;
}

}  // namespace

extern "C" {

long vpc_miw_impute_scratch(long B, int S, int d, int L, int s_chunk) {
    int sc;
    long nchunk;
    if (!miw_impute_plan(B, S, d, L, s_chunk, &sc, &nchunk)) return 0;
    return B * nchunk * (2 + d);
}

int vpc_miw_impute(const float* params, const float* x, const float* mask, const float* eps, unsigned long long seed,
                   unsigned long long offset, long row0, float* part, long part_floats, float* xm, float* lse, long B, int S,
                   int d, int L, int s_chunk, void* stream) {
    int sc;
    long nchunk;
    if (!miw_impute_plan(B, S, d, L, s_chunk, &sc, &nchunk)) return VPC_ERR_ARG;
    if (!params || !x || !mask || !part || !xm) return VPC_ERR_ARG;
    if (part_floats < B * nchunk * (2 + d)) return VPC_ERR_ARG;
    if (!eps && !miw_impute_counters_ok(offset, row0, B)) return VPC_ERR_ARG;
    MiwImputeArgs a{};
    a.prm = params; a.x = x; a.mask = mask; a.eps = eps; a.part = part;
    a.seed = seed; a.offset = offset; a.row0 = row0;
    a.B = (int)B; a.S = S; a.d = d; a.L = L; a.sc = sc; a.nchunk = (int)nchunk;
    const int width = d > L ? d : L;
    while ((1 << a.cpl) < width) ++a.cpl;
    hipLaunchKernelGGL(miw_impute_pick(d, L), dim3((unsigned)(B * nchunk)), dim3(THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(miw_impute_merge_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, part, (int)nchunk, d, xm,
                       lse);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_impute_draws(float* eps_out, long B, int S, int L, unsigned long long seed, unsigned long long offset, long row0,
                         void* stream) {
    if (!eps_out || B < 1 || S < 1 || S > MIW_IMP_MAX_S || L < 1 || L > MIW_SMALL_MAX_L) return VPC_ERR_ARG;
    if (!miw_impute_counters_ok(offset, row0, B)) return VPC_ERR_ARG;
    const long n = 2 * B * S * L;
    const long blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffL) return VPC_ERR_ARG;
    hipLaunchKernelGGL(miw_impute_draws_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, eps_out, n, B, S, L,
                       (uint64_t)seed, (uint64_t)offset, row0);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
