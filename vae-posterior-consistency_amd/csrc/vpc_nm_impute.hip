// Streaming importance-weighted imputation of the MNAR path (the llh_eval branch of REG_notMIWAE_v2.loss / notMIWAE_myversion.loss,
// src/models/VAE.py:2398-2461 / :2774-2813, as src/experiment_main/evaluate.py:13-69 calls it once per data row), fp32 (gfx950):
// encoder, sampler, decoder, the per-sample log-weight with the self-masking missingness model and the self-normalised weighted
// mean of the decoder's mean head in ONE kernel in the N-split shape of vpc_miw_impute.hip - one workgroup of 8 waves,
// v_mfma_f32_16x16x4_f32, the out tiles of a layer split over the waves, activations handed from layer to layer through LDS as
// [16 rows][SP] fp32, weights read from the model's flat parameter buffer (_NMBase._flat_spec order, row-major nn.Linear
// [out][in]) with range-checked fragment reads.  No decoder row is ever written to memory.
//
//   nm_impute_kernel        workgroup (row, chunk) owns data row `row` and the samples [chunk sc, min(S, (chunk + 1) sc)) of it.
//                           Encoder once on the row (xin = x * mask -> h1 -> h2 -> heads (mean | logvar), ELU between; the heads stay
//                           in LDS), then per 16-sample tile z = mean + eps_a * exp(logvar / 2) (draw requested a tile ahead) -> g1 ->
//                           g2 -> the head pair (Wxm | Wxl) as one [2 d][128] operand, whose epilogue writes xm = sigmoid(.) and
//                           xl = clamp(., -10, 0) to LDS straight from the accumulators; per sample the log-weight a_s = -l_w (32 lanes
//                           per sample, up to 4 columns each, a fixed lane tree); and an online softmax over the chunk, tile after
//                           tile: the tile's max over its live samples, one rescale, then lane k sums column k over the tile's
//                           samples in sample order.  (m, l, acc[0 .. d)) go to the partial slot (row, chunk).
//   nm_impute_merge_kernel  per row the chunks' partials combined in chunk order: xm = acc / l, lse = m + log l.
//
//   l_w = sum_k [ 0.5 log 2pi + 0.5 m_k xl_k + (m_k x_k - m_k xm_k)^2 / (2 exp(m_k xl_k)) ]       (VAE.py:2425 / :2788)
//       + KLterm
//       - sum_k [ m_k logit_k - softplus(logit_k) ],  logit_k = -softplus(W_k) (xm_k (1 - m_k) + x_k m_k - b_k)   (:2407-2435 / :2777-2802)
//   REG:  KLterm = sum_l 0.5 (exp(lv_l) + mu_l^2 - 1 - lv_l), once per workgroup; plane b of the draws is never read.
//   !REG: KLterm = sum_l [log N(z'; mu, sd) - log N(z'; 0, 1)] on z' = mu + eps_b * sd, the fresh rsample() of VAE.py:2791-2798.
//
// No float atomics, fixed orders: bit-reproducible for a given chunk length.  Only the q side enters (VAE.py:2458-2461: the
// imputation uses the q pass's weights and the q pass's x_mean), so there is no mask_p, no p pass and no alpha.
// The draws are those of vpc_miw_impute.hip (vpc_rng.h: miw_imp_normal, planes a / b = Philox streams 5 / 6);
// vpc_miw_impute_draws materialises them.
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_small_device.h"
#include "vpc_miw_chain.h"
#include "vpc_nm_device.h"
#include "vpc_rng.h"

#include <cmath>

namespace vpc {

constexpr int NM_IMP_MAX_D = 128, NM_IMP_MAX_L = 16;

struct NmImputeArgs {
    const float* prm;   // flat parameters
    const float* x;     // [B][d]
    const float* mask;  // [B][d] 0 / 1 floats
    const float* eps;   // [2][B][S][L] injected draws (a | b) or nullptr: Philox
    float* part;        // [B][nchunk][2 + d]  (m, l, acc)
    uint64_t seed, offset;
    long row0;          // global index of row 0 (the draw counters' row)
    int B, S, d, L, sc, nchunk;  // sc: chunk length (a multiple of 16)
};

// offsets of the tensors in the flat parameter buffer: [W b | We1 be1 We2 be2 (Wmu Wls) (bmu bls) | Wd1 bd1 Wd2 bd2 (Wxm Wxl) (bxm bxl)]
struct NmOff {
    int W, b, We1, be1, We2, be2, Wh, bh, Wd1, bd1, Wd2, bd2, Wx, bx, n;
    __host__ __device__ NmOff(int d, int L) {
        int o = 0;
        W = o; o += d;
        b = o; o += d;
        We1 = o; o += MIW_HID * d;
        be1 = o; o += MIW_HID;
        We2 = o; o += MIW_HID * MIW_HID;
        be2 = o; o += MIW_HID;
        Wh = o; o += 2 * L * MIW_HID;
        bh = o; o += 2 * L;
        Wd1 = o; o += MIW_HID * L;
        bd1 = o; o += MIW_HID;
        Wd2 = o; o += MIW_HID * MIW_HID;
        bd2 = o; o += MIW_HID;
        Wx = o; o += 2 * d * MIW_HID;
        bx = o; o += 2 * d;
        n = o;
    }
};

// eps[plane][row][s][l]: the injected tensor or the counter rule of vpc_rng.h - one path for both
__device__ __forceinline__ float nm_imp_draw(const NmImputeArgs& a, int plane, int row, int s, int l) {
    if (a.eps) return a.eps[(((long)plane * a.B + row) * a.S + s) * a.L + l];
    return miw_imp_normal(a.seed, a.offset, plane, a.row0 + row, s, l);
}

__device__ __forceinline__ f32x4 nm_elu4(f32x4 v) {  // ELU(alpha = 1)
    return f32x4{v[0] > 0.f ? v[0] : expm1f(v[0]), v[1] > 0.f ? v[1] : expm1f(v[1]), v[2] > 0.f ? v[2] : expm1f(v[2]),
                 v[3] > 0.f ? v[3] : expm1f(v[3])};
}

// LDS: six activation buffers - A: xin, then z; B: h1, then g1; C: h2, then g2; HD: the encoder's heads (row 0 is the data row);
// XM / XL: the tile's sigmoid(mean head) / clamped logvar head - and behind them the tile's 16 log-weights
enum { NI_A = 0, NI_B, NI_C, NI_HD, NI_XM, NI_XL, NI_COUNT };
static_assert((NI_COUNT * SBUF + 16) * 4 <= 65536, "static LDS");

// HT = out tiles of the 2 d decoder heads per wave (1: 2 d <= 128, 2), LT = tiles of the 2 L encoder heads (1, 2), REG: the class
template <int HT, int LT, bool REG>
__global__ __launch_bounds__(THREADS) void nm_impute_kernel(NmImputeArgs a) {
    constexpr int CT = 2 * HT;  // columns of a log-weight lane: 32 lanes per sample
    __shared__ __attribute__((aligned(16))) float lds[NI_COUNT * SBUF + 16];
    auto buf = [&](int b) { return lds + b * SBUF; };
    float* lw_t = lds + NI_COUNT * SBUF;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, q = lane >> 4;
    const int d = a.d, L = a.L;
    const NmOff o(d, L);
    const float* P = a.prm;
    const int row = blockIdx.x / a.nchunk, chunk = blockIdx.x - row * a.nchunk;
    const int s0 = chunk * a.sc;
    const int ns = a.S - s0 < a.sc ? a.S - s0 : a.sc;  // >= 1: nchunk = ceil(S / sc)
    const float* xr = a.x + (long)row * d;
    const float* mr = a.mask + (long)row * d;
    const int yt = (2 * d + 15) >> 4;  // out tiles of the decoder heads
    int cc = c, qq = q;
    // ================================================================ encoder: one tile, row 0 live
    {
        f32x4 fW1[8], fW2[8], fW3[8];
        miw_ldA<8>(P + o.We1, MIW_HID, d, w, cc, qq, fW1);
        for (int i = tid; i < 16 * MIW_HID; i += THREADS) {
            const int r = i >> 7, f = i & 127;
            buf(NI_A)[r * SP + f] = (r == 0 && f < d) ? xr[f] * mr[f] : 0.f;
        }
        miw_ldA<8>(P + o.We2, MIW_HID, MIW_HID, w, cc, qq, fW2);
        lds_barrier();
        launder(cc, qq);
        st_act(buf(NI_B), w, cc, qq, nm_elu4(miw_mm<8>(fW1, buf(NI_A), cc, qq, miw_bias(P + o.be1, MIW_HID, w, qq))));
        if (w < LT) miw_ldA<8>(P + o.Wh, 2 * L, MIW_HID, w, cc, qq, fW3);
        lds_barrier();
        launder(cc, qq);
        st_act(buf(NI_C), w, cc, qq, nm_elu4(miw_mm<8>(fW2, buf(NI_B), cc, qq, miw_bias(P + o.be2, MIW_HID, w, qq))));
        lds_barrier();
        launder(cc, qq);
        if (w < LT)  // heads -> (mean | logvar), no activation
            st_act(buf(NI_HD), w, cc, qq, miw_mm<8>(fW3, buf(NI_C), cc, qq, miw_bias(P + o.bh, 2 * L, w, qq)));
        lds_barrier();
        launder(cc, qq);
    }
    // the decoder's fragments do not change from tile to tile: requested once, here
    f32x4 fW4[1], fW5[8], fW6[HT][8], bias6[HT];
    miw_ldA<1>(P + o.Wd1, MIW_HID, L, w, cc, qq, fW4);
    miw_ldA<8>(P + o.Wd2, MIW_HID, MIW_HID, w, cc, qq, fW5);
    const f32x4 bias4 = miw_bias(P + o.bd1, MIW_HID, w, qq), bias5 = miw_bias(P + o.bd2, MIW_HID, w, qq);
#pragma unroll
    for (int h = 0; h < HT; ++h) {  // (tiles past yt: rows past 2 d, zeros)
        miw_ldA<8>(P + o.Wx, 2 * d, MIW_HID, w + 8 * h, cc, qq, fW6[h]);
        bias6[h] = miw_bias(P + o.bx, 2 * d, w + 8 * h, qq);
    }
    // ================================================================ the chunk's ns samples in tiles of 16
    // sampler: thread (zr, zl) of waves 0 .. 3.  Log-weight: thread (lr, lk), 32 lanes per sample: columns lk + 32 i of x / mask /
    // the missingness model / the decoder heads, and latent lk of the KL term.  Softmax: thread k < d owns column k.
    const int zr = tid >> 4, zl = tid & 15;
    const bool zown = tid < 256 && zl < L;
    const float zmu = zown ? buf(NI_HD)[zl] : 0.f, zsd = zown ? expf(0.5f * buf(NI_HD)[L + zl]) : 0.f;
    const int lr = tid >> 5, lk = tid & 31;
    const bool kl = lk < L;
    const float lmu = kl ? buf(NI_HD)[lk] : 0.f, llv = kl ? buf(NI_HD)[L + lk] : 0.f;
    const float lsd = expf(0.5f * llv);
    float xk[CT], mk[CT], spk[CT], bk[CT];
#pragma unroll
    for (int i = 0; i < CT; ++i) {
        const int k = lk + 32 * i;
        const bool ok = k < d;
        xk[i] = ok ? xr[k] : 0.f;
        mk[i] = ok ? mr[k] : 0.f;
        spk[i] = ok ? softplus_f(P[o.W + k]) : 0.f;
        bk[i] = ok ? P[o.b + k] : 0.f;
    }
    auto tree32 = [](float v) {  // the sample's 32 lanes (one half of a wave), every lane gets the sum
        for (int of = 16; of > 0; of >>= 1) v += __shfl_xor(v, of, 64);
        return v;
    };
    // what a sample's log-weight has whatever the draw: the Gaussian constant of all d columns and, REG, the analytic KL
    float lw_const = NM_HALF_LOG_2PI * (float)d;
    if (REG) lw_const += tree32(kl ? 0.5f * (expf(llv) + lmu * lmu - 1.f - llv) : 0.f);
    auto eps_a = [&](int t0) { return (zown && t0 + zr < ns) ? nm_imp_draw(a, 0, row, s0 + t0 + zr, zl) : 0.f; };
    auto eps_b = [&](int t0) { return (!REG && kl && t0 + lr < ns) ? nm_imp_draw(a, 1, row, s0 + t0 + lr, lk) : 0.f; };
    const bool kown = tid < d;  // (d <= 128: waves 0 and 1)
    float m_run = -INFINITY, l_run = 0.f, acc = 0.f;
    float e_next = eps_a(0);
    for (int t0 = 0; t0 < ns; t0 += 16) {
        const int nl = ns - t0 < 16 ? ns - t0 : 16;  // live samples of the tile
        if (tid < 256) buf(NI_A)[zr * SP + zl] = (zown && zr < nl) ? zmu + e_next * zsd : 0.f;
        lds_barrier();
        launder(cc, qq);
        e_next = eps_a(t0 + 16);
        const float eb = eps_b(t0);
        st_act(buf(NI_B), w, cc, qq, nm_elu4(miw_mm<1>(fW4, buf(NI_A), cc, qq, bias4)));
        lds_barrier();
        launder(cc, qq);
        st_act(buf(NI_C), w, cc, qq, nm_elu4(miw_mm<8>(fW5, buf(NI_B), cc, qq, bias5)));
        lds_barrier();
        launder(cc, qq);
#pragma unroll
        for (int h = 0; h < HT; ++h) {
            const int mt = w + 8 * h;
            if (mt < yt) {  // (wave-uniform) features < d: the mean head, d .. 2 d - 1: the logvar head
                const f32x4 v = miw_mm<8>(fW6[h], buf(NI_C), cc, qq, bias6[h]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = 16 * mt + 4 * qq + j;
                    if (f < d) buf(NI_XM)[cc * SP + f] = sigmoid_f(v[j]);
                    else if (f < 2 * d) buf(NI_XL)[cc * SP + f - d] = fminf(fmaxf(v[j], -10.f), 0.f);
                }
            }
        }
        lds_barrier();
        launder(cc, qq);
        {
            const bool live = lr < nl;  // a dead sample's rows are never read
            float s = 0.f;
            if (live) {
#pragma unroll
                for (int i = 0; i < CT; ++i) {
                    const int k = lk + 32 * i;
                    if (k < d) {
                        const float xm = buf(NI_XM)[lr * SP + k], mxl = mk[i] * buf(NI_XL)[lr * SP + k];
                        const float r = mk[i] * xk[i] - mk[i] * xm;
                        const float lg = -spk[i] * (xm * (1.f - mk[i]) + xk[i] * mk[i] - bk[i]);
                        s += 0.5f * mxl + 0.5f * r * r * expf(-mxl) + (softplus_f(lg) - mk[i] * lg);
                    }
                }
                if (!REG && kl) {  // log N(z'; mu, sd) - log N(z'; 0, 1) on the fresh draw
                    const float z = lmu + eb * lsd;
                    s += -0.5f * eb * eb - 0.5f * llv + 0.5f * z * z;
                }
            }
            s = tree32(s);
            if (live && lk == 0) lw_t[lr] = -(s + lw_const);
        }
        lds_barrier();
        launder(cc, qq);
        if (kown) {  // online softmax, a tile at a time: the tile's max, one rescale, the samples in order
            float tm = lw_t[0];
            for (int s = 1; s < nl; ++s) tm = fmaxf(tm, lw_t[s]);
            if (tm > m_run) {  // (workgroup-uniform)
                const float r = expf(m_run - tm);
                l_run *= r;
                acc *= r;
                m_run = tm;
            }
            for (int s = 0; s < nl; ++s) {
                const float wgt = expf(lw_t[s] - m_run);
                l_run += wgt;
                acc += wgt * buf(NI_XM)[s * SP + tid];
            }
        }
        // (no barrier: the next tile's first write to XM / XL / lw_t lies behind three barriers every reader of this tile has passed)
    }
    if (kown) {
        float* p = a.part + ((long)row * a.nchunk + chunk) * (2 + d);
        if (tid == 0) {
            p[0] = m_run;
            p[1] = l_run;
        }
        p[2 + tid] = acc;
    }
}

// one 128-thread workgroup per row, thread k: column k.  The chunks' (m, l, acc) in chunk order.
__global__ __launch_bounds__(128) void nm_impute_merge_kernel(const float* __restrict__ part, int nchunk, int d,
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

}  // namespace vpc

using namespace vpc;

namespace {

typedef void (*NmImputeKernel)(NmImputeArgs);
// <HT, LT, REG>: two head tiles per wave past 2 d = 128, two tiles of encoder heads past 2 L = 16, the model class
NmImputeKernel nm_impute_pick(int d, int L, int regularised) {
    switch ((2 * d > 128 ? 4 : 0) | (2 * L > 16 ? 2 : 0) | (regularised ? 1 : 0)) {
        case 0: return nm_impute_kernel<1, 1, false>;
        case 1: return nm_impute_kernel<1, 1, true>;
        case 2: return nm_impute_kernel<1, 2, false>;
        case 3: return nm_impute_kernel<1, 2, true>;
        case 4: return nm_impute_kernel<2, 1, false>;
        case 5: return nm_impute_kernel<2, 1, true>;
        case 6: return nm_impute_kernel<2, 2, false>;
        default: return nm_impute_kernel<2, 2, true>;
    }
}

constexpr int NM_IMP_MAX_S = 1 << 28;  // 4 s + group stays inside the low counter word with room to spare

// chunk length in samples (a multiple of 16) and chunks per row; false outside the limits
bool nm_impute_plan(long B, int S, int d, int L, int s_chunk, int* sc, long* nchunk) {
    if (B < 1 || S < 1 || S > NM_IMP_MAX_S || d < 1 || d > NM_IMP_MAX_D || L < 1 || L > NM_IMP_MAX_L || s_chunk < 1) return false;
    const int c = s_chunk < S ? s_chunk : S;
    *sc = (c + 15) / 16 * 16;
    *nchunk = (S + *sc - 1) / *sc;
    return B <= 0x7fffffffL && B * *nchunk <= 0x7fffffffL;
}
bool nm_impute_counters_ok(uint64_t offset, long row0, long B) {
    return row0 >= 0 && offset <= 0xffffffffull && offset + (uint64_t)row0 + (uint64_t)B <= 0x100000000ull;
}

}  // namespace

extern "C" {

long vpc_nm_impute_scratch(long B, int S, int d, int L, int s_chunk) {
    int sc;
    long nchunk;
    if (!nm_impute_plan(B, S, d, L, s_chunk, &sc, &nchunk)) return 0;
    return B * nchunk * (2 + d);
}

int vpc_nm_impute(const float* params, const float* x, const float* mask, const float* eps, unsigned long long seed,
                  unsigned long long offset, long row0, float* part, long part_floats, float* xm, float* lse, long B, int S,
                  int d, int L, int s_chunk, int regularised, void* stream) {
    int sc;
    long nchunk;
    if (!nm_impute_plan(B, S, d, L, s_chunk, &sc, &nchunk)) return VPC_ERR_ARG;
    if (!params || !x || !mask || !part || !xm) return VPC_ERR_ARG;
    if (part_floats < B * nchunk * (2 + d)) return VPC_ERR_ARG;
    if (!eps && !nm_impute_counters_ok(offset, row0, B)) return VPC_ERR_ARG;
    NmImputeArgs a{};
    a.prm = params; a.x = x; a.mask = mask; a.eps = eps; a.part = part;
    a.seed = seed; a.offset = offset; a.row0 = row0;
    a.B = (int)B; a.S = S; a.d = d; a.L = L; a.sc = sc; a.nchunk = (int)nchunk;
    hipLaunchKernelGGL(nm_impute_pick(d, L, regularised), dim3((unsigned)(B * nchunk)), dim3(THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(nm_impute_merge_kernel, dim3((unsigned)B), dim3(128), 0, (hipStream_t)stream, part, (int)nchunk, d, xm,
                       lse);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
