// Evaluate-stage forward of an ensemble, fp32 (gfx950): G members x (MC pass x batch x 16-row tile) in one launch, and the
// launch that turns the tile records into the four numbers eval_vae reports.
//
// Reference semantics: the loop body of eval_vae (src/experiment_main/evaluate.py:136-297) for Reg_VAE / vanilla_VAE: model.forward
// (src/models/VAE.py:496-507; :1153-1169) -> model.loss(llh_eval=True, stage='evaluate') (VAE.py:410-420: only the q pass reaches an
// output; mask_p, alpha and the p pass do not) -> the RMSE on ~mask (evaluate.py:229-234), then the mean over the batches of a pass
// and over the M passes (evaluate.py:238-245).
//
// eval_small_kernel: one workgroup of 8 waves per 16-row tile, the feature tiles of a layer split over the waves as in
// step_small_kernel (vpc_small.hip): stage order, MFMA shapes and the one-stage-ahead weight-fragment requests are those of phase
// "E" (pass 0) and of the decoder forward of the tile body (vpc_small_body.h), the helpers those of vpc_small_device.h.  Seven
// activation buffers (X, H1, H2, ML, Z, G1, G2) of 9 216 bytes: two workgroups per CU.  A tile lies inside ONE batch (the
// per-batch quantities are non-linear); the host's tile table says where its rows are.  Five sums per tile, one record of doubles
// per (member, tile), no atomics.
// eval_reduce_multi_kernel: blockIdx.y = member; tiles -> batches -> passes -> out[g][4] in fp64, in a fixed order.
#include "vpc_abi_internal.h"
#include "vpc_device.h"
#include "vpc_small_device.h"
#include "vpc_rng.h"

namespace vpc {

enum { E_X = 0, E_H1, E_H2, E_ML, E_Z, E_G1, E_G2, E_COUNT };
constexpr int EVAL_TERMS = VPC_EVAL_TERMS;  // S_A, S_I, SQ, CNT, KL
constexpr int EVAL_LDS = (E_COUNT * SBUF + WAVES * EVAL_TERMS) * 4;
static_assert(2 * EVAL_LDS <= 163840, "two workgroups per CU");

struct EvalArgs {
    const float* x;              // member 0's [N][d] data
    const uint8_t* mask;         // member 0's [N][d] mask bytes
    const float* eps;            // member 0's [R][16] injected normals (draw == 0)
    const float* enc_img;
    const float* dec_img;
    const VpcMember* members;
    const long long* tiles;      // [n_tiles][4]: data row, valid rows, draw row, batch
    double* part;                // member 0's [n_tiles][EVAL_TERMS] records
    long sx, sm, seps, simg, spart;  // member strides in elements (sx / sm / seps 0: shared by all members)
    long N, R;                   // data rows, draw rows
    unsigned long long offset;   // Philox offset of the call (draw != 0)
    long tile0;                  // first tile of this launch
    float x_logvar;
    int d, d_real, L, draw;
};

template <int DT>
__global__ __launch_bounds__(THREADS) void eval_small_kernel(EvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    auto buf = [&](int b) { return lds + b * SBUF; };
    float* red = lds + E_COUNT * SBUF;
    constexpr int S1 = s_for_tiles(DT);
    const EncImg ei(DT);
    const DecImg di(DT);
    const unsigned mem = blockIdx.y;
    const long tile_id = a.tile0 + blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    double* rec = a.part + mem * a.spart + tile_id * EVAL_TERMS;
    // (uniform addresses: scalar loads)
    const long long* te = a.tiles + 4 * tile_id;
    const long xrow0 = te[0], nvl = te[1], erow0 = te[2];
    // a tile entry that points outside the arrays reads nothing: its record is zero (the host builds the table; this is the fence)
    if (xrow0 < 0 || nvl < 1 || nvl > 16 || xrow0 + nvl > a.N || erow0 < 0 || erow0 + nvl > a.R) {
        if (threadIdx.x < EVAL_TERMS) rec[threadIdx.x] = 0.0;
        return;
    }
    const int nv = (int)nvl;
    const float* xg = a.x + mem * a.sx;
    const uint8_t* mg = a.mask + mem * a.sm;
    const float* enc_img = a.enc_img + mem * a.simg;
    const float* dec_img = a.dec_img + mem * a.simg;
    // (re-derived from opaque base pointers per phase, as the tile body does: keeps the fragment loads of all layers from being
    // hoisted to the top of the kernel)
    const float *W1, *b1, *W2, *W3, *W4, *W5, *W6;
    auto weights = [&]() {
        const float* e_ = enc_img;
        const float* d_ = dec_img;
        asm volatile("" : "+s"(e_), "+s"(d_)::"memory");
        W1 = e_ + ei.oW1; b1 = e_ + ei.ob1; W2 = e_ + ei.oW2; W3 = e_ + ei.oW3;
        W4 = d_ + di.oW4; W5 = d_ + di.oW5; W6 = d_ + di.oW6;
    };
    const float inv_s2 = expf(-a.x_logvar), half_lv = 0.5f * a.x_logvar;
    const bool ok = c < nv;
    // ---- this wave's column tile of x and of the mask words (range-checked: rows past the tile's valid rows read 0; the last
    // tile's columns past d read column 0 and are cleared)
    const bool colok = 16 * w + 4 * q + 3 < a.d;
    f32x4 xv = zero4();
    uint32_t mw = 0;
    if (w < DT) {
        const int vo = c * a.d + (colok ? 16 * w + 4 * q : 0);
        xv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rows_rsrc(xg, xrow0, xrow0 + nv, a.d), 4 * vo, 0, 0));
        mw = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(mg) + xrow0 * a.d, 0, (uint32_t)(nv * a.d), 0x00020000), vo, 0, 0);
        if (!colok) { mw = 0; xv = zero4(); }
    }
    int cc = c, qq = q;
    launder(cc, qq);
    // ================================================================ encoder forward (phase E of the tile body, pass 0)
    {
        weights();
        f32x4 fW1[DT], fW2[H1T], fW3[H2T], bias1 = zero4();
        if (w < H1T) {
            ldW<DT, S1>(W1, w, cc, qq, fW1);
            bias1 = *reinterpret_cast<const f32x4*>(b1 + 16 * w + 4 * qq);
        }
        if (w < DT) st_act(buf(E_X), w, cc, qq, xv * mask_to_f32(mw));  // x.float() * mask  (VAE.py:388)
        if (w < H2T) ldW<H1T, 128>(W2, w, cc, qq, fW2);
        lds_barrier();
        launder(cc, qq);
        if (w < H1T) {
            f32x4 in[DT];
#pragma unroll
            for (int t = 0; t < DT; ++t) in[t] = ld_act(buf(E_X), t, cc, qq);
            st_act(buf(E_H1), w, cc, qq, relu4(mmW<DT>(fW1, in, bias1)));
        }
        if (w < 2) ldW<H2T, 64>(W3, w, cc, qq, fW3);
        lds_barrier();
        launder(cc, qq);
        if (w < H2T) {
            f32x4 in[H1T];
#pragma unroll
            for (int t = 0; t < H1T; ++t) in[t] = ld_act(buf(E_H1), t, cc, qq);
            st_act(buf(E_H2), w, cc, qq, relu4(mmW<H1T, NK1>(fW2, in, zero4())));
        }
        lds_barrier();
        launder(cc, qq);
        if (w < 2) {  // wave 0: mean tile, wave 1: logvar tile
            f32x4 in[H2T];
#pragma unroll
            for (int t = 0; t < H2T; ++t) in[t] = ld_act(buf(E_H2), t, cc, qq);
            f32x4 o = mmW<H2T, NK2>(fW3, in, zero4());
            if (!ok) o = zero4();  // rows past the valid ones: statistics 0
            st_act(buf(E_ML), w, cc, qq, o);
        }
    }
    lds_barrier();
    launder(cc, qq);
    // ================================================================ decoder forward and the five sums
    float S_A = 0.f, S_I = 0.f, SQ = 0.f, CNT = 0.f, KL = 0.f;
    {
        weights();
        f32x4 fW4[1], fW5[H2T], fW6[H1T];
        if (w < H2T) ldW<1, S4>(W4, w, cc, qq, fW4);
        if (w < H1T) ldW<H2T, 64>(W5, w, cc, qq, fW5);
        if (w == 0) {  // z = mean + eps * exp(logvar / 2); z[L] = 1 drives the bias chain; the row's KL to the standard normal
            const f32x4 mu = ld_act(buf(E_ML), 0, cc, qq), lv = ld_act(buf(E_ML), 1, cc, qq);
            f32x4 e;
            if (a.draw) {
                // group q of draw row r has the counter vpc_fill_normal gives float index 16 r + 4 q of a flat [R x 16] array
                e = eps_normal4((uint64_t)((erow0 + cc) * 4 + qq) + a.offset, a.members[mem].seed);
            } else {
                e = ld_rows(rows_rsrc(a.eps + mem * a.seps, erow0, erow0 + nv, 16), cc, 16, 4 * qq);
            }
            f32x4 z;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool lat = 4 * qq + j < a.L;
                z[j] = mu[j] + ((lat && ok) ? e[j] : 0.f) * __expf(0.5f * lv[j]);
                if (4 * qq + j == a.L) z[j] = 1.f;
                if (lat) KL += 0.5f * (__expf(lv[j]) + mu[j] * mu[j] - 1.f - lv[j]);  // (rows past the valid ones: 0)
            }
            st_act(buf(E_Z), 0, cc, qq, z);
        }
        lds_barrier();
        launder(cc, qq);
        if (w < H2T) {
            const f32x4 in[1] = {ld_act(buf(E_Z), 0, cc, qq)};
            st_act(buf(E_G1), w, cc, qq, relu4(mmW<1>(fW4, in, zero4())));
        }
        if (w < DT) ldW<H1T, 128>(W6, w, cc, qq, fW6);
        lds_barrier();
        launder(cc, qq);
        if (w < H1T) {
            f32x4 in[H2T];
#pragma unroll
            for (int t = 0; t < H2T; ++t) in[t] = ld_act(buf(E_G1), t, cc, qq);
            st_act(buf(E_G2), w, cc, qq, relu4(mmW<H2T, NK2>(fW5, in, zero4())));
        }
        lds_barrier();
        launder(cc, qq);
        if (w < DT) {  // output tile w: x_hat = sigmoid(.), the terms on mask and on its complement
            f32x4 in[H1T];
#pragma unroll
            for (int t = 0; t < H1T; ++t) in[t] = ld_act(buf(E_G2), t, cc, qq);
            const f32x4 pre = mmW<H1T, NK1>(fW6, in, zero4());
            const f32x4 mA = mask_to_f32(mw);
            const float hinv_s2 = 0.5f * inv_s2;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = fast_sigmoid(pre[j]);
                const float diff = xh - xv[j];
                const float t = diff * diff * hinv_s2 + half_lv;
                // the complement counts real rows and REAL columns only: a padding column has a zero mask byte too
                const float mI = (ok && 16 * w + 4 * qq + j < a.d_real) ? 1.f - mA[j] : 0.f;
                S_A += mA[j] * t;
                S_I += mI * t;
                SQ += mI * diff * diff;
                CNT += mI;
            }
        }
    }
    // ================================================================ the tile's record
    const float s[EVAL_TERMS] = {S_A, S_I, SQ, CNT, KL};
#pragma unroll
    for (int i = 0; i < EVAL_TERMS; ++i) {
        const float v = wave_sum_dpp(s[i]);
        if (lane == 0) red[w * EVAL_TERMS + i] = v;
    }
    lds_barrier();
    if (threadIdx.x < EVAL_TERMS) {
        double t = 0.0;
        for (int k = 0; k < WAVES; ++k) t += (double)red[k * EVAL_TERMS + threadIdx.x];
        rec[threadIdx.x] = t;
    }
}

// ---- tiles -> batches -> passes -> out[g][4]
constexpr int RED_WAVES = 8;
struct EvalReduceArgs {
    const double* part;          // member 0's [n_tiles][EVAL_TERMS]
    const long long* batches;    // [n_batches][4]: rows, pass, first tile, tiles
    const long long* passes;     // [M][2]: first batch, batches
    const VpcMember* members;
    float* out;                  // [G][4]: rmse, elbo, negll, negll_imp
    long spart, n_tiles, n_batches;
    int M, d_real;
};

__device__ __forceinline__ double wave_sum_f64(double v) {  // (fixed order: a butterfly)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(RED_WAVES * 64) void eval_reduce_multi_kernel(EvalReduceArgs a) {
    __shared__ double tot[RED_WAVES][4];
    const unsigned mem = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double* part = a.part + mem * a.spart;
    const double bw = (double)a.members[mem].co.bq;  // the member's KL weight
    constexpr double HL2PI = 0.91893853320467274;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};  // this wave's passes p = w, w + RED_WAVES, ...: sum of the pass means
    for (int p = w; p < a.M; p += RED_WAVES) {
        long b0 = a.passes[2 * p], nb = a.passes[2 * p + 1];
        if (b0 < 0 || nb < 0 || b0 + nb > a.n_batches) nb = 0;  // (fence, as in the forward kernel; an empty pass gives 0 / 0)
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (long b = b0 + lane; b < b0 + nb; b += 64) {
            const long long* be = a.batches + 4 * b;
            const double n_b = (double)be[0];
            long t0 = be[2], nt = be[3];
            if (t0 < 0 || nt < 0 || t0 + nt > a.n_tiles) nt = 0;
            double s[EVAL_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (long t = t0; t < t0 + nt; ++t)
#pragma unroll
                for (int i = 0; i < EVAL_TERMS; ++i) s[i] += part[t * EVAL_TERMS + i];
            const double c = n_b * (double)a.d_real * HL2PI;  // masked entries contribute the constant too
            const double negll = (s[0] + c) / n_b, negll_imp = (s[1] + c) / n_b;
            v[0] += sqrt(s[2] / s[3]);  // no unobserved entry: 0 / 0 = NaN, as evaluate.py:232-234
            v[1] += negll + bw * s[4] / n_b;
            v[2] += negll;
            v[3] += negll_imp;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += wave_sum_f64(v[i]) / (double)nb;  // mean over the batches of the pass
    }
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) tot[w][i] = acc[i];
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = 0.0;
        for (int k = 0; k < RED_WAVES; ++k) t += tot[k][threadIdx.x];
        a.out[mem * 4 + threadIdx.x] = (float)(t / (double)a.M);  // mean over the passes
    }
}

}  // namespace vpc

using namespace vpc;

extern "C" int vpc_eval_small_multi_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img,
                                        const float* dec_img, const VpcMember* members, int G, const long long* tiles,
                                        long n_tiles, long N, long R, int draw, unsigned long long offset, float x_logvar,
                                        double* part, const long* strides, int d, int d_real, int L, int max_blocks,
                                        void* stream) {
    if (!x || !mask || !enc_img || !dec_img || !members || !tiles || !part || !strides) return VPC_ERR_ARG;
    if (G < 1 || G > 65535 || n_tiles < 1 || N < 1 || R < 1 || max_blocks < 0) return VPC_ERR_ARG;
    if (!draw && !eps) return VPC_ERR_ARG;
    if (d < 4 || d > MAX_D || d % 4 || L < 1 || L > MAX_L) return VPC_ERR_SHAPE;
    if (d_real < 1 || d_real > d || dt_for(d_real) != dt_for(d)) return VPC_ERR_ARG;
    if (!aligned16(x) || !aligned16(enc_img) || !aligned16(dec_img) || !aligned16(eps)) return VPC_ERR_ARG;
    if ((uintptr_t)mask % 4 || (uintptr_t)tiles % 8 || (uintptr_t)part % 8) return VPC_ERR_ARG;
    const long sx = strides[VPC_MS_X], sm = strides[VPC_MS_MASK], seps = strides[VPC_MS_EPS], simg = strides[VPC_MS_IMG],
               sp = strides[VPC_MS_LOSS];
    // every member's slice inside its stride, 16-byte (masks: 4-byte) aligned; the read-only inputs may be shared (stride 0)
    if ((sx != 0 && sx < N * (long)d) || sx % 4 || (sm != 0 && sm < N * (long)d) || sm % 4) return VPC_ERR_ARG;
    if (!draw && ((seps != 0 && seps < R * 16) || seps % 4)) return VPC_ERR_ARG;
    if (simg <= 0 || simg % 4 || sp < n_tiles * EVAL_TERMS) return VPC_ERR_ARG;
    EvalArgs a{};
    a.x = x; a.mask = mask; a.eps = draw ? nullptr : eps; a.enc_img = enc_img; a.dec_img = dec_img; a.members = members;
    a.tiles = tiles; a.part = part;
    a.sx = sx; a.sm = sm; a.seps = draw ? 0 : seps; a.simg = simg; a.spart = sp;
    a.N = N; a.R = R; a.offset = offset; a.x_logvar = x_logvar; a.d = d; a.d_real = d_real; a.L = L; a.draw = draw ? 1 : 0;
    // the grid is (tiles of the chunk, G): consecutive workgroups are tiles of one member, so the workgroups in flight read one or
    // two members' images.  A launch holds at most max_blocks workgroups (0: VPC_EVAL_MAX_BLOCKS); the tile table is walked in chunks.
    const long cap = max_blocks ? max_blocks : VPC_EVAL_MAX_BLOCKS;
    const long per = cap / G > 0 ? cap / G : 1;
    hipStream_t s = (hipStream_t)stream;
    for (long t0 = 0; t0 < n_tiles; t0 += per) {
        const long nt = n_tiles - t0 < per ? n_tiles - t0 : per;
        a.tile0 = t0;
        const dim3 grid((unsigned)nt, (unsigned)G);
#define VPC_CASE(T)                                                                                        \
    case T: {                                                                                              \
        auto kern = eval_small_kernel<T>;                                                                  \
        if (!lds_attr_done(reinterpret_cast<const void*>(kern), EVAL_LDS)) return VPC_ERR_HIP;             \
        hipLaunchKernelGGL(kern, grid, dim3(THREADS), EVAL_LDS, s, a);                                     \
        break;                                                                                             \
    }
        switch (dt_for(d)) { VPC_CASE(1) VPC_CASE(2) VPC_CASE(4) VPC_CASE(8) default: return VPC_ERR_SHAPE; }
#undef VPC_CASE
        if (hipGetLastError() != hipSuccess) return VPC_ERR_HIP;
    }
    return VPC_OK;
}

extern "C" int vpc_eval_reduce_multi(const double* part, const long long* batches, long n_batches, const long long* passes,
                                     int M, const VpcMember* members, int G, long part_stride, long n_tiles, int d_real,
                                     float* out, void* stream) {
    if (!part || !batches || !passes || !members || !out) return VPC_ERR_ARG;
    if (G < 1 || G > 65535 || M < 1 || n_batches < 1 || n_tiles < 1 || d_real < 1 || d_real > MAX_D) return VPC_ERR_ARG;
    if (part_stride < n_tiles * EVAL_TERMS) return VPC_ERR_ARG;
    if ((uintptr_t)part % 8 || (uintptr_t)batches % 8 || (uintptr_t)passes % 8 || (uintptr_t)out % 4) return VPC_ERR_ARG;
    EvalReduceArgs a{part, batches, passes, members, out, part_stride, n_tiles, n_batches, M, d_real};
    hipLaunchKernelGGL(eval_reduce_multi_kernel, dim3(1, (unsigned)G), dim3(RED_WAVES * 64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}
