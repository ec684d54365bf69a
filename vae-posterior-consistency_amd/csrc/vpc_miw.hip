// Elementwise / reduction kernels of the MIWAE path (reference src/models/VAE.py: MIWAE :3011-3134, Reg_MIWAE
// :3137-3301).  The layers are the generic fp32 GEMMs of vpc_gemm.hip; what is specific to the family runs here:
//
//   miw_sample     z[b,s,:] = mean[b] + softplus(raw[b]) * eps[b,s,:]                     (encoder :3059-3070 / :3188-3200)
//   miw_heads      (sigmoid | softplus + 0.001 | softplus + 3) of the [M][3d] decoder head GEMM     (decoder :3072-3076)
//   miw_loss       Student-t importance-weighted bound, forward and backward, in three launches:
//                    rows   per (pass, row, sample): masked Student-t sums, logpz - logq on the fresh draw, KL_reg
//                    slots  per (pass, slot): log-sum-exp with the reference's row/sample pairing, the softmax weights
//                           (scaled into gradient seeds), fixed-order loss partials, the llh_eval imputation
//                    grad   per element: decoder-head gradients; per (pass, row, l): encoder-head gradients; one
//                           workgroup reduces the loss partials in a fixed order into out8
//
//   miw_loss_multi the same three launches for G members of an ensemble (blockIdx.y = member; vpc_miw_loss_multi): the
//                  kernel bodies are the text fragments vpc_miw_rows_body.h / _slots_body.h / _grad_body.h of both forms
//
// The pairing couples rows across the whole batch, so the exchange between the per-row sums and the per-slot
// log-sum-exp goes through a scratch buffer between launches.  No float atomics; bit-reproducible.
#include "vpc_abi_internal.h"
#include "../../include/vpc.h"
#include "vpc_miw_device.h"

namespace vpc {

constexpr int MIW_WAVES = 4;  // waves per 256-thread workgroup of the row / slot kernels

struct MiwLossArgs {
    const float* x; const float* m; const float* mp;   // [B][d]; mp = nullptr for MIWAE
    const float* y[2]; long ldy; int raw;               // decoder heads of the q / p pass, rows b*S+s, [mean d | scale d | df d]
    const float* h[2];                                  // encoder heads [B][mean L | scale L] (activated)
    const float* e[2];                                  // fresh draws of loss(), [B][S][L]
    float* gy[2]; long ldg;                             // gradients w.r.t. the decoder heads (raw or activated as `raw`)
    float* gh[2];                                       // gradients w.r.t. the activated encoder heads [B][2L]
    float* xm_imp;                                      // [B][d] or nullptr
    float* lpo[2]; float* lw[2]; float* gpo[2]; float* gw[2];  // [B*S] each
    float* lpm; float* rl; float* kl;                   // [B*S], [B*S], [B]
    double* part;                                       // [nslot_blocks][8]
    double* out8; float* loss_f32; float* accum;
    int B, S, d, L, P, pairing, nslot_blocks;
    float alpha;
};

// The three kernel bodies are text fragments shared with the ensemble kernels below (vpc_miw_*_body.h).  Stand-alone: a member's
// array is the pointer itself.
#define MIW_AT(p, f) (p)
#define MIW_OUT(p, k) (p)
#define MIW_ALPHA a.alpha

// ---- launch 1: one wave per (pass, row b, sample s)
__global__ void __launch_bounds__(256) miw_rows_kernel(MiwLossArgs a) {
#include "vpc_miw_rows_body.h"
}

// the row of the likelihood term in slot (i, j): reference pairing = flat index i*B + j of the [S, B] reshape of the
// (row, sample)-ordered sums (VAE.py:3078-3081); per-row pairing = row j, sample i
__device__ __forceinline__ long miw_lpo_row(int pairing, int i, int j, int B, int S) {
    return pairing == VPC_MIW_PAIR_REFERENCE ? (long)i * B + j : (long)j * S + i;
}

// ---- launch 2: one wave per slot j, both passes; four waves per workgroup -> one row of partials per workgroup
__global__ void __launch_bounds__(256) miw_slots_kernel(MiwLossArgs a) {
#include "vpc_miw_slots_body.h"
}

// ---- launch 3: gradients + the fixed-order loss reduction
__global__ void __launch_bounds__(256) miw_grad_kernel(MiwLossArgs a, int nblk_elem, int nblk_head) {
#include "vpc_miw_grad_body.h"
}

#undef MIW_AT
#undef MIW_OUT
#undef MIW_ALPHA

// ---- the three launches for G members (vpc_miw_loss_multi): blockIdx.y = member; x / mask shared (stride 0) or per member,
// every other array the dense [G][..] stack of the stand-alone one, the scratch one stand-alone scratch per member
struct MiwLossMultiArgs {
    MiwLossArgs base;  // member 0
    const VpcMiwMember* members;
    long sx, sm;       // member strides of x and mask in floats
    long sscr;         // bytes of one member's scratch (a multiple of 64)
};
// where this workgroup's member sits behind the pointers of the base record, in elements of each array, and its alpha
struct MiwLossMem {
    long x, m, mp;   // data, mask, mask_p
    long y, h, e;    // decoder heads and their gradients; encoder heads and theirs; the draws
    long scr, part;  // the float arrays of the scratch; its double partials
    long out;        // out8 (x 8), loss_f32, accum
    float alpha;
};
__device__ __forceinline__ MiwLossMem miw_loss_member(const MiwLossMultiArgs& ma) {
    const MiwLossArgs& b = ma.base;
    const long g = blockIdx.y, N = (long)b.B * b.S, R = (long)b.P * b.B;
    MiwLossMem mo;
    mo.x = g * ma.sx; mo.m = g * ma.sm; mo.mp = g * b.B * b.d;
    mo.y = g * b.P * N * 3 * b.d;  // [P B S][3 d] per member
    mo.h = g * R * 2 * b.L;        // [P B][2 L]
    mo.e = g * 2 * b.P * N * b.L;  // [2 P][B][S][L]
    mo.scr = g * (ma.sscr / 4); mo.part = g * (ma.sscr / 8);
    mo.out = g;
    mo.alpha = ma.members[g].alpha;
    return mo;
}
#define MIW_AT(p, f) ((p) + mo.f)
#define MIW_OUT(p, k) ((p) + (k) * mo.out)
#define MIW_ALPHA mo.alpha
__global__ void __launch_bounds__(256) miw_rows_multi_kernel(MiwLossMultiArgs ma) {
    const MiwLossArgs& a = ma.base;
    const MiwLossMem mo = miw_loss_member(ma);
#include "vpc_miw_rows_body.h"
}
__global__ void __launch_bounds__(256) miw_slots_multi_kernel(MiwLossMultiArgs ma) {
    const MiwLossArgs& a = ma.base;
    const MiwLossMem mo = miw_loss_member(ma);
#include "vpc_miw_slots_body.h"
}
__global__ void __launch_bounds__(256) miw_grad_multi_kernel(MiwLossMultiArgs ma, int nblk_elem, int nblk_head) {
    const MiwLossArgs& a = ma.base;
    const MiwLossMem mo = miw_loss_member(ma);
#include "vpc_miw_grad_body.h"
}
#undef MIW_AT
#undef MIW_OUT
#undef MIW_ALPHA

__global__ void miw_sample_kernel(const float* __restrict__ heads, float* __restrict__ hact, const float* __restrict__ eps,
                                  float* __restrict__ z, long R, int S, int L) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * S * L) return;
    const long r = t / ((long)S * L);
    const long rem = t - r * S * L;
    const int s = (int)(rem / L), l = (int)(rem - (long)s * L);
    const float mu = heads[r * 2 * L + l];
    const float sc = miw_softplus(heads[r * 2 * L + L + l]);
    z[t] = eps ? mu + eps[t] * sc : mu;
    if (hact && s == 0) {
        hact[r * 2 * L + l] = mu;
        hact[r * 2 * L + L + l] = sc;
    }
}

__global__ void miw_sample_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ eps,
                                      const float* __restrict__ heads, const float* __restrict__ g_hact,
                                      float* __restrict__ out, long R, int S, int L) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * L) return;
    const long r = t / L;
    const int l = (int)(t - r * L);
    float gm = g_hact ? g_hact[r * 2 * L + l] : 0.f;
    float gs = g_hact ? g_hact[r * 2 * L + L + l] : 0.f;
    if (dz) {
        for (int s = 0; s < S; ++s) {
            const long i = (r * S + s) * L + l;
            gm += dz[i];
            if (eps) gs += dz[i] * eps[i];
        }
    }
    out[r * 2 * L + l] = gm;
    out[r * 2 * L + L + l] = gs * miw_softplus_d(heads[r * 2 * L + L + l]);
}

__global__ void miw_heads_kernel(const float* __restrict__ yr, const float* __restrict__ gact, float* __restrict__ out,
                                 long M, int d) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M * d) return;
    const long m = t / d;
    const int k = (int)(t - m * d);
    const float* y = yr + m * 3 * d;
    float* o = out + m * 3 * d;
    if (!gact) {
        const MiwHead h = miw_head(y, d, k, 1);
        o[k] = h.mu; o[d + k] = h.sc; o[2 * d + k] = h.v;
        return;
    }
    const float* g = gact + m * 3 * d;
    o[k] = g[k] * miw_sigmoid_d(y[k]);
    o[d + k] = g[d + k] * miw_softplus_d(y[d + k]);
    o[2 * d + k] = g[2 * d + k] * miw_softplus_d(y[2 * d + k]);
}

}  // namespace vpc

using namespace vpc;

static inline long miw_slot_blocks(long B) { return (B + MIW_WAVES - 1) / MIW_WAVES; }

extern "C" {

int vpc_miw_sample(const float* heads, float* hact, const float* eps, float* z, long R, int S, int L, void* stream) {
    if (!heads || !z || R <= 0 || S <= 0 || L <= 0) return VPC_ERR_ARG;
    const long n = R * S * L;
    hipLaunchKernelGGL(miw_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, heads,
                       hact, eps, z, R, S, L);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_sample_bwd(const float* dz, const float* eps, const float* heads, const float* g_hact, float* out, long R,
                       int S, int L, void* stream) {
    if (!heads || !out || R <= 0 || S <= 0 || L <= 0) return VPC_ERR_ARG;
    const long n = R * L;
    hipLaunchKernelGGL(miw_sample_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dz,
                       eps, heads, g_hact, out, R, S, L);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_heads(const float* y_raw, float* y_act, long M, int d, void* stream) {
    if (!y_raw || !y_act || M <= 0 || d <= 0) return VPC_ERR_ARG;
    const long n = M * d;
    hipLaunchKernelGGL(miw_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y_raw,
                       (const float*)nullptr, y_act, M, d);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_heads_bwd(const float* y_raw, const float* g_act, float* g_raw, long M, int d, void* stream) {
    if (!y_raw || !g_act || !g_raw || M <= 0 || d <= 0) return VPC_ERR_ARG;
    const long n = M * d;
    hipLaunchKernelGGL(miw_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y_raw,
                       g_act, g_raw, M, d);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

long vpc_miw_loss_scratch(long B, int S) {
    const long N = B * S;
    const long floats = 2 * 4 * N + 2 * N + B;  // lpo lw gpo gw per pass, lpm rl, kl
    return ((floats * 4 + 63) / 64) * 64 + miw_slot_blocks(B) * 8 * 8;
}

int vpc_miw_loss(const float* x, const float* mask, const float* mask_p, const float* y_q, const float* y_p, long ldy,
                 int raw, const float* heads_q, const float* heads_p, const float* eps_q, const float* eps_p,
                 float* g_y_q, float* g_y_p, long ldg, float* g_heads_q, float* g_heads_p, float* xm_imp,
                 void* scratch, long scratch_bytes, double* out8, float* loss_f32, float* accum, long B, int S, int d,
                 int L, double alpha, int pairing, void* stream) {
    const bool reg = mask_p != nullptr;
    if (!x || !mask || !y_q || !heads_q || !eps_q || !scratch || !out8 || B <= 0 || S <= 0 || d <= 0 || L <= 0 ||
        ldy < 3 * d || B * S > (1L << 30))
        return VPC_ERR_ARG;
    if (reg && (!y_p || !heads_p || !eps_p)) return VPC_ERR_ARG;
    if (pairing != VPC_MIW_PAIR_REFERENCE && pairing != VPC_MIW_PAIR_PER_ROW) return VPC_ERR_ARG;
    const bool grad = g_y_q != nullptr;
    if (grad && (!g_heads_q || ldg < 3 * d || (reg && (!g_y_p || !g_heads_p)))) return VPC_ERR_ARG;
    if (scratch_bytes < vpc_miw_loss_scratch(B, S) || ((uintptr_t)scratch & 7u)) return VPC_ERR_ARG;
    const long N = B * S;
    MiwLossArgs a{};
    a.x = x; a.m = mask; a.mp = mask_p;
    a.y[0] = y_q; a.y[1] = y_p; a.ldy = ldy; a.raw = raw;
    a.h[0] = heads_q; a.h[1] = heads_p;
    a.e[0] = eps_q; a.e[1] = eps_p;
    a.gy[0] = g_y_q; a.gy[1] = g_y_p; a.ldg = ldg;
    a.gh[0] = g_heads_q; a.gh[1] = g_heads_p;
    a.xm_imp = xm_imp;
    float* f = (float*)scratch;
    for (int p = 0; p < 2; ++p) {
        a.lpo[p] = f; f += N;
        a.lw[p] = f; f += N;
        a.gpo[p] = f; f += N;
        a.gw[p] = f; f += N;
    }
    a.lpm = f; f += N;
    a.rl = f; f += N;
    a.kl = f; f += B;
    const long fbytes = (((long)(f - (float*)scratch) * 4 + 63) / 64) * 64;
    a.part = (double*)((char*)scratch + fbytes);
    a.out8 = out8; a.loss_f32 = loss_f32; a.accum = accum;
    a.B = (int)B; a.S = S; a.d = d; a.L = L; a.P = reg ? 2 : 1; a.pairing = pairing;
    a.nslot_blocks = (int)miw_slot_blocks(B);
    a.alpha = (float)alpha;
    hipStream_t st = (hipStream_t)stream;
    const long rows = a.P * N;
    hipLaunchKernelGGL(miw_rows_kernel, dim3((unsigned)((rows + MIW_WAVES - 1) / MIW_WAVES)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(miw_slots_kernel, dim3((unsigned)a.nslot_blocks), dim3(256), 0, st, a);
    const long ne = grad ? (a.P * N * d + 255) / 256 : 0;
    const long nh = grad ? ((long)a.P * B * L + 255) / 256 : 0;
    if (ne + nh + 1 > 0x7fffffffL) return VPC_ERR_ARG;
    hipLaunchKernelGGL(miw_grad_kernel, dim3((unsigned)(ne + nh + 1)), dim3(256), 0, st, a, (int)ne, (int)nh);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_miw_loss_multi(const float* x, long x_stride, const float* mask, long mask_stride, const float* mask_p, const float* Y,
                       const float* hact, const float* eps, float* Gy, float* gh, void* scratch, long scratch_bytes,
                       double* out8, float* loss_f32, float* accum, const VpcMiwMember* members, int G, long B, int S, int d,
                       int L, int pairing, void* stream) {
    if (!x || !mask || !Y || !hact || !eps || !Gy || !gh || !scratch || !out8 || !members) return VPC_ERR_ARG;
    if (G < 1 || G > VPC_MIW_MULTI_MAX_MEMBERS || B <= 0 || S <= 0 || d <= 0 || d > 32 || L <= 0 || L > 16 ||
        B * S > (1L << 24))
        return VPC_ERR_ARG;
    if (pairing != VPC_MIW_PAIR_REFERENCE && pairing != VPC_MIW_PAIR_PER_ROW) return VPC_ERR_ARG;
    if ((x_stride != 0 && x_stride < B * d) || (mask_stride != 0 && mask_stride < B * d)) return VPC_ERR_ARG;
    const long sscr = vpc_miw_loss_scratch(B, S);
    if (scratch_bytes < G * sscr || ((uintptr_t)scratch & 7u)) return VPC_ERR_ARG;
    const int P = mask_p ? 2 : 1;
    const long N = B * S;
    MiwLossMultiArgs ma{};
    MiwLossArgs& a = ma.base;
    a.x = x; a.m = mask; a.mp = mask_p;
    a.y[0] = Y; a.y[1] = P == 2 ? Y + N * 3 * d : nullptr; a.ldy = 3 * d; a.raw = 1;
    a.h[0] = hact; a.h[1] = P == 2 ? hact + B * 2 * L : nullptr;
    a.e[0] = eps + P * N * L; a.e[1] = P == 2 ? eps + (P + 1) * N * L : nullptr;  // behind the P sampling planes
    a.gy[0] = Gy; a.gy[1] = P == 2 ? Gy + N * 3 * d : nullptr; a.ldg = 3 * d;
    a.gh[0] = gh; a.gh[1] = P == 2 ? gh + B * 2 * L : nullptr;
    float* f = (float*)scratch;
    for (int p = 0; p < 2; ++p) {
        a.lpo[p] = f; f += N;
        a.lw[p] = f; f += N;
        a.gpo[p] = f; f += N;
        a.gw[p] = f; f += N;
    }
    a.lpm = f; f += N;
    a.rl = f; f += N;
    a.kl = f; f += B;
    const long fbytes = (((long)(f - (float*)scratch) * 4 + 63) / 64) * 64;
    a.part = (double*)((char*)scratch + fbytes);
    a.out8 = out8; a.loss_f32 = loss_f32; a.accum = accum;
    a.B = (int)B; a.S = S; a.d = d; a.L = L; a.P = P; a.pairing = pairing;
    a.nslot_blocks = (int)miw_slot_blocks(B);
    ma.members = members; ma.sx = x_stride; ma.sm = mask_stride; ma.sscr = sscr;
    hipStream_t st = (hipStream_t)stream;
    const long rows = P * N, ne = (P * N * d + 255) / 256, nh = ((long)P * B * L + 255) / 256;
    const unsigned g = (unsigned)G;
    hipLaunchKernelGGL(miw_rows_multi_kernel, dim3((unsigned)((rows + MIW_WAVES - 1) / MIW_WAVES), g), dim3(256), 0, st, ma);
    hipLaunchKernelGGL(miw_slots_multi_kernel, dim3((unsigned)a.nslot_blocks, g), dim3(256), 0, st, ma);
    hipLaunchKernelGGL(miw_grad_multi_kernel, dim3((unsigned)(ne + nh + 1), g), dim3(256), 0, st, ma, (int)ne, (int)nh);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
