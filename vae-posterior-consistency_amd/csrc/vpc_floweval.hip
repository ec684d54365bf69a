// Batched evaluation of a flow model (include/vpc.h, vpc_flow_fwd_tiles / vpc_flow_eval_tiles / vpc_flow_eval_finalize;
// reference src/experiment_main/evaluate.py:160-245 around VAE.py:1816-1831, :1950-1969, :2099-2104).  The rows of every batch
// of every Monte-Carlo pass stand behind each other and go through the layers once (vpc_gemm.hip); what is not
// row-independent runs here, with a table of batches ("tiles", tab[t] .. tab[t + 1] - 1 = the rows of tile t):
//
//   flow_fwd_tiles        Flow.forward, torch.any(inside) (:1698) taken per tile
//   flow_eval_rows        the evaluate-stage loss terms and the RMSE sums: blockIdx.y = tile, one wave per row, the launch 1 of
//                         vpc_flow_loss on the tile's rows, then the two RMSE columns in the same shape
//   flow_eval_reduce      blockIdx.x = tile: the launch 2 of vpc_flow_loss on the tile's partials, then the two RMSE columns
//   flow_eval_finalize    per-tile ratios, the mean over each pass's tiles, the mean over the passes: one workgroup
//
// The per-element and per-row code is the text of the flow path's kernels (vpc_flow_fwd_elem_body.h, vpc_flow_loss_rows_body.h,
// vpc_flow_loss_reduce_body.h): a tile's rows come out bit for bit as vpc_flow_fwd / vpc_flow_loss give them for that tile alone.
// The kernels read the DEVICE copy of a table and clamp what they read to [0, R]: whatever it holds, no access leaves the arrays.
// No float atomics anywhere; every reduction has a fixed order (the rule at the top of vpc_flow.hip).
#include "vpc_abi_internal.h"
#include "vpc_flow_loss_args.h"

namespace vpc {

__device__ __forceinline__ long flow_clamp(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One thread per (row, latent) of the R stacked rows.  A workgroup's 256 elements lie in rows row0 .. row1, which may belong to
// several tiles (a tile may be one row): it finds row0's tile by bisection and takes the predicate of every tile up to row1's,
// each over that tile's draws alone (flow_pass_inside: one 256-element chunk for any non-degenerate draw).  Every thread of
// the workgroup walks the same tiles, so the barriers inside are uniform.
__global__ void __launch_bounds__(256) flow_fwd_tiles_kernel(const float* __restrict__ t, long ldt,
                                                             const float* __restrict__ eps, float* __restrict__ z,
                                                             float* __restrict__ zlp, long R,
                                                             const long* __restrict__ tab, int n_tiles) {
    __shared__ int sh[4];
    const long n = R * FLOW_L;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long r = g / FLOW_L;
    const int i = (int)(g - r * FLOW_L);
    const long row0 = (long)blockIdx.x * blockDim.x / FLOW_L;
    const long end = ((long)blockIdx.x + 1) * blockDim.x;
    const long row1 = ((end < n ? end : n) - 1) / FLOW_L;  // the last row this workgroup holds an element of
    int tlo = 0, thi = n_tiles - 1;  // the last tile whose first row is <= row0
    while (tlo < thi) {
        const int mid = (tlo + thi + 1) >> 1;
        if (tab[mid] <= row0) tlo = mid; else thi = mid - 1;
    }
    bool any_inside = false;
    for (int ti = tlo; ti < n_tiles; ++ti) {
        const long ra = flow_clamp(tab[ti], 0, R), rb = flow_clamp(tab[ti + 1], ra, R);
        if (ra > row1) break;
        const bool f = flow_pass_inside(eps + ra * FLOW_L, rb - ra, sh);
        if (r >= ra && r < rb) any_inside = f;
    }
    if (g >= n) return;
#include "vpc_flow_fwd_elem_body.h"
}

struct FlowEvalArgs {
    FlowLossArgs base;   // the stacked arrays (row 0), tile 0's partials, d, beta, var, logs; P = 1: the evaluate-stage loss reads no p pass
    const long* tab;     // device copy of tile_row0 [n_tiles + 1]
    long R;
    int pitch;           // partial blocks reserved per tile = ceil(max tile rows / 4)
    double* part2;       // [n_tiles][pitch][2]: the partials of columns 4 and 5
    double* out8;        // [n_tiles][8]: the tile's out8 as vpc_flow_loss lays it out
    double* stats;       // [n_tiles][8]
};

// the record of vpc_flow_loss on tile `tile` alone: its rows of the stacked arrays, its partial blocks, its out8
__device__ __forceinline__ FlowLossArgs flow_eval_tile(const FlowEvalArgs& e, const long tile) {
    FlowLossArgs a = e.base;
    const long ra = flow_clamp(e.tab[tile], 0, e.R), rb = flow_clamp(e.tab[tile + 1], ra, e.R);
    a.x += ra * a.d; a.m += ra * a.d;
    a.xm[0] += ra * a.ldxm;
    a.z[0] += ra * FLOW_L; a.zlp[0] += ra * FLOW_L;
    a.B = (int)(rb - ra);
    const int nblk = (a.B + FLOW_WAVES - 1) / FLOW_WAVES;
    a.nblk = nblk < e.pitch ? nblk : e.pitch;  // (a device table with a longer tile than the host's: stay inside the partials)
    a.part += tile * e.pitch * 8;
    a.out8 = e.out8 + tile * 8;
    return a;
}

__global__ void __launch_bounds__(256) flow_eval_rows_kernel(FlowEvalArgs e) {
    const FlowLossArgs a = flow_eval_tile(e, blockIdx.y);
    if ((int)blockIdx.x >= a.nblk) return;  // this tile has fewer rows than the longest one (uniform: before any barrier)
#include "vpc_flow_loss_rows_body.h"
    // columns 4 and 5 in the same shape: fp32 within the wave's row, doubles above (evaluate.py:232-235, x_mean * ~mask - x * ~mask)
    __shared__ float sh_e[FLOW_WAVES][2];
    float se = 0.f, sc = 0.f;
    if (b < B) {
        const float* xr = a.x + (long)b * d;
        const float* mr = a.m + (long)b * d;
        const float* yr = a.xm[0] + (long)b * a.ldxm;
        for (int k = lane; k < d; k += 64) {
            const float w = 1.f - mr[k];
            const float dv = yr[k] * w - xr[k] * w;
            se += dv * dv;
            sc += w;
        }
        se = flow_wave_sum(se);
        sc = flow_wave_sum(sc);
    }
    if (lane == 0) {
        sh_e[wv][0] = se;
        sh_e[wv][1] = sc;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s2 = 0.0;
        for (int w = 0; w < FLOW_WAVES; ++w) s2 += (double)sh_e[w][threadIdx.x];
        e.part2[((long)blockIdx.y * e.pitch + blockIdx.x) * 2 + threadIdx.x] = s2;
    }
}

__global__ void __launch_bounds__(256) flow_eval_reduce_kernel(FlowEvalArgs e) {
    const FlowLossArgs a = flow_eval_tile(e, blockIdx.x);
#include "vpc_flow_loss_reduce_body.h"
    // columns 4 and 5: 32 lanes in a strided fixed order, then in lane order, as the body sums its columns
    __shared__ double sh_e[2][33];
    if (threadIdx.x < 64) {
        const int c2 = threadIdx.x >> 5, l2 = threadIdx.x & 31;
        const double* p2 = e.part2 + (long)blockIdx.x * e.pitch * 2;
        double s2 = 0.0;
        for (int k = l2; k < a.nblk; k += 32) s2 += p2[(long)k * 2 + c2];
        sh_e[c2][l2] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // (the thread that wrote the tile's out8 above)
        double u4 = 0.0, u5 = 0.0;
        for (int j = 0; j < 32; ++j) {
            u4 += sh_e[0][j];
            u5 += sh_e[1][j];
        }
        const double* o8 = a.out8;
        double* st = e.stats + (long)blockIdx.x * 8;
        st[0] = o8[0];  // loss_q = RE_q + beta KL_q
        st[1] = o8[1];  // RE_q
        st[2] = o8[3];  // KL_q
        st[3] = o8[7];  // RE_q_imputed
        st[4] = u4;
        st[5] = u5;
        st[6] = (double)a.B;
        st[7] = 0.0;
    }
}

// thread j: the passes j, j + 256, ..; a pass's tiles in table order.  Then the threads in order (M <= 256: the passes in order).
__global__ void __launch_bounds__(256) flow_eval_finalize_kernel(const double* __restrict__ stats, long n_tiles,
                                                                 const long* __restrict__ ptab, long M,
                                                                 double* __restrict__ out4) {
    __shared__ double sh[256][4];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long p = threadIdx.x; p < M; p += blockDim.x) {
        const long ta = flow_clamp(ptab[p], 0, n_tiles), tb = flow_clamp(ptab[p + 1], ta, n_tiles);
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (long ti = ta; ti < tb; ++ti) {
            const double* st = stats + ti * 8;
            const double rows = st[6];
            s[0] += sqrt(st[4] / st[5]);
            s[1] += st[0] / rows;
            s[2] += st[1] / rows;
            s[3] += st[3] / rows;
        }
        const double nt = (double)(tb - ta);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += s[k] / nt;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[threadIdx.x][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        double u = 0.0;
        for (int j = 0; j < 256; ++j) u += sh[j][threadIdx.x];
        out4[threadIdx.x] = u / (double)M;
    }
}

}  // namespace vpc

using namespace vpc;

// a host table [n + 1]: 0 first, strictly ascending, `last` last; max_step: its longest interval
static bool flow_table_ok(const long* tab, long n, long last, long* max_step) {
    if (!tab || n < 1 || tab[0] != 0 || tab[n] != last) return false;
    long mx = 0;
    for (long i = 0; i < n; ++i) {
        const long step = tab[i + 1] - tab[i];
        if (step <= 0) return false;
        if (step > mx) mx = step;
    }
    if (max_step) *max_step = mx;
    return true;
}

static inline long flow_eval_part_doubles(long pitch, long n_tiles) { return n_tiles * pitch * 8; }

extern "C" {

int vpc_flow_fwd_tiles(const float* t, long ldt, const float* eps, float* z, float* z_log_prob, long R, const long* tile_row0,
                       const long* tile_row0_dev, long n_tiles, void* stream) {
    if (!t || !eps || !z || !z_log_prob || !tile_row0_dev || ldt < FLOW_CTX || R <= 0 || R > (1L << 26) || n_tiles > R ||
        !flow_table_ok(tile_row0, n_tiles, R, nullptr))
        return VPC_ERR_ARG;
    const long n = R * FLOW_L;
    hipLaunchKernelGGL(flow_fwd_tiles_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, ldt,
                       eps, z, z_log_prob, R, tile_row0_dev, (int)n_tiles);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

long vpc_flow_eval_tiles_scratch(long max_tile_rows, long n_tiles) {
    if (max_tile_rows <= 0 || n_tiles <= 0) return 0;
    const long pitch = flow_loss_blocks(max_tile_rows);
    return (flow_eval_part_doubles(pitch, n_tiles) + n_tiles * pitch * 2 + n_tiles * 8) * 8;
}

int vpc_flow_eval_tiles(const float* x, const float* mask, const float* x_mean, long ldxm, const float* z,
                        const float* z_log_prob, long R, int d, const long* tile_row0, const long* tile_row0_dev, long n_tiles,
                        float beta, void* scratch, long scratch_bytes, double* stats, void* stream) {
    long max_rows = 0;
    if (!x || !mask || !x_mean || !z || !z_log_prob || !tile_row0_dev || !scratch || !stats || d <= 0 || ldxm < d || R <= 0 ||
        R > (1L << 26) || n_tiles > 65535 || !flow_table_ok(tile_row0, n_tiles, R, &max_rows))
        return VPC_ERR_ARG;
    if (((uintptr_t)scratch & 7u) || scratch_bytes < vpc_flow_eval_tiles_scratch(max_rows, n_tiles)) return VPC_ERR_ARG;
    FlowEvalArgs e{};
    FlowLossArgs& a = e.base;
    a.x = x; a.m = mask;
    a.xm[0] = x_mean; a.ldxm = ldxm;
    a.z[0] = z; a.zlp[0] = z_log_prob;
    a.d = d; a.P = 1; a.eval = 1;
    a.beta = beta;
    flow_loss_obs(a);
    e.tab = tile_row0_dev;
    e.R = R;
    e.pitch = (int)flow_loss_blocks(max_rows);
    a.part = (double*)scratch;
    e.part2 = a.part + flow_eval_part_doubles(e.pitch, n_tiles);
    e.out8 = e.part2 + n_tiles * e.pitch * 2;
    e.stats = stats;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(flow_eval_rows_kernel, dim3((unsigned)e.pitch, (unsigned)n_tiles), dim3(256), 0, st, e);
    hipLaunchKernelGGL(flow_eval_reduce_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, e);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

int vpc_flow_eval_finalize(const double* stats, long n_tiles, const long* pass_tile0, const long* pass_tile0_dev, long M,
                           double* out4, void* stream) {
    if (!stats || !pass_tile0_dev || !out4 || n_tiles < 1 || !flow_table_ok(pass_tile0, M, n_tiles, nullptr)) return VPC_ERR_ARG;
    hipLaunchKernelGGL(flow_eval_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, stats, n_tiles, pass_tile0_dev, M,
                       out4);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}

}  // extern "C"
