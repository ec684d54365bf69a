// Argument block and shared constants of the decoder kernels (vpc_dec.hip: 4 waves x 2 batch tiles, all three modes;
// vpc_dec8.hip: 8 waves x 1 batch tile, fused mode).
#pragma once
#include <cstdint>
#include "vpc_layout.h"
#include "vpc_abi_internal.h"

namespace vpc {

enum { MODE_FWD = 0, MODE_FUSED = 1, MODE_BWD = 2 };

struct DecArgs {
    const float* x;
    const float* img;
    const uint8_t* mA[2];
    const uint8_t* mB[2];
    float cA[2], cE[2];
    const float* mean[2];
    const float* logvar[2];
    const float* eps[2];
    const float* eps_ml;
    const float* z_in[2];
    const float* dxhat[2];
    float* xhat[2];
    float* dmean[2];
    float* dlogvar[2];
    float* dz[2];
    float* part;
    double* loss_part;
    float bq, bp, cr, wml, inv_B, x_logvar;
    long B;
    int d, L, npass, ntiles;
    int lp;   // row pitch of the [B][.] latent arrays: L (dense, API tensors) or 16 (padded workspaces)
    int psplit;  // 1: the passes are spread over blockIdx.y (small-batch shape), 0: every workgroup loops over them
    int dbg;  // ablation mask, only honoured by the diagnostic build (-DVPC_ABLATE); 0 in the product build
};

// In-kernel eps draw, the second argument of dec8_draw_kernel (a record of its own: DecArgs keeps its size, and with it the
// kernel-argument offsets in every other decoder kernel): the lane that forms z draws its eps group with vpc_draw_step's
// counter and stores it to eps_w[p] (the same array as DecArgs::eps[p]), where the pass end, dump and the draw-rule checks
// read it
struct DecDraw {
    float* eps_w[2];
    unsigned long long seed, off_eps;
    const long long* state;          // graph replay: state[1] is added to off_eps
    long eps_rows_global, eps_row_lo;  // row shard of the global [planes][rows_global][16] eps array (B rows from eps_row_lo)
};

constexpr int DEC_CH = 64;  // batch rows per wgrad staging chunk

// VPC_DBG(bit) guards the ablation switches of the diagnostic build (tools/ablate.sh).  In the product build it
// is an always-false test of a value the optimiser cannot see through: the switches cost one s_cbranch each
// and, more importantly, cut the kernel's 17k-line straight-line body into scheduling regions.  hipcc's
// scheduler otherwise hoists loads across the whole body, overshoots the 512-register budget and spills
// (measured on MI355X: 326 us without the region cuts, 252 us with them).
#ifdef VPC_ABLATE
#define VPC_DBG(bit) ((a.dbg & (bit)) != 0)
#else
__device__ __forceinline__ int opaque_zero() {
    int z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    return z;
}
#define VPC_DBG(bit) ((opaque_zero() & (bit)) != 0)
#endif
// scheduling-region cut with no other effect (a never-taken branch around an empty asm)
#define VPC_CUT()                                              \
    do {                                                       \
        if (VPC_DBG(0x4000)) asm volatile("s_nop 0");          \
    } while (0)

size_t dec8_lds(int DT, int prec);
int dec8_dispatch(const DecArgs& a, bool vec, int grid, int prec, hipStream_t s);
int dec8_draw_dispatch(const DecArgs& a, const DecDraw& dr, int grid, hipStream_t s);  // fp32, vector layout, the eps draw inside (vpc_dec8.hip)
// vpc_decoder_fused_draw_f32 up to its launch (vpc_dec.hip): the entry's checks, the drawing kernel's argument blocks and its
// workgroup shape, for vpc_step_f32 (vpc_step_f32.hip), which runs that kernel's body as a phase
int dec_fused_draw_prepare(const float* x, const float* dec_img, int npass, const uint8_t* const* maskA,
                           const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* mean,
                           const float* const* logvar, float* const* eps, float inv_B, float x_logvar, float* const* dmean,
                           float* const* dlogvar, float* partials, double* loss_partials, long B, int d, int L,
                           unsigned long long seed, unsigned long long offset_eps, const long long* state, long eps_rows_global,
                           long eps_row_lo, DecArgs& a, DecDraw& dd, TileShape& ts);

}  // namespace vpc
