// The row-tiled fp32 step's three MFMA kernels as three PHASES of one launch (gfx950):
//   E  encoder forward sweep, mask_p drawn      vpc_enc_sweep_body.h   = enc_fwd_sweep_kernel<8, true>
//   D  fused decoder, eps drawn                 vpc_dec8_body.h        = dec8_draw_kernel<8>
//   B  encoder backward                         vpc_enc_bwd_body.h     = enc_bwd_kernel<8, true, false, 8, PREC_F32>, psplit 0
// Each phase is the text of its kernel: its own tile loop, its own weight image, its own partial-block and loss-partial
// writes.  What goes away is two kernel boundaries, with the write-back of the dirty lines the predecessor leaves behind.
//
// Why workgroup barriers are all the synchronisation there is: in the throughput shape the three kernels run the same
// persistent grid - workgroup b takes tiles b, b + gridDim.x, ... in every phase - and everything one phase reads of another
// was written by the SAME workgroup: mean / logvar, h1 / h2, dmean / dlogvar by the very lane that reads them back (local
// row 16 w + c, columns 4 q ...), mask_p by the waves of the workgroup for the 128 rows of its own tiles.  Only the gradient
// partial blocks cross workgroups, and they are read by the next launch (vpc_reduce_step*).  So no workgroup ever waits for, or
// assumes anything about, another one.
//
// The join between two phases: every wave waits for its own global stores (vmcnt(0)) and meets the others at a workgroup
// barrier (__syncthreads: all of a workgroup's waves share one CU and one L1, so what was stored before the barrier is what a
// load after it returns); behind the barrier no wave reads the previous phase's LDS image any more, and the next phase's
// load_image may write over it.  The barriers sit outside the tile loops: a workgroup without a tile still reaches them.
#include "vpc_device.h"
#include "vpc_bf16.h"
#include "vpc_abi_internal.h"
#include "vpc_enc_args.h"
#include "vpc_dec_args.h"
#include "vpc_rng.h"
#include <cstdlib>

namespace vpc {

constexpr int DEC8_WAVES = 8, DEC8_THREADS = 512;  // as vpc_dec8.hip (names the decoder fragment expects)

#ifdef VPC_ABLATE
#define ABL(bit) VPC_DBG(bit)   // as vpc_dec8.hip
#else
#define ABL(bit) false
#endif

struct StepF32Args {  // (host side: the five argument blocks of one launch)
    EncFwdArgs e;
    EncDraw ed;
    DecArgs d;
    DecDraw dd;
    EncBwdArgs b;
};

__device__ __forceinline__ void phase_join() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    asm volatile("" ::: "memory");
}

// Each phase sees its argument blocks as objects of its own named `a` / `dr`, copied from the kernel's parameters - what a
// by-value kernel parameter is to the stand-alone kernel.  (Bound as references to the parameters, the fragments' lambdas capture
// a reference to a reference, hipcc's SLP vectoriser then pairs the KL seeds at the decoder's pass end differently, and dmean /
// dlogvar come out a few ulp away from dec8_draw_kernel's: the phases must give the kernels' bytes.)
template <int DT>
__global__ __launch_bounds__(512, 2) void step_f32_kernel(EncFwdArgs ea, EncDraw edr, DecArgs da, DecDraw ddr, EncBwdArgs ba) {
    {  // ---- phase E
        constexpr bool DRAW = true;
        EncFwdArgs a = ea;
        EncDraw dr = edr;
#include "vpc_enc_sweep_body.h"
    }
    phase_join();
    {  // ---- phase D
        constexpr bool VEC = true, DRAW = true;
        constexpr int PREC = PREC_F32;
        DecArgs a = da;
        DecDraw dr = ddr;
#include "vpc_dec8_body.h"
    }
    phase_join();
    {  // ---- phase B
        constexpr bool VEC = true, AUG = false;
        constexpr int NW = 8, PREC = PREC_F32;
        EncBwdArgs a = ba;
#include "vpc_enc_bwd_body.h"
    }
}

}  // namespace vpc

using namespace vpc;

// see include/vpc.h
extern "C" int vpc_step_f32(const float* x, const float* enc_img, const float* dec_img, const uint8_t* mask_in,
                            uint8_t* mask_p_out, const uint8_t* const* maskB, const VpcLossCoef* co, float* const* h1,
                            float* const* h2, float* const* mean, float* const* logvar, float* const* eps, float* const* dmean,
                            float* const* dlogvar, float inv_B, float x_logvar, float* partE, float* partD, double* loss_partials,
                            int* nblocksE_out, int* nblocksD_out, long B, int d, int L, float keep_prob, unsigned long long seed,
                            unsigned long long offset_mask, unsigned long long offset_eps, const long long* state,
                            long mask_elem_lo, long eps_rows_global, long eps_row_lo, int force_shape, void* stream) {
    StepF32Args P{};
    TileShape tsE, tsD, tsB;
    if (int e = enc_fwd_draw_prepare(x, enc_img, mask_in, mask_p_out, h1, h2, mean, logvar, B, d, L, keep_prob, seed, offset_mask,
                                     state, mask_elem_lo, P.e, P.ed, tsE))
        return e;
    const uint8_t* const masks[2] = {mask_in, mask_p_out};
    if (int e = dec_fused_draw_prepare(x, dec_img, 2, masks, maskB, co, mean, logvar, eps, inv_B, x_logvar, dmean, dlogvar, partD,
                                       loss_partials, B, d, L, seed, offset_eps, state, eps_rows_global, eps_row_lo, P.d, P.dd, tsD))
        return e;
    bool vecB = false;
    if (int e = enc_bwd_prepare(x, enc_img, 2, masks, h1, h2, dmean, dlogvar, 16, 0, PREC_F32, partE, B, d, L, force_shape != 0,
                                P.b, vecB, tsB))
        return e;
    if (!vecB) return VPC_ERR_SHAPE;
    // one persistent grid for the three phases: the shape each kernel would run on its own has to be the same one
    const TileShape* ts[3] = {&tsE, &tsD, &tsB};
    for (const TileShape* t : ts)
        if (t->small || t->grid_y != 1 || t->grid_x != tsE.grid_x || t->ntiles != tsE.ntiles) return VPC_ERR_PHASES;
    if (P.e.psplit || P.d.psplit || P.b.psplit) return VPC_ERR_PHASES;
    size_t lds = dec8_lds(8, PREC_F32);
    if (enc_fwd_lds(8) > lds) lds = enc_fwd_lds(8);
    if (enc_bwd_lds(8, 8) > lds) lds = enc_bwd_lds(8, 8);
    auto kern = step_f32_kernel<8>;
    if (!lds_attr_done(reinterpret_cast<const void*>(kern), lds)) return VPC_ERR_HIP;
    if (nblocksE_out) *nblocksE_out = tsB.nblocks;
    if (nblocksD_out) *nblocksD_out = tsD.nblocks;
    enc_fwd_set_form(VPC_ENC_FWD_SWEEP_DRAW);
    hipLaunchKernelGGL(kern, dim3(tsE.grid_x), dim3(512), lds, (hipStream_t)stream, P.e, P.ed, P.d, P.dd, P.b);
    return hipGetLastError() == hipSuccess ? VPC_OK : VPC_ERR_HIP;
}
