/* vpc.h - C ABI of libvpc_hip.so: the MI355X (gfx950) kernels behind the VAE posterior-consistency
 * training step.
 *
 * The reference (stschia/VAE-posterior-consistency) is pure Python and has no FFI / plugin registry; its
 * boundary for this path is the model-class API in src/models/VAE.py.  The Python
 * host package `vae-posterior-consistency_amd` mirrors that API and calls ONLY the entry points below
 * (ctypes).  Each entry point names the reference lines whose arithmetic it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the comment says "host"; the caller owns all buffers, the
 *    library allocates no device memory and keeps no state between calls except two per-device caches of constants
 *    (CU count, "dynamic-LDS attribute already raised for this kernel"), both mutex / atomic protected;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); every launch goes on it;
 *  - return value: 0 ok, 1 bad argument, 2 unsupported shape (d > 128 or L > 15), 3 HIP runtime error.
 *    No exceptions cross the ABI;
 *  - fp32 tensors are row-major and exactly the reference's shapes: x, xhat [B][d]; mean, logvar, eps, z
 *    [B][L]; masks are one byte per element holding 0 or 1 (the kernels convert them with v_cvt_f32_ubyte), [B][d];
 *  - `npass` = 1 (vanilla_VAE) or 2 (Reg_VAE: pass 0 = q, encoded with `mask`; pass 1 = p, encoded with
 *    `mask_p`); per-pass pointers are passed as HOST arrays of `npass` device pointers;
 *  - h1 [B][112] and h2 [B][64] are padded fp32 workspaces (16-byte aligned) that carry the hidden
 *    activations from vpc_encoder_fwd to vpc_encoder_bwd;
 *  - weights are consumed as packed "images" (see csrc/vpc_layout.h) produced by vpc_pack_weights from the
 *    flat fp32 parameter vector in state_dict order
 *        seq_encoder.{0,2,4}.{weight,bias}, seq_decoder.{0,2,4}.{weight,bias}   (VAE.py:366-376);
 *  - weight gradients leave the kernels as per-workgroup partial blocks; vpc_reduce_partials turns them
 *    into the flat gradient in the same order (deterministic summation order).
 */
#ifndef VPC_H
#define VPC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host-side layout queries (no GPU needed) --------------------------------------------------- */

/* Sizes (in elements) for model (d, L).  Any out pointer may be NULL.  mask_augm != 0 selects the
 * mask-augmented encoder of Reg_VAE_mask / vanilla_VAE_mask (src/models/VAE.py:510-667, 995-1116): the encoder
 * input is [x*mask | mask] of width 2d (needs 2d <= 128), seq_encoder.0.weight is [100][2d]. */
int vpc_layout_sizes(int d, int L, int mask_augm, int* enc_img_floats, int* dec_img_floats, int* n_enc_params,
                     int* n_params, int* enc_part_floats, int* dec_part_floats, int* loss_terms, int* tile_rows);

/* HOST arrays: pack_idx[n_params] (offset of flat parameter i in the combined image [enc | dec]),
 * grad_idx[n_params] (offset of its gradient inside an encoder (i < n_enc) / decoder partial block),
 * img_template[enc_img_floats + dec_img_floats] (zeros plus the constant ones of the bias chain). */
int vpc_build_indices(int d, int L, int mask_augm, int* pack_idx, int* grad_idx, float* img_template);

/* The same pair for the point-net classes Reg_EDDI / vanilla_EDDI (src/models/VAE.py:694-700): the tiled part of the model is
 * the trunk pnp_encoder2 K -> 100 -> 50 -> 2L as the encoder (input width K <= 32) and seq_decoder L -> 50 -> 100 -> d.
 * n_params counts those twelve tensors in state_dict order (pack_idx / grad_idx cover them), n_front_params the four front-end
 * tensors that follow them in the flat parameter vector of vpc_reduce_step_adam_eddi: type_pars1 [d][K], type_bias1 [d],
 * pnp_encoder1.0.weight [K][2+K], pnp_encoder1.0.bias [K]. */
int vpc_layout_sizes_pointnet(int d, int K, int L, int* enc_img_floats, int* dec_img_floats, int* n_enc_params, int* n_params,
                              int* n_front_params, int* enc_part_floats, int* dec_part_floats, int* loss_terms, int* tile_rows);
int vpc_build_indices_pointnet(int d, int K, int L, int* pack_idx, int* grad_idx, float* img_template);

/* Compute units of the current device. */
int vpc_num_cus(void);
/* Upper bound of *nblocks_out of any kernel below (= 2 * CUs: the small-batch shape spreads the two passes over
 * separate workgroups): size `partials` / `loss_partials` buffers for this many blocks. */
int vpc_max_partial_blocks(void);

/* ---- precision of the matrix products (argument `precision` of vpc_encoder_fwd / vpc_encoder_bwd /
 * vpc_decoder_fused) ------------------------------------------------------------------------------------------
 *   0  f32     v_mfma_f32_16x16x4_f32 on the fp32 images (exact fp32 FMA chains; the path every parity claim of the
 *              1e-4 target refers to)
 *   1  bf16x3  "split bf16": operands carried as bf16 hi + bf16 lo, hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16
 *              with fp32 accumulation - fp32-class accuracy at 16/3 of the fp32 MFMA rate
 *   2  bf16    plain bf16 inputs, fp32 accumulation (BASELINE configs 2 / 3 name bf16); loss math stays fp32
 * 1 and 2 take the images of vpc_build_indices_bf16 / vpc_pack_weights_bf16 instead of the fp32 images, exist for
 * d % 4 == 0 in the plain (not mask-augmented) encoder, and in vpc_decoder_fused for d in (64, 128]. */
int vpc_layout_sizes_bf16(int d, int L, int mask_augm, int* enc_img_floats, int* dec_img_floats);
/* HOST arrays: pack_idx_bf[n_params], img_template_bf[enc + dec floats of vpc_layout_sizes_bf16] */
int vpc_build_indices_bf16(int d, int L, int mask_augm, int* pack_idx_bf, float* img_template_bf);
/* img_bf <- flat parameters as bf16 hi / lo pairs (the layer-1 bias stays fp32) */
int vpc_pack_weights_bf16(const float* flat_params, const int* pack_idx_bf, float* img_bf, int n, void* stream);

/* ---- parameters --------------------------------------------------------------------------------- */

/* img[pack_idx[i]] = flat_params[i].  Replaces nothing in the reference (nn.Linear keeps [out][in]). */
int vpc_pack_weights(const float* flat_params, const int* pack_idx, float* img, int n, void* stream);

/* grad_out[i] = scale * sum_b partials[b * block_stride + grad_idx[i]], i < n. */
int vpc_reduce_partials(const float* partials, int nblocks, long block_stride, const int* grad_idx,
                        float* grad_out, int n, float scale, void* stream);

/* torch.optim.Adam(lr, betas, eps), no weight decay / amsgrad - src/experiment_main/train.py:21,116.
 * `step` is the 1-based step count; if step_dev != NULL the count is read from device memory instead (word 0
 * of the `state` vpc_reduce_step maintains) so that a captured HIP graph can be replayed.  If pack_idx/img are
 * non-NULL the updated value is also written into the packed image (saves the vpc_pack_weights launch).
 * accum != NULL: accum[0] += loss_in[0] in the same launch (data parallel: the epoch total of the all-reduced step
 * loss, train.py:117, without a separate tiny kernel). */
int vpc_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n, float lr,
                  float beta1, float beta2, float eps, long step, const long long* step_dev, const int* pack_idx,
                  float* img, const float* loss_in, float* accum, void* stream);

/* ---- encoder: Reg_VAE.encoder / vanilla_VAE.encoder, src/models/VAE.py:387-395, 1155-1163 -------- */

/* For each pass p: h = MLP(x * mask[p]); mean[p], logvar[p] = chunk(h); if z[p]: z = mean + eps[p] *
 * exp(logvar / 2) (eps[p] NULL -> z = mean, the sample=False branch).  eps / z arrays may be NULL.
 * lat_pitch = row pitch in floats of mean / logvar: L (the reference's dense [B][L] tensors) or 16 (padded
 * 16-byte aligned workspaces of the fused path, pad entries written as 0; z must then be NULL). */
int vpc_encoder_fwd(const float* x, const float* enc_img, int npass, const uint8_t* const* mask,
                    const float* const* eps, float* const* h1, float* const* h2, float* const* mean,
                    float* const* logvar, float* const* z, int lat_pitch, int mask_augm, int precision, long B, int d,
                    int L, void* stream);

/* Autograd of the above (src/experiment_main/train.py:115): given d loss / d mean and d loss / d logvar
 * (with the reparameterisation path already folded in) accumulate the encoder weight gradients of all
 * passes into partial blocks [*nblocks_out][enc_part_floats].  x needs no gradient (layer-0 dgrad skipped). */
int vpc_encoder_bwd(const float* x, const float* enc_img, int npass, const uint8_t* const* mask,
                    const float* const* h1, const float* const* h2, const float* const* dmean,
                    const float* const* dlogvar, int lat_pitch, int mask_augm, int precision, float* partials,
                    int* nblocks_out, long B, int d, int L, void* stream);

/* ---- decoder: Reg_VAE.decoder, src/models/VAE.py:397-401 ----------------------------------------- */

/* xhat = sigmoid(MLP(z)) */
int vpc_decoder_fwd(const float* z, const float* dec_img, float* xhat, long B, int d, int L, void* stream);

/* Autograd of the above: (z, dxhat) -> dz [B][L] and decoder partial blocks (forward is recomputed). */
int vpc_decoder_bwd(const float* z, const float* dxhat, const float* dec_img, float* dz, float* partials,
                    int* nblocks_out, long B, int d, int L, void* stream);

/* ---- loss ---------------------------------------------------------------------------------------- */
/* Every entry point that computes or finalises the loss evaluates ONE generic form (VAE.py:403-467, 469-494, 1171-1208;
 * SURVEY.md Appendix A)
 *   loss * B = sum_p [ cA[p] * NLL(A_p, xhat_p) + cE[p] * NLL(A_p & ~B_p, xhat_p) ]
 *              + bq * KL(q || N(0,1)) + bp * KL(p || N(0,1)) + cr * KL(q || p) - wml * log N(z'; mu_p, var_p)
 * whose coefficients travel as one record, VpcLossCoef `co` (host memory, read before the call returns; NULL is
 * VPC_ERR_ARG; one pass: cA[1] = cE[1] = 0).  inv_B, x_logvar and npass stay arguments of their own.  It is also the head
 * of a VpcMember record (ensemble step).
 * Here NLL(m, xhat) = sum_ij [ 0.5 log 2pi + m_ij (0.5 x_logvar + (x_ij - xhat_ij)^2 / (2 exp(x_logvar))) ]
 * and z' = mean_q + eps_ml * exp(logvar_q / 2).  maskA/maskB are per-pass byte masks (maskB[p] may be
 * NULL).  Per-workgroup partial sums are written as doubles, loss_partials[nblocks][8]:
 *   0 S_A(pass 0)  1 S_E(pass 0)  2 S_A(pass 1)  3 KL0(q)  4 KL0(p)  5 KL(q||p)  6 loglik  7 S_notA(pass 0)
 * where S_* are the NLL sums WITHOUT the 0.5 log 2pi constants.  Seeds are d(loss)/d(.) times inv_B. */
typedef struct VpcLossCoef {
    float cA[2], cE[2], bq, bp, cr, wml;
} VpcLossCoef; /* 32 bytes */

/* K4: loss on materialised tensors (the model.loss(...) API).  dxhat/dmean/dlogvar NULL -> no seeds. */
int vpc_loss_fwd_bwd(const float* x, int npass, const float* const* xhat, const uint8_t* const* maskA,
                     const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* mean,
                     const float* const* logvar, const float* eps_ml, float inv_B, float x_logvar,
                     float* const* dxhat, float* const* dmean, float* const* dlogvar, double* loss_partials,
                     int max_blocks, int* nblocks_out, long B, int d, int L, void* stream);

/* Fused training path: reparameterise + decoder forward + loss + backward seeds + decoder backward in one
 * pass (nothing of size B x d is written).  Outputs the TOTAL seeds on the encoder outputs
 * (dmean[p], dlogvar[p], reparameterisation path included), decoder partial blocks and loss partials
 * (term 7 unused).  mean / logvar / eps / eps_ml / dmean / dlogvar are padded [B][16] workspaces (lat_pitch must
 * be 16; pad entries of mean / logvar must be 0 as vpc_encoder_fwd writes them, pad entries of eps are ignored).  Replaces VAE.py:389-392 (rsample), 397-401, 403-467 and their autograd. */
int vpc_decoder_fused(const float* x, const float* dec_img, int npass, const uint8_t* const* maskA,
                      const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* mean,
                      const float* const* logvar, const float* const* eps, const float* eps_ml, float inv_B,
                      float x_logvar, float* const* dmean, float* const* dlogvar, int lat_pitch, int precision,
                      float* partials, double* loss_partials, int* nblocks_out, long B, int d, int L, void* stream);

/* out9[0] = loss / B_global with the NLL constants of the B_local rows this rank processed (so that the
 * sum over data-parallel ranks is the loss of the concatenated batch), out9[1..8] = the 8 raw sums;
 * if accum != NULL, accum[0] += out9[0] (device-side epoch total, train.py:117 without a host sync). */
int vpc_loss_finalize(const double* loss_partials, int nblocks, const VpcLossCoef* co, long B_local, long B_global,
                      int d, float* out9, float* accum, void* stream);

/* vpc_reduce_partials (encoder) + vpc_reduce_partials (decoder) + vpc_loss_finalize in ONE launch: the whole
 * post-backward reduction of the fused step.  grad_out[0, n_enc) from the encoder blocks, [n_enc, n) from the
 * decoder blocks (grad_idx as returned by vpc_build_indices), out9 / accum as vpc_loss_finalize.  If state != NULL
 * (two int64 words on the device) the kernel also does state[0] += 1 (optimiser step count) and
 * state[1] += rng_inc (Philox counter offset): the per-step counters of a replayed HIP graph.
 * inv_maps (optional): the inverse maps (block position -> parameter) vpc_build_inverse_maps wrote for this
 * grad_idx.  With them - and both strides multiples of 4 floats and the block pointers 16-byte aligned, true for the
 * blocks the kernels above write - the blocks are read in layout order, 16 bytes per lane, instead of 4-byte
 * gathers through grad_idx.  The library allocates nothing and keeps no state: the caller owns the map buffer.
 * Summation order is fixed either way (reproducible), but differs between the two forms in the last bits. */
int vpc_build_inverse_maps(const int* grad_idx, int n_enc, int n, long enc_stride, long dec_stride, int* inv_out,
                           void* stream); /* inv_out: enc_stride + dec_stride ints (device) */
int vpc_reduce_step(const float* enc_partials, int enc_blocks, long enc_stride, const float* dec_partials,
                    int dec_blocks, long dec_stride, const int* grad_idx, const int* inv_maps, float* grad_out,
                    int n_enc, int n, const double* loss_partials, int loss_blocks, const VpcLossCoef* co, long B_local,
                    long B_global, int d, float* out9, float* accum, long long* state, long long rng_inc, void* stream);

/* vpc_reduce_step + vpc_adam_step in ONE launch (single process, eager): Adam is elementwise, so the thread that
 * finishes gradient i updates parameter i (and its packed-image entry) on the spot.  Same result as the two
 * calls in sequence; `step` >= 1 is the optimiser step count of THIS update. */
int vpc_reduce_step_adam(const float* enc_partials, int enc_blocks, long enc_stride, const float* dec_partials,
                         int dec_blocks, long dec_stride, const int* grad_idx, const int* inv_maps, float* grad_out,
                         int n_enc, int n, const double* loss_partials, int loss_blocks, const VpcLossCoef* co,
                         long B_local, long B_global, int d, float* out9, float* accum, float* params, float* exp_avg,
                         float* exp_avg_sq, float lr, float beta1, float beta2, float eps, long step,
                         const int* pack_idx, float* img, void* stream);
/* the same, re-packing the compact bf16 image of the whole-step kernel instead of the fp32 images: pack_idx_c / img_c of
 * vpc_step_build_indices_bf16 (a plain-bf16 step then needs no vpc_step_pack_weights_bf16 launch) */
int vpc_reduce_step_adam_bf16c(const float* enc_partials, int enc_blocks, long enc_stride, const float* dec_partials,
                         int dec_blocks, long dec_stride, const int* grad_idx, const int* inv_maps, float* grad_out,
                         int n_enc, int n, const double* loss_partials, int loss_blocks, const VpcLossCoef* co,
                         long B_local, long B_global, int d, float* out9, float* accum, float* params, float* exp_avg,
                         float* exp_avg_sq, float lr, float beta1, float beta2, float eps, long step,
                         const int* pack_idx_c, float* img_c, void* stream);

/* ---- random draws (Philox4x32-10, counter = GLOBAL element-group index + offset) -------------------
 * Data parallel: a rank that holds rows [row_lo, row_lo + B_local) of a global batch passes
 * where its shard starts, and every element gets the counter it would get in the single-process run on the
 * concatenated batch - the drawn mask_p / eps of a row do not depend on the world size. */

/* mask_out = mask_in AND (U < keep_prob): create_missing_uci(shape, rate) * mask with keep_prob = 1 - rate/100
 * (src/utils/utils.py:36-39, src/experiment_main/train.py:53-55).  mask_in NULL = all ones.  U has 16 random
 * bits (one Philox call serves 8 elements; element i uses counter (elem_lo + i) / 8 + offset): keep_prob is resolved
 * to 2^-16.  elem_lo = index of mask_out[0] in the global array (row_lo * d; 0 for a single process). */
int vpc_draw_mask(const uint8_t* mask_in, uint8_t* mask_out, long n, float keep_prob, unsigned long long seed,
                  unsigned long long offset, long elem_lo, void* stream);

/* vpc_draw_mask + vpc_fill_normal in one launch (the two per-step draws of the fused step).  If state != NULL,
 * state[1] (device) is added to both offsets.  mask_elem_lo as vpc_draw_mask's elem_lo; eps_* as vpc_fill_normal's
 * row-shard arguments. */
int vpc_draw_step(const uint8_t* mask_in, uint8_t* mask_out, long n_mask, float keep_prob, float* eps_out, long n_eps,
                  unsigned long long seed, unsigned long long offset_mask, unsigned long long offset_eps,
                  const long long* state, long mask_elem_lo, long eps_rows_local, long eps_rows_global,
                  long eps_row_lo, int eps_pitch, void* stream);

/* out ~ N(0,1): the eps of Normal.rsample() (VAE.py:389-392); one Philox call per 4 floats.  state (optional,
 * device): state[1] is added to the offset (the per-step counter of a replayed HIP graph, as vpc_draw_step).
 * rows_local == 0: flat array, group g uses counter g + offset.  rows_local > 0: out is [planes][rows_local][pitch]
 * (pitch % 4 == 0), the rows [row_lo, row_lo + rows_local) of a global [planes][rows_global][pitch] array, and a
 * group uses the counter of its position in the global array. */
int vpc_fill_normal(float* out, long n, unsigned long long seed, unsigned long long offset, const long long* state,
                    long rows_local, long rows_global, long row_lo, int pitch, void* stream);

/* The row-tiled fp32 step (8-wave kernels: d in (64, 128], d % 8 == 0, x 16-byte aligned, masks 4-byte aligned) with
 * vpc_draw_step's two draws made by the kernels that consume them - same counters, same values, one launch less.  Both run
 * the throughput shape (128-row tiles) at every B.
 * vpc_encoder_fwd_draw_f32 = vpc_draw_mask + vpc_encoder_fwd(npass 2, lat_pitch 16, precision 0): pass 0 runs on mask_in,
 * pass 1 on mask_p = mask_in AND (U < keep_prob), which the kernel draws for the mask words it holds (seed, offset_mask,
 * state, mask_elem_lo as vpc_draw_step; mask_elem_lo % 8 == 0) and stores to mask_p_out [B][d].
 * vpc_decoder_fused_draw_f32 = vpc_fill_normal + vpc_decoder_fused(lat_pitch 16, precision 0, wml == 0): eps[p] [B][16] is
 * WRITTEN - the lane that forms z draws its four values (seed, offset_eps, state as vpc_draw_step; eps[p] is plane p, rows
 * [eps_row_lo, eps_row_lo + B), of a global [npass][eps_rows_global][16] array) - and read back at the end of the pass. */
int vpc_encoder_fwd_draw_f32(const float* x, const float* enc_img, const uint8_t* mask_in, uint8_t* mask_p_out,
                             float* const* h1, float* const* h2, float* const* mean, float* const* logvar, long B, int d,
                             int L, float keep_prob, unsigned long long seed, unsigned long long offset_mask,
                             const long long* state, long mask_elem_lo, void* stream);
/* Which kernel form the last vpc_encoder_fwd / vpc_encoder_fwd_draw_f32 call of this process launched (-1: none yet): the
 * pass loop (one pass after the other over a tile) or the sweep (fp32, vector layout, plain encoder, d in (64, 128], two passes
 * in one workgroup: both passes of a tile in one sweep over the weights - the same bytes in every workspace).  VPC_ENC_SWEEP=0
 * in the environment keeps the pass loop everywhere, =1 takes the sweep wherever it is eligible; unset, only
 * vpc_encoder_fwd_draw_f32 takes it (the form it makes faster).  For tests and A/B runs. */
#define VPC_ENC_FWD_PASSES 0
#define VPC_ENC_FWD_PASSES_DRAW 1
#define VPC_ENC_FWD_SWEEP 2
#define VPC_ENC_FWD_SWEEP_DRAW 3
int vpc_encoder_fwd_last_form(void);
int vpc_decoder_fused_draw_f32(const float* x, const float* dec_img, int npass, const uint8_t* const* maskA,
                               const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* mean,
                               const float* const* logvar, float* const* eps, float inv_B, float x_logvar,
                               float* const* dmean, float* const* dlogvar, float* partials, double* loss_partials,
                               int* nblocks_out, long B, int d, int L, unsigned long long seed,
                               unsigned long long offset_eps, const long long* state, long eps_rows_global, long eps_row_lo,
                               void* stream);

/* vpc_encoder_fwd_draw_f32 + vpc_decoder_fused_draw_f32(npass 2) + vpc_encoder_bwd(npass 2, lat_pitch 16, precision 0) as three
 * phases of ONE launch (csrc/vpc_step_f32.hip): the same code per phase, the same bytes in every workspace, partial block and
 * loss partial; two kernel boundaries less.  The arguments are the union of the three entry points' (the masks of the decoder
 * and of the backward pass are {mask_in, mask_p_out}); nblocksE_out / nblocksD_out are the encoder / decoder partial-block
 * counts for vpc_reduce_step*.  The phases share one persistent grid with nothing but workgroup barriers between them, so the
 * three kernels must agree on grid and tile count: the two drawing kernels run the throughput shape at every B,
 * vpc_encoder_bwd the shape of its batch size - force_shape != 0 runs it in the throughput shape too (tests, A/B runs).  If
 * they disagree the call returns 4 and has launched nothing: the caller makes the three launches.  Records the sweep as the
 * last encoder form (vpc_encoder_fwd_last_form). */
int vpc_step_f32(const float* x, const float* enc_img, const float* dec_img, const uint8_t* mask_in, uint8_t* mask_p_out,
                 const uint8_t* const* maskB, const VpcLossCoef* co, float* const* h1, float* const* h2, float* const* mean,
                 float* const* logvar, float* const* eps, float* const* dmean, float* const* dlogvar, float inv_B,
                 float x_logvar, float* partE, float* partD, double* loss_partials, int* nblocksE_out, int* nblocksD_out,
                 long B, int d, int L, float keep_prob, unsigned long long seed, unsigned long long offset_mask,
                 unsigned long long offset_eps, const long long* state, long mask_elem_lo, long eps_rows_global,
                 long eps_row_lo, int force_shape, void* stream);

/* ---- data parallel: the step's ONE collective on the caller's stream (RCCL over xGMI) -------
 * The reference has no distributed code; these entry points exist so that the flat bucket [gradients | loss terms]
 * (37 548 + 9 floats) is all-reduced as an ordinary node of the compute stream - no hop to a communication stream,
 * capturable in the same HIP graph as vpc_reduce_step and vpc_adam_step.  librccl is opened lazily (dlopen).
 *   vpc_rccl_unique_id   rank 0: 128-byte ncclUniqueId into HOST memory; the caller ships it to the other ranks
 *                        (the Python host uses the torch.distributed process group it already has for that)
 *   vpc_rccl_comm_init   every rank, collectively: ncclCommInitRank on the CURRENT device -> opaque communicator
 *   vpc_allreduce_flat   in-place ncclAllReduce(sum, fp32) of bucket[0, count) on `stream`
 *   vpc_rccl_comm_destroy */
int vpc_rccl_unique_id(void* id128_host);
int vpc_rccl_comm_init(const void* id128_host, int nranks, int rank, void** comm_out);
int vpc_allreduce_flat(void* comm, float* bucket, long count, void* stream);
int vpc_rccl_comm_destroy(void* comm);

/* ---- active variable selection reward (config 5) -------------------------------------------------------
 * Replaces the candidate loop of active_learning_func (src/experiment_main/evaluate.py:424-433) and the
 * functions it calls, R_lindley_chain / chaini_I / chaini_II (evaluate.py:514-634): for every row n and every
 * feature u < d-1 with mask[n][u] == 0
 *     R[n][u] = 1/M sum_m [ KL_I(n,u,m) - KL_II(n,u,m) ]          (-1e4 where mask[n][u] != 0)
 * with the reference's KL expression (first term divided by the std, evaluate.py:582-583) and its carry-over of
 * the imputed target between MC samples (evaluate.py:531-536).  x [n][d], mask [n][d] bytes, im [M][n][d]
 * (MC imputations, evaluate.py:396-414), W1 [100][d] / b1 [100] = seq_encoder.0 (flat parameter views),
 * enc_img = packed encoder image; pre / stat / w1t are scratch buffers of the sizes vpc_reward_scratch returns
 * (16-byte aligned; w1t also holds the rows' candidate lists).  The target is the last column, as in the reference. */
int vpc_reward_scratch(int n, int d, int M, long* pre_floats, long* stat_floats, long* w1t_floats);
int vpc_reward_matrix(const float* x, const uint8_t* mask, const float* im, const float* W1, const float* b1,
                      const float* enc_img, float* pre, float* stat, float* w1t, float* R, int n, int d, int L, int M,
                      void* stream);

/* The same reward for the other encoder families of active_learning_func (evaluate.py:374-378, 403-409, 444-448: every
 * 'reg_vae*' / 'vanilla_vae*' / '*_EDDI*' model), selected by `kind` = the encoder's first layer:
 *   VPC_REWARD_DENSE       Reg_VAE / vanilla_VAE (VAE.py:366-395) of any width d <= 4096: W1 [100][d]
 *   VPC_REWARD_DENSE_MASK  Reg_VAE_mask / vanilla_VAE_mask (input [x*mask | mask], VAE.py:545-548): W1 [100][2d]
 *   VPC_REWARD_POINTNET    Reg_EDDI / vanilla_EDDI (VAE.py:713-741): W1 [100][K] / b1 = pnp_encoder2.0, AC [2][K][d] the
 *                          folded front-end of vpc_eddi_fold, 1 <= K <= 32 (AC and K are ignored by the other kinds)
 * w23_img = [W2 | W3] of a packed encoder image (the part from EncImg::oW2 on, 10240 floats, the same for every input width:
 * the image of layout(K, L) for the point-net trunk, 16-byte aligned).  pre / stat / w1t: vpc_reward_scratch_ex's sizes.
 * The DENSE kind at d <= 128 runs the kernels of vpc_reward_matrix.  L <= 15 (one latent tile) for every kind. */
#define VPC_REWARD_DENSE 0
#define VPC_REWARD_DENSE_MASK 1
#define VPC_REWARD_POINTNET 2
int vpc_reward_scratch_ex(int kind, int n, int d, int M, int K, long* pre_floats, long* stat_floats, long* w1t_floats);
int vpc_reward_matrix_ex(int kind, const float* x, const uint8_t* mask, const float* im, const float* W1, const float* b1,
                         const float* AC, int K, const float* w23_img, float* pre, float* stat, float* w1t, float* R, int n,
                         int d, int L, int M, void* stream);

/* ---- MNAR path (config 3): REG_notMIWAE_v2 / notMIWAE_myversion --------------------------------------
 * Reference: src/models/VAE.py:2327-2505 and :2691-2847 (encoder d->128->128 ELU + heads, K-fold replicated
 * draw, decoder L->128->128 ELU + Sigmoid / Hardtanh(-10,0) heads, self-masking missingness model).  The
 * layers are generic fp32 MFMA GEMMs (any M, N, K), the loss is one fused forward+backward kernel.
 * Activation codes: 0 none, 1 ELU, 2 Sigmoid for output features < split and Hardtanh(-10,0) from split on,
 * 3 ReLU.  All matrices row-major with an explicit row pitch (ld*, in floats).  `precision` as above (0 f32, 1 bf16x3,
 * 2 bf16): the operands stay fp32 in memory and in LDS and are converted in registers - no separate weight images. */

/* y[M][N] = act(x[M][K] w[N][K]^T + bias[N])            nn.Linear + activation (VAE.py:2343-2363) */
int vpc_linear_fwd(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, long M, int N,
                   int K, int act, int act_split, int precision, void* stream);

/* dx[M][K] = ((dy * act'(y_gate)) w[N][K]) * act_prev'(x_out)     data gradient of the same layer.
 * y_gate (the layer's outputs, activation code `gate`) may be NULL when dy is already the pre-activation
 * gradient; x_out (the layer's inputs = previous layer's outputs, activation `act_prev`) may be NULL. */
int vpc_linear_dgrad(const float* dy, long lddy, const float* y_gate, long ldyg, int gate, int gate_split,
                     const float* w, const float* x_out, long ldx, int act_prev, float* dx, long lddx, long M, int N,
                     int K, int precision, void* stream);

/* dw[N][K] (+)= (dy * act'(y_gate))^T x,  db[N] (+)= column sums; split over M into per-workgroup partials in
 * `scratch` (vpc_linear_wgrad_scratch floats) that are summed in a fixed order.  db may be NULL.
 * dw == NULL: only the partials are written (one launch); vpc_linear_wgrad_reduce then sums the partials of up to 8 such
 * calls - each with its own scratch buffer, HOST arrays of n_layers entries - in ONE launch, with the same summation order
 * (the fused MNAR step: 6 weight gradients, 7 launches instead of 12). */
long vpc_linear_wgrad_scratch(long M, int N, int K);
int vpc_linear_wgrad(const float* dy, long lddy, const float* y_gate, long ldyg, int gate, int gate_split,
                     const float* x, long ldx, float* dw, float* db, float* scratch, long scratch_floats, long M, int N,
                     int K, int accumulate, int precision, void* stream);
int vpc_linear_wgrad_reduce(int n_layers, const float* const* scratch, const long* M, const int* N, const int* K,
                            float* const* dw, float* const* db, const int* accumulate, void* stream);

/* ---- the same layer for FEW rows (csrc/vpc_rows.hip): M <= vpc_rows_max_rows() = 128 rows, 1 <= N, K <= 1024, fp32 only.
 * The split is over output features, the contraction of the weight gradient (at most 128 rows) stays inside one wave, and
 * nothing is summed by a second launch: there is neither `precision` nor `scratch`.  Activation codes, the gate, the row
 * pitches and the 16-byte / scalar access rule are those of vpc_linear_*.  M < 1, N < 1, K < 1, a pitch below its width or
 * a NULL mandatory pointer: bad argument; M > 128, N > 1024 or K > 1024: unsupported shape.  Nothing is launched then.
 * Results are bitwise reproducible (no atomics, one summation order). */
int vpc_rows_max_rows(void);

/* y[M][N] = act(x[M][K] w[N][K]^T + bias[N])            nn.Linear + activation (VAE.py:1878-1900, :2343-2363); bias may be
 * NULL. */
int vpc_rows_fwd(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, long M, int N, int K,
                 int act, int act_split, void* stream);

/* One layer's whole backward in ONE launch (autograd of the same layer: what vpc_linear_dgrad, vpc_linear_wgrad and
 * vpc_linear_wgrad_reduce do in three):
 *   dw[N][K] (+)= (dy * gate'(y_gate))^T x,  db[N] (+)= column sums     (dw == NULL: skipped, x / db unused; db may be NULL)
 *   dx[M][K]  = ((dy * gate'(y_gate)) w[N][K]) * act_prev'(x_out)       (dx == NULL: skipped, w / x_out unused)
 * x [M][K] (pitch ldx) is the layer's input; x_out (pitch ldxo, may be NULL) is the same activations as the data gradient
 * gates with them, activation code act_prev.  y_gate may be NULL (dy is the pre-activation gradient).  accumulate != 0
 * adds to dw / db.  dw and dx both NULL: bad argument. */
int vpc_rows_bwd(const float* dy, long lddy, const float* y_gate, long ldyg, int gate, int gate_split, const float* w,
                 const float* x, long ldx, const float* x_out, long ldxo, int act_prev, float* dx, long lddx, float* dw,
                 float* db, long M, int N, int K, int accumulate, void* stream);

/* z[b*K+k][:] = mean[b] + eps[b][k] * exp(logvar[b]/2), heads = [mean L | logvar L]; eps NULL -> z = mean
 * (encoder, VAE.py:2382-2391 / :2753-2765) and its backward (sum over the K replicas, plus g_heads if given). */
int vpc_nm_sample(const float* heads, long ldh, const float* eps, float* z, long ldz, long B, int K, int L,
                  void* stream);
int vpc_nm_sample_bwd(const float* dz, long lddz, const float* eps, const float* heads, long ldh, const float* g_heads,
                      long ldg, float* out, long ldo, long B, int K, int L, void* stream);
/* out = x * mask (float mask; encoder input VAE.py:2379 / :2750) */
int vpc_nm_mul(const float* x, const float* mask, float* out, long n, void* stream);

/* Loss of REG_notMIWAE_v2 (mask_p != NULL; VAE.py:2398-2471) or notMIWAE_myversion (mask_p == NULL, eps_kl =
 * the fresh draw of VAE.py:2791-2798; :2774-2823) and, when g_xm_q != NULL, every gradient: with respect to the
 * decoder heads (x_mean | x_logvar, rows b*K+k, pitch ldg_*), the encoder heads ([B][2L]), and W / b.
 * Masks are float 0/1.  out8 (device doubles) = loss, loss_q, loss_p, KL_reg, NLL_E, mean RE_q, sum lse_q,
 * sum lse_p; means run over B_global rows (data parallel: sum out8[0] over ranks).  xm_imp != NULL also
 * writes the self-normalised imputation sum_k softmax(-l_w)_k x_mean[b][k] (llh_eval branch :2458-2461).
 * loss_f32 / accum (optional, device): loss as a float, and accum[0] += loss (train.py:117 without a host sync).
 * state (optional, two int64 on the device): state[0] += 1 (optimiser step count, read by vpc_adam_step's step_dev)
 * and state[1] += rng_inc (Philox counter offset read by vpc_nm_prep) - the per-step counters of a replayed graph.
 * gated != 0: g_xm / g_xl are gradients w.r.t. the head PRE-activations (already through Sigmoid' / Hardtanh'), so
 * vpc_linear_dgrad / vpc_linear_wgrad take them with y_gate = NULL (the fused step; autograd callers pass 0). */
int vpc_nm_loss_blocks(long B);
long vpc_nm_loss_scratch(long B, int d);
int vpc_nm_loss(const float* x, const float* mask, const float* mask_p, const float* xm_q, const float* xl_q, long ld_q,
                const float* xm_p, const float* xl_p, long ld_p, const float* heads_q, const float* heads_p, long ldh,
                const float* W, const float* b, const float* eps_kl, float* g_xm_q, float* g_xl_q, long ldg_q,
                float* g_xm_p, float* g_xl_p, long ldg_p, float* g_heads_q, float* g_heads_p, long ldgh, float* gW,
                float* gb, int accumulate_wb, float* xm_imp, void* scratch, long scratch_bytes, double* out8,
                float* loss_f32, float* accum, long long* state, long long rng_inc, int gated, long B, long B_global,
                int K, int d, int L, double alpha, void* stream);

/* Per-step input preparation of the fused MNAR step in one launch: mask_p = mask * (U < keep_prob) (float masks,
 * create_missing_uci * mask, train.py:53-55; Philox counter = element index / 4 + offset), xin[0:B] = x * mask and,
 * when mask_p_out != NULL, xin[B:2B] = x * mask_p (the two encoder passes stacked); when n_eps > 0 also
 * eps_out[0:n_eps] ~ N(0,1) (counter offset_eps).  If state != NULL, state[1] (device) is added to both offsets:
 * the per-step counter of a replayed HIP graph (bumped by vpc_nm_loss).  elem_lo (multiple of 4) = index of x[0] in
 * the global [B_global][d] array and eps_* = row-shard description of eps_out as in vpc_fill_normal (rows = data rows,
 * pitch = K * L): the draws of a row do not depend on the data-parallel sharding. */
int vpc_nm_prep(const float* x, const float* mask, float* mask_p_out, float* xin, long B, int d, float keep_prob,
                float* eps_out, long n_eps, unsigned long long seed, unsigned long long offset,
                unsigned long long offset_eps, const long long* state, long elem_lo, long eps_rows_local,
                long eps_rows_global, long eps_row_lo, int eps_pitch, void* stream);

/* ---- layer-fused K-fold decoder of the regularised MNAR step, plain bf16 MFMA inputs (csrc/vpc_nmdec.hip) ----------
 * Replaces, for REG_notMIWAE_v2 and notMIWAE_myversion at obs_dim = 128 (latent_dim <= 15, 8 <= K <= 64; hidden width 128), the launches
 *   vpc_nm_sample -> 3 x vpc_linear_fwd -> vpc_nm_loss -> 3 x (vpc_linear_wgrad, vpc_linear_dgrad) -> vpc_nm_sample_bwd
 * of one training step with precision = 2 (src/models/VAE.py:2382-2396 / :2753-2772 K-fold rsample + decoder, :2398-2471 /
 * :2774-2823 loss, and
 * their autograd, src/experiment_main/train.py:115): the K replicas of a few data rows are one workgroup tile, and no
 * array of B * K rows crosses HBM.  Same mathematics, gradient weights and bf16 rounding points as that chain, except
 * that ELU' is taken from the bf16-rounded activation and the bias gradients are column sums of the bf16-rounded dY
 * (tests/test_nmdec.py; oracle/notmiwae_oracle.py mirrors both).
 *   vpc_nmdec_applicable     1 when vpc_nmdec_step covers the shape (VPC_NMDEC=0 in the environment: never)
 *   vpc_nmdec_layout         floats of the weight image, floats of one partial block, most workgroups of a launch
 *   vpc_nmdec_build_indices  HOST tables over the model's flat parameter buffer (n entries, order
 *                            [W b | We1 be1 We2 be2 Wmu Wls bmu bls | Wd1 bd1 Wd2 bd2 Wxm Wxl bxm bxl]): pack_idx as
 *                            vpc_step_pack_weights_bf16 reads it (decoder + missingness model, then the encoder), grad_idx =
 *                            position of the parameter's gradient inside a partial block (-1: not produced here)
 *   vpc_nmdec_step           mask_p != NULL (REG_notMIWAE_v2): heads [2 B][ldh] = encoder (mean | logvar) of the q rows, then
 *                            of the p rows; eps [2 B K][L] likewise.  mask_p == NULL (notMIWAE_myversion): heads [B][ldh],
 *                            eps [2][B K][L] = the decoder's draws, then the draws of its Monte-Carlo KL; alpha is ignored.
 *                            dht [2 B][2 L] receives d loss / d heads (sum over K of dz + the analytic KL gradients);
 *                            grad (flat, n entries) receives the entries grad_idx names (fixed-order sum of the blocks; inv_idx,
 *                            optional device table [part_floats]: parameter index of a block position or -1 - the blocks are
 *                            then read in layout order, 16 bytes per lane);
 *                            out8 / loss_f32 / accum / state / rng_inc / B_global / alpha as vpc_nm_loss.
 *                            part: max_blocks x part_floats floats, stat_part: max_blocks x 5 doubles (caller-owned). */
int vpc_nmdec_applicable(long B, int K, int d, int L);
int vpc_nmdec_layout(long B, int K, int d, int L, int* img_floats, long* part_floats, int* max_blocks);
int vpc_nmdec_build_indices(int d, int L, int hid, int* pack_idx, int* grad_idx, int n);
/* the encoder forward of the same step (seq_encoder + q_mu | q_logstd, VAE.py:2378-2384 / :2749-2756) as ONE launch instead of three
 * vpc_linear_fwd: xin [R][128] = x * mask of the stacked passes -> h1, h2 [R][128] (fp32, ELU applied: the backward GEMMs read them),
 * heads [R][2 L]; img = the image buffer vpc_nmdec_layout sizes and vpc_nmdec_build_indices' pack_idx fills (the encoder's weights sit
 * behind the decoder's).  Rounding points of vpc_linear_fwd with precision 2. */
int vpc_nmenc_fwd(const float* img, const float* xin, float* h1, float* h2, float* heads, long R, int d, int L, void* stream);
/* the encoder BACKWARD of the same step (autograd of VAE.py:2378-2384 behind d loss / d heads) as one launch + the fixed-order
 * reduction of its partial blocks, instead of three vpc_linear_wgrad, two vpc_linear_dgrad and vpc_linear_wgrad_reduce:
 * dht [R][2 L] (vpc_nmdec_step's), h1 / h2 / xin [R][128] as vpc_nmenc_fwd saw / stored them -> the gradients of We1 be1 We2 be2
 * [Wmu ; Wls] [bmu ; bls] inside grad (flat, layout of vpc_nmdec_build_indices) at the entries inv_idx names.  Rounding points of the
 * precision-2 GEMMs (bf16 dY, X, W operands; ELU' from the fp32 h), except that the bias gradients sum the bf16-rounded dY.
 * part: scratch of part_floats floats, 16-byte aligned - vpc_nmdec_step's partial blocks serve once that call is enqueued.
 * vpc_nmenc_build_indices: inv_idx [*part_floats ints] = flat parameter index of a block position or -1 (NULL: size query only). */
int vpc_nmenc_bwd(const float* img, const float* xin, const float* h1, const float* h2, const float* dht, float* part,
                  long part_floats, const int* inv_idx, float* grad, long R, int d, int L, void* stream);
int vpc_nmenc_build_indices(int d, int L, int hid, int* inv_idx, long* part_floats, int n);
/* everything behind vpc_nmenc_fwd of a SINGLE-DEVICE step (train.py:87-101, 116: loss.backward(); optimizer.step()) in three launches:
 * vpc_nmdec_step's tile kernel, vpc_nmenc_bwd's tile kernel and one tail launch that sums both sets of partial blocks into grad
 * (fixed order), applies torch.optim.Adam (as vpc_adam_step, host step count) to every gradient it finishes, re-packs that
 * parameter's place in the bf16 image (pack_idx of vpc_nmdec_build_indices; img is read by the tile kernels and updated by the tail)
 * and writes the loss terms.  Arguments as those two calls; inv_idx (decoder blocks) is required; part_e: its own scratch of
 * part_e_floats floats (max_blocks x vpc_nmenc_build_indices' part_floats suffices) - both sets are live until the tail. */
int vpc_nm_fused_bwd_step(float* img, const float* x, const float* mask, const float* mask_p, const float* xin, const float* h1,
                          const float* h2, const float* heads, long ldh, const float* eps, float* dht, float* part,
                          double* stat_part, float* part_e, long part_e_floats, const int* inv_idx, const int* inv_idx_e,
                          float* grad, int n, double* out8, float* loss_f32, float* accum, long B, long B_global, int K, int d,
                          int L, double alpha, float* params, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                          float beta2, float eps_adam, long step, const int* pack_idx, void* stream);
int vpc_nmdec_step(const float* img, const float* x, const float* mask, const float* mask_p, const float* heads, long ldh,
                   const float* eps, float* dht, float* part, double* stat_part, const int* grad_idx, const int* inv_idx,
                   float* grad, int n, double* out8, float* loss_f32, float* accum, long long* state, long long rng_inc, long B, long B_global,
                   int K, int d, int L, double alpha, void* stream);

/* ---- PNP / EDDI encoder front-end (Reg_EDDI / vanilla_EDDI, src/models/VAE.py:719-733, 903-917) ----------
 * agg[b] = sum_j mask[b][j] relu(W [x_bj, x_bj E_j, t_j] + c), W = pnp_encoder1.0.weight [K][2+K], c its bias,
 * E = type_pars1 [d][K], t = type_bias1 [d].  The layer folds per feature into pre = x_bj A_j + C_j
 * (vpc_eddi_fold writes AC = [A | C], each [K][d]); nothing of size B*d*(2+K) is materialised.  d <= 128, K <= 32.
 * mask2 != NULL stacks a second pass over the same x (the mask / mask_p passes of one training step): agg and dagg
 * then have 2B rows ([pass][B][K]) and the gradients are those of both passes.
 * vpc_eddi_front_bwd: gradients of (E, t, W, c) from dagg; scratch of vpc_eddi_front_scratch(rows, d, K) floats with
 * rows = B or 2B. */
int vpc_eddi_fold(const float* E, const float* tb, const float* Wp, const float* cp, float* AC, int d, int K,
                  void* stream);
int vpc_eddi_front_fwd(const float* x, const uint8_t* mask, const uint8_t* mask2, const float* AC, float* agg, long B,
                       int d, int K, void* stream);
long vpc_eddi_front_scratch(long rows, int d, int K);
int vpc_eddi_front_bwd(const float* x, const uint8_t* mask, const uint8_t* mask2, const float* AC, const float* dagg,
                       const float* E, const float* tb, const float* Wp, float* scratch, long scratch_floats, float* gE,
                       float* gtb, float* gWp, float* gcp, int accumulate, long B, int d, int K, void* stream);

/* ---- the same front-end at image width (Reg_EDDI_mnist / vanilla_EDDI_mnist, src/models/VAE.py:62-77, 255-270) -------
 * Same arguments, layouts and meaning as the four entry points above, for any d <= 1024 (784: MNIST), K <= 32
 * (csrc/vpc_eddi.hip: the folded table is tiled along k, 4 rows of A and C per workgroup over all d features, because
 * [2][K][d] no longer fits LDS).  vpc_eddiw_front_bwd recomputes the ReLU gates and sums its per-workgroup partial blocks in a
 * fixed order: the same inputs give bitwise the same gradients.  scratch: vpc_eddiw_front_scratch(rows, d, K) floats. */
int vpc_eddiw_fold(const float* E, const float* tb, const float* Wp, const float* cp, float* AC, int d, int K,
                   void* stream);
int vpc_eddiw_front_fwd(const float* x, const uint8_t* mask, const uint8_t* mask2, const float* AC, float* agg, long B,
                        int d, int K, void* stream);
long vpc_eddiw_front_scratch(long rows, int d, int K);
int vpc_eddiw_front_bwd(const float* x, const uint8_t* mask, const uint8_t* mask2, const float* AC, const float* dagg,
                        const float* E, const float* tb, const float* Wp, float* scratch, long scratch_floats, float* gE,
                        float* gtb, float* gWp, float* gcp, int accumulate, long B, int d, int K, void* stream);

/* ---- whole-step kernel, plain bf16 (csrc/vpc_step.hip): vpc_encoder_fwd + vpc_decoder_fused + vpc_encoder_bwd with
 * precision 2 as ONE launch per 128-row tile - the step body of src/experiment_main/train.py:87-115 for Reg_VAE /
 * vanilla_VAE (src/models/VAE.py:496-507 forward, :403-467 loss, autograd backward) with nothing but x, the masks and eps
 * read from HBM and nothing but the gradient partial blocks and loss terms written.  obs_dim in (64, 128], obs_dim % 4 == 0,
 * plain (not mask-augmented) encoder, any batch (the grid is min(tiles, CUs) workgroups looping over their tiles).
 * Takes its own weight image (all six layers, bf16, 98.5 KB): vpc_step_layout_bf16 gives its size in floats and the
 * kernel's dynamic-LDS bytes; vpc_step_build_indices_bf16 fills HOST arrays pack_idx_c[n_params] / img_template_c[floats];
 * vpc_step_pack_weights_bf16 writes img_c from the flat parameters (after every optimiser step): entry i of pack_idx_c >= 0 is
 * the u16 position of parameter i inside the image, < 0 the dword -(idx + 1) of a value that stays fp32, INT_MIN = skip.
 * vpc_step_fused_bf16: arguments as vpc_decoder_fused (mask[p] is the encoder mask AND the first loss mask of pass p;
 * eps[p] [B][16] padded rows, eps_ml likewise); partE / partD / loss_partials are written in the layouts of
 * vpc_encoder_bwd / vpc_decoder_fused (*nblocks_out blocks each), so vpc_reduce_step(_adam) consumes them unchanged.
 * The kernel runs two sweeps over a workgroup's tiles (decoder-side gradients, then encoder-side gradients: csrc/vpc_step.hip);
 * the seeds on (mean | logvar) cross from one to the other through `workspace` as packed bf16, 16 bytes per lane. */
/* 1 when the library runs a (B, d, L, npass) plain-bf16 step through vpc_step_fused_bf16: obs_dim in (64, 128], obs_dim % 4 == 0, any
 * batch (VPC_TILE=64 / VPC_STEP_FUSED=0 in the environment: the three small-shape kernels, for A/B runs), else 0 */
int vpc_step_fused_applicable(long B, int d, int L, int npass);
/* floats of the caller-owned `workspace` of vpc_step_fused_bf16 for B rows (16-byte aligned; contents are scratch) */
long vpc_step_workspace_floats(long B);
int vpc_step_layout_bf16(int d, int L, int* img_floats, int* lds_bytes);
int vpc_step_build_indices_bf16(int d, int L, int* pack_idx_c, float* img_template_c);
int vpc_step_pack_weights_bf16(const float* flat_params, const int* pack_idx_c, float* img_c, int n, void* stream);
int vpc_step_fused_bf16(const float* x, const float* img_c, int npass, const uint8_t* const* mask,
                        const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* eps,
                        const float* eps_ml, float inv_B, float x_logvar,
                        float* partE, float* partD, double* loss_partials, float* workspace, int* nblocks_out, long B,
                        int d, int L, void* stream);

/* ---- small-batch whole-step kernel, fp32 (csrc/vpc_small.hip): the same step as vpc_encoder_fwd -> vpc_decoder_fused ->
 * vpc_encoder_bwd with precision 0 (src/experiment_main/train.py:87-115; src/models/VAE.py:496-507, 403-467) as ONE launch in
 * which a workgroup owns a 16-row tile and the feature tiles of every layer are split over its 8 waves - for the reference's
 * own batch sizes (64 / 128, Data/imputation_args*.json) and the per-GPU shards of strong scaling, where the row-tiled kernels
 * are three serial single-tile latencies.  Weights are read from the fp32 images of vpc_build_indices / vpc_pack_weights in
 * global memory; partial blocks and loss terms in the layouts of vpc_encoder_bwd / vpc_decoder_fused.  Plain (not
 * mask-augmented) encoder, obs_dim % 4 == 0, B <= 32 x CUs rows (one workgroup per tile); maskB[p] must be NULL or mask[1 - p].
 * vpc_step_small_max_rows: batches up to this many rows take this path inside FusedTrainer (0 = off; env VPC_STEP_SMALL). */
long vpc_step_small_max_rows(void);
int vpc_step_small_f32(const float* x, const float* enc_img, const float* dec_img, int npass, const uint8_t* const* mask,
                       const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* eps,
                       const float* eps_ml, float inv_B, float x_logvar, float* partE,
                       float* partD, double* loss_partials, int* nblocks_out, long B, int d, int L, void* stream);
/* vpc_draw_step + vpc_step_small_f32 in ONE launch: every workgroup draws the mask_p bytes (mask[1] = mask_in & keep; mask_in NULL:
 * none - vanilla_VAE) and the normals of ITS 16 rows (eps_out = eps[0], planes [B][16]: eps[1] and eps_ml follow it, n_eps floats
 * in all) with the Philox counters vpc_draw_step would use - seed, offsets, state, mask_elem_lo and the eps_* shard description
 * (eps_pitch 16, eps_rows_local = B) as there -, stores them where the step reads them, and runs the step: the same draws
 * (train.py:53-55, VAE.py:389-392), one launch less at the batch sizes where a launch is a fifth of the step. */
int vpc_step_small_draw_f32(const float* x, const float* enc_img, const float* dec_img, int npass, const uint8_t* const* mask,
                            const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* eps,
                            const float* eps_ml, float inv_B, float x_logvar,
                            float* partE, float* partD, double* loss_partials, int* nblocks_out, long B, int d, int L,
                            const uint8_t* mask_in, float keep_prob, float* eps_out, long n_eps, unsigned long long seed,
                            unsigned long long offset_mask, unsigned long long offset_eps, const long long* state,
                            long mask_elem_lo, long eps_rows_local, long eps_rows_global, long eps_row_lo, int eps_pitch,
                            void* stream);
/* vpc_step_small_f32 / vpc_step_small_draw_f32 for the mask-augmented classes Reg_VAE_mask / vanilla_VAE_mask
 * (src/models/VAE.py:545-555, 1031-1041: encoder input cat([x * mask, mask]); src/experiment_main/train.py:87-115): the images are
 * those of the mask-augmented layout (vpc_layout_sizes / vpc_build_indices with mask_augm = 1), and the kernel's input stage builds
 * the 2 d_real wide input - x_f m_f, then m_f, then zeros up to the tile edge - per pass, with mask[p].  d_real is obs_dim; d is
 * the ROW PITCH of x and the masks, 4 ceil(d_real / 4), whose padding columns carry mask 0 (draws are made at that pitch).
 * VPC_ERR_SHAPE when d_real < 1, d_real > d, d - d_real > 3, d % 4 != 0 or 2 d_real > 128; VPC_ERR_ARG on the pointer and
 * alignment conditions of the plain entries; nothing is launched in either case.  All other arguments as there. */
int vpc_step_small_aug_f32(const float* x, const float* enc_img, const float* dec_img, int npass, const uint8_t* const* mask,
                           const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* eps,
                           const float* eps_ml, float inv_B, float x_logvar, float* partE,
                           float* partD, double* loss_partials, int* nblocks_out, long B, int d, int d_real, int L, void* stream);
int vpc_step_small_aug_draw_f32(const float* x, const float* enc_img, const float* dec_img, int npass, const uint8_t* const* mask,
                                const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* eps,
                                const float* eps_ml, float inv_B, float x_logvar,
                                float* partE, float* partD, double* loss_partials, int* nblocks_out, long B, int d, int d_real, int L,
                                const uint8_t* mask_in, float keep_prob, float* eps_out, long n_eps, unsigned long long seed,
                                unsigned long long offset_mask, unsigned long long offset_eps, const long long* state,
                                long mask_elem_lo, long eps_rows_local, long eps_rows_global, long eps_row_lo, int eps_pitch,
                                void* stream);
/* vpc_step_small_f32 / vpc_step_small_draw_f32 for the point-net classes Reg_EDDI / vanilla_EDDI: replaces the launch chain
 * fold -> front-end -> three trunk GEMMs -> fused decoder -> trunk wgrads / dgrads -> front-end backward of the step
 * (src/models/VAE.py:713-741, 897-925 encoder with the point-net front-end :719-733, 903-917; :743-747 decoder; :749-813, 933-964
 * loss; src/experiment_main/train.py:87-115).  The images are those of vpc_build_indices_pointnet.  `front` holds the front-end
 * parameters in flat order (type_pars1 [d_real][K] | type_bias1 [d_real] | pnp_encoder1.0.weight [K][2+K] | .bias [K]); every
 * workgroup folds them (A_j = w_x + W_E E_j, C_j = w_t t_j + c) into LDS, builds agg[r][k] = sum_j m[r][j] relu(x[r][j] A_j[k] +
 * C_j[k]) as the trunk's input, and in the backward pass goes on from dh1 to dagg = dh1 . W1 and the front-end's gradient block of
 * its 16 rows: front_partials [tiles][2][K][d] = (dA | dC), both passes summed, no atomics.  Tile 0 copies `front` to
 * front_snapshot [d_real K + d_real + K (2 + K) + K] for the chain rule of vpc_reduce_step_adam_eddi.  d_real is obs_dim; d is the
 * ROW PITCH of x and the masks, 4 ceil(d_real / 4), mask 0 in the padding (draws are made at that pitch).
 * VPC_ERR_SHAPE when K < 1, K > 32, d > 64, d % 4 != 0, d_real < 1, d_real > d or d - d_real > 3 (no instantiation: K <= 16 / 32
 * against obs_dim <= 16 / 32 / 64); VPC_ERR_ARG on null pointers, x / images not 16-byte or front / front_partials /
 * front_snapshot not 4-byte aligned, and the conditions of the plain entries; nothing is launched in either case. */
int vpc_step_small_eddi_f32(const float* x, const float* enc_img, const float* dec_img, int npass, const uint8_t* const* mask,
                            const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* eps,
                            const float* eps_ml, float inv_B, float x_logvar, float* partE,
                            float* partD, double* loss_partials, int* nblocks_out, long B, int d, int d_real, int L, int K,
                            const float* front, float* front_partials, float* front_snapshot, void* stream);
int vpc_step_small_eddi_draw_f32(const float* x, const float* enc_img, const float* dec_img, int npass, const uint8_t* const* mask,
                                 const uint8_t* const* maskB, const VpcLossCoef* co, const float* const* eps,
                                 const float* eps_ml, float inv_B, float x_logvar,
                                 float* partE, float* partD, double* loss_partials, int* nblocks_out, long B, int d, int d_real, int L,
                                 int K, const float* front, float* front_partials, float* front_snapshot,
                                 const uint8_t* mask_in, float keep_prob, float* eps_out, long n_eps, unsigned long long seed,
                                 unsigned long long offset_mask, unsigned long long offset_eps, const long long* state,
                                 long mask_elem_lo, long eps_rows_local, long eps_rows_global, long eps_row_lo, int eps_pitch,
                                 void* stream);
/* The tail behind them, ONE launch (train.py:114-117; replaces the reductions, vpc_eddi_front_bwd's tail and vpc_adam_step of the
 * chain): vpc_reduce_step_adam over the trunk and decoder blocks and the loss terms (layout-order reduction: inv_maps of
 * vpc_build_inverse_maps is required), and for the front-end the fixed-order sum of front_partials over the tiles, the chain rule
 * from (dA, dC) to (type_pars1, type_bias1, pnp_encoder1.0.weight, .bias) - dE[j][e] = sum_k W_E[k][e] dA[k][j], dt[j] = sum_k
 * w_t[k] dC[k][j], dW[k] = [sum_j dA | sum_j dA E[j][.] | sum_j dC t[j]], dc[k] = sum_j dC[k][j], with E, t, W read from
 * front_snapshot - and Adam.  grad_out, params, exp_avg, exp_avg_sq: the model's flat vectors [trunk | decoder | front-end];
 * n = trunk + decoder parameters (pack_idx [n], img: the point-net images, re-packed).  d = obs_dim, d_pitch the row pitch of the
 * front-end blocks (<= 64). */
int vpc_reduce_step_adam_eddi(const float* enc_partials, int enc_blocks, long enc_stride, const float* dec_partials,
                              int dec_blocks, long dec_stride, const int* inv_maps, float* grad_out, int n,
                              const double* loss_partials, int loss_blocks, const VpcLossCoef* co, long B_local, long B_global,
                              int d, float* out9, float* accum, float* params, float* exp_avg, float* exp_avg_sq, float lr,
                              float beta1, float beta2, float eps, long step, const int* pack_idx, float* img,
                              const float* front_partials, int front_blocks, const float* front_snapshot, int K, int d_pitch,
                              void* stream);

/* ---- ensemble step: G independent models of ONE architecture in one pair of launches (csrc/vpc_small.hip, csrc/vpc_misc.hip).
 * The reference trains lists of tiny runs: src/experiment_main/imputation.py:21-39 wraps the step loop of
 * src/experiment_main/train.py:28-117 in `for missing in [...]: for alpha in [...]:` per split, every run at batch 64, where the
 * single-model step occupies 4 workgroups.  Here workgroup (tile t, member g) runs the tile body of vpc_step_small(_draw)_f32 on
 * member g's buffers, and the reduction + Adam launch runs per member on blockIdx.y: every member gets, bit for bit, the partial
 * blocks, gradient, loss terms, Adam state and re-packed images its stand-alone vpc_step_small(_draw)_f32 + vpc_reduce_step_adam
 * would give it.
 *
 * Member table: G device-resident VpcMember records (64 bytes each, read with ordinary loads), everything that may differ
 * between members beside their buffers.  Shared, by value: npass, the Philox offsets, inv_B, x_logvar, B, d, L (one class, shape and
 * reg_type, so every member consumes the same counters; member g draws with ITS seed in its own element space, as the unsharded
 * vpc_step_small_draw_f32 does: eps_rows_local = eps_rows_global = B, mask_elem_lo = 0).
 *
 * Buffers: the pointers are member 0's; member g's slice starts g * strides[k] ELEMENTS further (host array of VPC_MS_COUNT longs):
 *   VPC_MS_X, VPC_MS_MASK     x [B][d] fp32, mask [B][d] bytes; stride 0 = one batch shared by every member
 *   VPC_MS_MASK_P             mask_p [B][d] bytes (npass 2; written when draw != 0; 0 = shared, injected only)
 *   VPC_MS_EPS                eps planes [nplanes][B][16] fp32: eps_q, eps_p (npass 2), eps_ml (nplanes 3)
 *   VPC_MS_IMG                the fp32 weight images: enc_img and dec_img of member g are both g * stride floats further
 *   VPC_MS_PARTE, _PARTD      partial blocks: member g's tiles-per-member blocks [tiles][enc / dec_part_floats]
 *   VPC_MS_LOSS               loss partials [tiles][8] doubles
 *   VPC_MS_PARAM              rows of params / exp_avg / exp_avg_sq / grad_out (vpc_reduce_step_adam_multi only)
 * Strides of fp32 arrays are multiples of 4, of byte masks multiples of 4; a non-zero stride holds the member's slice.
 *
 * Limits (VPC_ERR_SHAPE / VPC_ERR_ARG outside them, never a fault): fp32, plain encoder, d % 4 == 0, d <= 128, L <= 15, tiles per
 * member = ceil(B / 16) <= 2 x CUs as vpc_step_small_f32, and G x tiles <= VPC_MULTI_MAX_BLOCKS workgroups; the caller's partial-block
 * strides must hold `tiles` blocks per member (8192 workgroups admit G = 2048 at B = 64; a block is ~193 KB of partials).
 * order: 0 = workgroup id g * tiles + t; 1 = members partitioned over (id % 8), all tiles of a member on ids of one residue (the
 * workgroups that share an XCD's L2 - a speed choice, the results are the same). */
#define VPC_MULTI_MAX_BLOCKS 8192
typedef struct VpcMember {
    VpcLossCoef co;                      /* loss coefficients (cA[1] = cE[1] = 0 for npass 1) */
    float keep_prob;                     /* mask_p keep probability */
    float lr;                            /* Adam learning rate */
    unsigned long long seed;             /* Philox seed of the member's draws */
    int use_maskB;                       /* != 0: the E terms of pass 0 use mask & ~mask_p (maskB = {mask_p, NULL}) */
    int reserved[3];
} VpcMember;
enum { VPC_MS_X = 0, VPC_MS_MASK, VPC_MS_MASK_P, VPC_MS_EPS, VPC_MS_IMG, VPC_MS_PARTE, VPC_MS_PARTD, VPC_MS_LOSS, VPC_MS_PARAM,
       VPC_MS_COUNT };
/* draw == 0: mask_p and the eps planes are given; draw != 0: drawn in the launch (mask_p = mask & keep, then the normals). */
int vpc_step_small_multi_f32(const float* x, const uint8_t* mask, uint8_t* mask_p, float* eps, const float* enc_img,
                             const float* dec_img, const VpcMember* members, int G, int npass, int nplanes, int draw,
                             unsigned long long offset_mask, unsigned long long offset_eps, float inv_B, float x_logvar,
                             float* partE, float* partD, double* loss_partials, const long* strides, long B, int d, int L,
                             int order, void* stream);
/* vpc_reduce_step_adam with blockIdx.y = member (train.py:114-117 per member): member g's `blocks` partial blocks -> row g of
 * grad_out (same summation order), its loss terms -> out9[g][9] and accum[g] +=, Adam with the member's lr on row g of params /
 * exp_avg / exp_avg_sq (rows VPC_MS_PARAM floats apart) and the re-pack of ITS image (pack_idx shared, img rows VPC_MS_IMG apart).
 * The step count (bias corrections) is shared.  inv_maps (vpc_build_inverse_maps) is required. */
int vpc_reduce_step_adam_multi(const float* enc_partials, const float* dec_partials, const double* loss_partials, int blocks,
                               long enc_stride, long dec_stride, const long* strides, const int* inv_maps,
                               const VpcMember* members, int G, float* grad_out, long B, int d, float* out9, float* accum,
                               float* params, float* exp_avg, float* exp_avg_sq, float beta1, float beta2, float eps, long step,
                               const int* pack_idx, float* img, void* stream);

/* ---- the ensemble step for the mask-augmented and the point-net families: the same pair of launches with the tile bodies of
 * vpc_step_small_aug(_draw)_f32 (Reg_VAE_mask / vanilla_VAE_mask, src/models/VAE.py:510-667, 995-1116) and of
 * vpc_step_small_eddi(_draw)_f32 (Reg_EDDI / vanilla_EDDI, VAE.py:670-853, 856-992) per (tile, member) workgroup, around the step
 * loop of src/experiment_main/train.py:87-117 under the drivers' loops of src/experiment_main/imputation.py:21-39.  Member g gets,
 * bit for bit, what its stand-alone small-batch step and tail give it.  Arguments as vpc_step_small_multi_f32 /
 * vpc_reduce_step_adam_multi, and besides:
 *   d_real    the members' obs_dim; d is the ROW PITCH 4 ceil(d_real / 4) of x and the masks (mask 0 in the padding), and the pitch
 *             the draws of draw != 0 are made at (point-net members keep their stand-alone stream, which is drawn at the pitch
 *             obs_dim: the caller asks for draws only where d == d_real)
 *   K, front, front_partials, front_snapshot (point-net)   as vpc_step_small_eddi_f32; the pointers are member 0's.  `front` lies
 *             inside the member's row [trunk | decoder | front-end] of the parameter stack: member g's is strides[VPC_MS_PARAM]
 *             floats further.  Every member's tile 0 leaves that member's snapshot.
 * The stride vector of these three entries has VPC_MS_COUNT_FAMILIES slots: the nine of the entries above, then
 *   VPC_MS_PARTF   front_partials [tiles][2][K][d] floats of a member (point-net)
 *   VPC_MS_SNAP    front_snapshot [d_real K + d_real + K (2 + K) + K] floats of a member (point-net)
 * (vpc_step_small_multi_aug_f32 reads the first eight only).  The images are those of the mask-augmented layout (vpc_build_indices
 * with mask_augm = 1), resp. the point-net layout (vpc_build_indices_pointnet), rows VPC_MS_IMG apart.
 * Limits: those of the single-model entries - 2 d_real <= 128 (mask-augmented); K <= 32 and d <= 64 (point-net); d % 4 == 0,
 * d - d_real <= 3, L <= 15 - and those of the ensemble entries - tiles <= 2 x CUs, G x tiles <= VPC_MULTI_MAX_BLOCKS, every member's
 * slice inside its stride, read-only inputs may be shared (stride 0), written ones (mask_p and eps under draw != 0, the partial
 * blocks, front_partials, front_snapshot) not.  VPC_ERR_SHAPE / VPC_ERR_ARG outside them; nothing is launched then. */
enum { VPC_MS_PARTF = VPC_MS_COUNT, VPC_MS_SNAP, VPC_MS_COUNT_FAMILIES };
int vpc_step_small_multi_aug_f32(const float* x, const uint8_t* mask, uint8_t* mask_p, float* eps, const float* enc_img,
                                 const float* dec_img, const VpcMember* members, int G, int npass, int nplanes, int draw,
                                 unsigned long long offset_mask, unsigned long long offset_eps, float inv_B, float x_logvar,
                                 float* partE, float* partD, double* loss_partials, const long* strides, long B, int d, int d_real,
                                 int L, int order, void* stream);
int vpc_step_small_multi_eddi_f32(const float* x, const uint8_t* mask, uint8_t* mask_p, float* eps, const float* enc_img,
                                  const float* dec_img, const VpcMember* members, int G, int npass, int nplanes, int draw,
                                  unsigned long long offset_mask, unsigned long long offset_eps, float inv_B, float x_logvar,
                                  float* partE, float* partD, double* loss_partials, const long* strides, long B, int d, int d_real,
                                  int L, int K, const float* front, float* front_partials, float* front_snapshot, int order,
                                  void* stream);
/* vpc_reduce_step_adam_eddi with blockIdx.y = member (the tail of vpc_step_small_multi_eddi_f32; the mask-augmented members take
 * vpc_reduce_step_adam_multi with the mask-augmented layout's maps): per member the trunk and decoder blocks, the loss terms with
 * the coefficients of record g, the fixed-order sum of ITS front_partials, the chain rule from ITS front_snapshot and Adam with
 * the member's lr on row g of params / exp_avg / exp_avg_sq [trunk | decoder | front-end] - the front-end in place.  n = trunk +
 * decoder parameters (pack_idx [n]); d = obs_dim, d_pitch the row pitch of the front-end blocks (<= 64). */
int vpc_reduce_step_adam_eddi_multi(const float* enc_partials, const float* dec_partials, const double* loss_partials, int blocks,
                                    long enc_stride, long dec_stride, const long* strides, const int* inv_maps,
                                    const VpcMember* members, int G, float* grad_out, int n, long B, int d, float* out9,
                                    float* accum, float* params, float* exp_avg, float* exp_avg_sq, float beta1, float beta2,
                                    float eps, long step, const int* pack_idx, float* img, const float* front_partials,
                                    const float* front_snapshot, int K, int d_pitch, void* stream);

/* ---- ensemble evaluation: the evaluate stage of G members over a list of batches and M Monte-Carlo passes in one pair of launches
 * (csrc/vpc_evalsmall.hip).  Replaces the loop body of eval_vae, src/experiment_main/evaluate.py:136-297, for Reg_VAE / vanilla_VAE:
 * model.forward (src/models/VAE.py:496-507, :1153-1169), model.loss(llh_eval=True, stage='evaluate') (VAE.py:410-420: the q pass
 * only - mask_p, alpha and the p pass reach no output) and the RMSE on ~mask (evaluate.py:229-234).
 *
 * Tables (device-resident, long long):
 *   tiles   [n_tiles][4]    data row of the tile's first row | valid rows 1..16 | draw row of its first row | batch index.  A tile
 *                           lies inside ONE batch.  Data row and draw row are separate: M passes over an unshuffled data set read
 *                           the same x rows with M different eps, without an M-fold copy.  0 <= data row, data row + valid <= N;
 *                           0 <= draw row, draw row + valid <= R (an entry outside these reads nothing and counts as zero).
 *   batches [n_batches][4]  rows in the batch | MC pass index | first tile | tiles (a batch's tiles are consecutive)
 *   passes  [M][2]          first batch | batches (a pass's batches are consecutive)
 * eps: draw == 0: planes [G or 1][R][16] of normals (row r = draw row r, columns >= L ignored); draw != 0: drawn in registers,
 * no buffer: the eps of draw row r, columns 4 q .. 4 q + 3, under member g is what vpc_fill_normal writes at float index 16 r + 4 q
 * of a flat [R x 16] array with seed members[g].seed and this call's `offset` (one Philox counter per group: the call consumes 4 R).
 * Members: the VpcMember table of the ensemble step (seed; co.bq = the member's KL weight); pointers are member 0's, member g's slice
 * g * strides[k] ELEMENTS further (VPC_MS_X, VPC_MS_MASK, VPC_MS_EPS: 0 = shared by all members; VPC_MS_IMG; VPC_MS_LOSS = the
 * records, in doubles).  d = row pitch of x and mask (multiple of 4: the host pads), d_real <= d the model's obs_dim: columns
 * [d_real, d) are padding and enter neither the sums on mask (zero mask bytes) nor the sums on its complement.
 *
 * vpc_eval_small_multi_f32: one record of VPC_EVAL_TERMS doubles per (member, tile), with t = (x_hat - x)^2 / (2 sigma^2) +
 * x_logvar / 2:  sum mask t | sum (1 - mask) t | sum (1 - mask)(x_hat - x)^2 | sum (1 - mask) | sum over rows of KL(q || N(0, I)).
 * A pure function of its inputs (no atomics).  One launch holds at most max_blocks workgroups (0: VPC_EVAL_MAX_BLOCKS); the entry
 * walks the tile table in chunks (a lower max_blocks gives the same records: it lets a small case walk the chunk loop).  Limits as the ensemble step: fp32, plain encoder, d % 4 == 0, d <= 128, L <= 15, G <= 65535;
 * VPC_ERR_ARG / VPC_ERR_SHAPE outside them (d_real > d and misaligned pointers included), never a fault. */
#define VPC_EVAL_TERMS 5
#define VPC_EVAL_MAX_BLOCKS 65536
int vpc_eval_small_multi_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img, const float* dec_img,
                             const VpcMember* members, int G, const long long* tiles, long n_tiles, long N, long R, int draw,
                             unsigned long long offset, float x_logvar, double* part, const long* strides, int d, int d_real,
                             int L, int max_blocks, void* stream);
/* vpc_eval_small_multi_f32 for G Reg_VAE_mask / vanilla_VAE_mask members (model.loss, evaluate stage: src/models/VAE.py:570-580,
 * :1053-1060; the encoder input [x*mask | mask] of VAE.py:545-548 is built in the kernel's input stage): same arguments, tables,
 * draw rule, records and chunking.  d is the row pitch 4 ceil(d_real / 4) of x and mask (mask 0 in the padding), d_real the
 * model's obs_dim, the images are those of the mask-augmented layout (vpc_build_indices with mask_augm = 1), rows VPC_MS_IMG
 * apart.  2 d_real > 128 or d - d_real > 3: VPC_ERR_SHAPE; otherwise limits and errors as vpc_eval_small_multi_f32. */
int vpc_eval_small_multi_aug_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img, const float* dec_img,
                                 const VpcMember* members, int G, const long long* tiles, long n_tiles, long N, long R, int draw,
                                 unsigned long long offset, float x_logvar, double* part, const long* strides, int d, int d_real,
                                 int L, int max_blocks, void* stream);
/* ... and for G Reg_EDDI / vanilla_EDDI members (VAE.py:757-767, :935-950 - vanilla_EDDI computes the imputed term in every
 * stage; the point-net front-end of VAE.py:719-733, :903-917 runs as the kernel's input stage, folded per workgroup as in
 * vpc_step_small_multi_eddi_f32).  Images of the point-net layout (vpc_build_indices_pointnet); K = emb_dim; `front` is member 0's
 * front-end parameters (E [d_real][K] | t [d_real] | W [K][2 + K] | c [K]) inside its row [trunk | decoder | front-end] of the
 * parameter stack, member g's strides[VPC_MS_PARAM] floats further - read in place, no copy.  The eps draw does not depend on the
 * pitch of x: the entry draws at every d_real.  K < 1, K > 32 or d_real > 64: VPC_ERR_SHAPE; a front that is null or not 4-byte
 * aligned, or a VPC_MS_PARAM stride below the front-end's size: VPC_ERR_ARG; otherwise as vpc_eval_small_multi_aug_f32. */
int vpc_eval_small_multi_eddi_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img, const float* dec_img,
                                  const VpcMember* members, int G, const long long* tiles, long n_tiles, long N, long R, int draw,
                                  unsigned long long offset, float x_logvar, double* part, const long* strides, int d, int d_real,
                                  int L, int K, const float* front, int max_blocks, void* stream);
/* The records -> out[G][4] = (rmse, elbo, negll, negll_imp), blockIdx.y = member, fp64, fixed summation order (family-independent:
 * the three forward entries above share it).  Per batch of n_b
 * rows: negll = (S_A + n_b d_real log(2 pi) / 2) / n_b and negll_imp likewise from S_I (masked entries contribute the constant,
 * as _finish / VAE.py:414-419), elbo = negll + co.bq KL / n_b, rmse = sqrt(SQ / CNT) - 0 / 0 = NaN for a batch without an
 * unobserved entry, as evaluate.py:232-234.  Then the mean over the batches of a pass and the mean over the passes
 * (evaluate.py:238-245). */
int vpc_eval_reduce_multi(const double* part, const long long* batches, long n_batches, const long long* passes, int M,
                          const VpcMember* members, int G, long part_stride, long n_tiles, int d_real, float* out, void* stream);

/* ---- ensemble acquisition: the loop of active_learning_func (src/experiment_main/evaluate.py:300-511) for G members of one
 * ensemble, a fixed number of launches per acquisition step and no host round trip (csrc/vpc_evalsmall.hip, csrc/vpc_reward.hip).
 *
 * vpc_impute_small_multi_f32: the M Monte-Carlo forwards of evaluate.py:396-414 (and of :380-392): the forward of
 * vpc_eval_small_multi_f32 - same arguments, tile table, fences, draw rule and max_blocks chunking, same arithmetic up to x_hat -
 * that WRITES instead of summing.  mode 0: out[g][draw row][0..d_real) = x_hat, a dense [R][d_real] array per member (real rows
 * and real columns only); under the table of (n, batch_size = n, M) draw row m n + i is row i of pass m, so out is im [M][n][d].
 * mode 1: out[g][draw row] = (x_hat[T] - x[T])^2 of the target column T = d_real - 1.  out_stride: floats between members
 * (>= R d_real / >= R).  Limits and errors as vpc_eval_small_multi_f32; mode outside {0, 1}: VPC_ERR_ARG. */
int vpc_impute_small_multi_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img, const float* dec_img,
                               const VpcMember* members, int G, const long long* tiles, long n_tiles, long N, long R, int draw,
                               unsigned long long offset, float x_logvar, int mode, float* out, long out_stride,
                               const long* strides, int d, int d_real, int L, int max_blocks, void* stream);
/* vpc_impute_small_multi_f32 for G Reg_VAE_mask / vanilla_VAE_mask members (the forwards of evaluate.py:396-414 and :380-392 on
 * VAE.py:570-580, :1053-1060; the encoder input [x*mask | mask] of VAE.py:545-548 is built in the kernel's input stage): the forward
 * of vpc_eval_small_multi_aug_f32 - d the row pitch 4 ceil(d_real / 4), images of the mask-augmented layout, its shape limits and
 * pointer checks - with mode / out / out_stride as vpc_impute_small_multi_f32. */
int vpc_impute_small_multi_aug_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img, const float* dec_img,
                                   const VpcMember* members, int G, const long long* tiles, long n_tiles, long N, long R, int draw,
                                   unsigned long long offset, float x_logvar, int mode, float* out, long out_stride,
                                   const long* strides, int d, int d_real, int L, int max_blocks, void* stream);
/* ... and for G Reg_EDDI / vanilla_EDDI members (the same forwards on VAE.py:757-767, :935-950; front-end VAE.py:719-733, :903-917
 * as the input stage): the forward of vpc_eval_small_multi_eddi_f32 - images of the point-net layout, K = emb_dim, `front` member
 * 0's front-end inside its row of the parameter stack, strides[VPC_MS_PARAM] floats between members, its limits (K <= 32,
 * d_real <= 64) and checks - with mode / out / out_stride as vpc_impute_small_multi_f32. */
int vpc_impute_small_multi_eddi_f32(const float* x, const uint8_t* mask, const float* eps, const float* enc_img,
                                    const float* dec_img, const VpcMember* members, int G, const long long* tiles, long n_tiles,
                                    long N, long R, int draw, unsigned long long offset, float x_logvar, int mode, float* out,
                                    long out_stride, const long* strides, int d, int d_real, int L, int K, const float* front,
                                    int max_blocks, void* stream);
/* target_mse of evaluate.py:390-392 per member: out[g * out_stride] = mean of sq[g * sq_stride + 0..R) (the mode-1 squared errors
 * of the R = M n draw rows), accumulated in fp64 in a fixed order (no atomics), stored as float. */
int vpc_target_mse_multi(const float* sq, long sq_stride, long R, int G, float* out, long out_stride, void* stream);
/* vpc_reward_matrix (evaluate.py:424-433 around :514-634) with a member dimension: the same three launches with blockIdx.y =
 * member, for the plain model at d <= 128.  Pointers are member 0's; member g's slice starts g * strides[k] ELEMENTS further
 * (host array of VPC_RM_COUNT longs):
 *   VPC_RM_X      x [n][d] (0 = shared)            VPC_RM_MASK   mask [n][d] bytes          VPC_RM_IM     im [M][n][d]
 *   VPC_RM_PARAM  W1 [100][d] and b1 [100]: both g * stride floats further (rows of a parameter stack)
 *   VPC_RM_IMG    enc_img (rows of an image stack; multiple of 4)
 *   VPC_RM_PRE, VPC_RM_STAT, VPC_RM_W1T   the workspaces, vpc_reward_scratch_multi's sizes per member (multiples of 4)
 *   VPC_RM_R      R [n][d-1]
 * R[g] is bit for bit what vpc_reward_matrix gives on member g's operands (same per-item arithmetic and in-wave summation order;
 * only the order in which items are handed out differs).  chunk: the workspaces hold `chunk` members; members go through them in
 * ceil(G / chunk) rounds of three launches (the inputs and R are indexed by the member, the workspaces by the member's place in its
 * round).  Limits as vpc_reward_matrix. */
enum { VPC_RM_X = 0, VPC_RM_MASK, VPC_RM_IM, VPC_RM_PARAM, VPC_RM_IMG, VPC_RM_PRE, VPC_RM_STAT, VPC_RM_W1T, VPC_RM_R, VPC_RM_COUNT };
int vpc_reward_scratch_multi(int n, int d, int M, long* pre_floats, long* stat_floats, long* w1t_floats);
int vpc_reward_matrix_multi(const float* x, const uint8_t* mask, const float* im, const float* W1, const float* b1,
                            const float* enc_img, float* pre, float* stat, float* w1t, float* R, int G, int chunk,
                            const long* strides, int n, int d, int L, int M, void* stream);
/* vpc_reward_matrix_ex (evaluate.py:424-433 around :514-634, the encoders of VAE.py:545-548 and :713-741) with a member dimension,
 * for kind = VPC_REWARD_DENSE_MASK (2 d <= 128) and VPC_REWARD_POINTNET (d <= 64, K <= 32) - the members the family forwards above
 * serve; VPC_REWARD_DENSE: VPC_ERR_ARG (vpc_reward_matrix_multi).  The three launches of vpc_reward_matrix_ex with blockIdx.y =
 * member and its choice of kernels per kind, so R[g] is bit for bit what vpc_reward_matrix_ex gives on member g's operands.
 * Pointers are member 0's; the stride vector has VPC_RM_COUNT_EX longs: the nine slots of vpc_reward_matrix_multi, where
 *   VPC_RM_PARAM  W1 [100][2 d] (DENSE_MASK) or [100][K] (POINTNET) and b1 [100], rows of a parameter stack
 *   VPC_RM_IMG    w23_img = [W2 | W3] of a packed encoder image (10240 floats, 16-byte aligned; multiple of 4)
 *   VPC_RM_PRE, VPC_RM_STAT, VPC_RM_W1T   vpc_reward_scratch_multi_ex's sizes per member
 * and then
 *   VPC_RM_AC     AC [2][K][d], the folded front-end of vpc_eddi_fold_multi (POINTNET; ignored by DENSE_MASK, as AC and K are).
 * chunk as vpc_reward_matrix_multi.  2 d > 128 / d > 64, K < 1, K > 32, L > 15: VPC_ERR_SHAPE; a member slice outside its stride, a
 * misaligned workspace or w23_img, a null AC under POINTNET: VPC_ERR_ARG; nothing is launched in either case. */
enum { VPC_RM_AC = VPC_RM_COUNT, VPC_RM_COUNT_EX };
int vpc_reward_scratch_multi_ex(int kind, int n, int d, int M, int K, long* pre_floats, long* stat_floats, long* w1t_floats);
int vpc_reward_matrix_multi_ex(int kind, const float* x, const uint8_t* mask, const float* im, const float* W1, const float* b1,
                               const float* AC, int K, const float* w23_img, float* pre, float* stat, float* w1t, float* R, int G,
                               int chunk, const long* strides, int n, int d, int L, int M, void* stream);
/* The fold of the point-net front-end (VAE.py:719-727: A_j = w_x + W_E E_j, C_j = w_t t_j + c) for G members in one launch:
 * vpc_eddi_fold on member g's front-end (E [d][K] | t [d] | W [K][2 + K] | c [K], front_stride floats after member 0's: its row of
 * the parameter stack, read in place) -> AC0 + g * AC_stride, [2][K][d], bit for bit vpc_eddi_fold's output.  The acquisition loop
 * calls it once per run: the parameters do not change inside one.  Limits as vpc_eddi_fold; a stride below its slice: VPC_ERR_ARG. */
int vpc_eddi_fold_multi(const float* front0, long front_stride, float* AC0, long AC_stride, int G, int d, int K, void* stream);
/* The acquisition of evaluate.py:435-440 per (member, row): i_opt = the lowest index among the maxima of R[g][row][0..d-1)
 * (torch.argmax on finite input), mask[g][row][i_opt] = 1 (bytes, rows mask_pitch apart; mask2, if not NULL, is the same mask kept at
 * a second row pitch - the forward reads rows padded to a multiple of 4 columns, the reward rows of d), action[g][row] = i_opt with
 * rows action_pitch ints apart (the step's column of an action history [n][d-1]). */
int vpc_acquire_multi(const float* R, long R_stride, uint8_t* mask, long mask_stride, int mask_pitch, uint8_t* mask2,
                      long mask2_stride, int mask2_pitch, int* action, long action_stride, int action_pitch, int G, int n, int d,
                      void* stream);

/* ---- MIWAE path: MIWAE / Reg_MIWAE (csrc/vpc_miw.hip) ------------------------------------------------------------
 * Reference: src/models/VAE.py:3011-3134 and :3137-3301.  Encoder d->128->128 ReLU -> [mean L | raw L] and decoder
 * L->128->128 ReLU -> [mean d | scale d | df d] run on vpc_linear_fwd / dgrad / wgrad (ACT_RELU, last layer ACT_NONE);
 * these entry points add the softplus scale of the sampler, the Student-t decoder heads and the importance-weighted
 * bound.  fp32 throughout; masks are float 0/1; `R` = data rows of the stacked passes, `S` = num_samples. */

/* z[r*S+s][:] = mean[r] + softplus(raw[r]) * eps[r][s][:] (eps NULL -> z = mean), heads [R][mean L | raw L] the encoder
 * head GEMM; hact (optional) [R][mean L | softplus(raw) L].  VAE.py:3059-3070 / :3188-3200 (Normal(mean, scale).rsample()). */
int vpc_miw_sample(const float* heads, float* hact, const float* eps, float* z, long R, int S, int L, void* stream);
/* out [R][2L] = d / d heads: mean <- sum_s dz + g_hact[mean]; raw <- (sum_s dz * eps + g_hact[scale]) * softplus'(raw).
 * dz [R*S][L] and g_hact [R][2L] may each be NULL. */
int vpc_miw_sample_bwd(const float* dz, const float* eps, const float* heads, const float* g_hact, float* out, long R,
                       int S, int L, void* stream);
/* y_act[m] = (sigmoid | softplus + 0.001 | softplus + 3) of y_raw[m] = [mean d | scale d | df d], [M][3d] each (decoder,
 * VAE.py:3072-3076; Softplus with beta 1, threshold 20); the backward maps d / d y_act to d / d y_raw. */
int vpc_miw_heads(const float* y_raw, float* y_act, long M, int d, void* stream);
int vpc_miw_heads_bwd(const float* y_raw, const float* g_act, float* g_raw, long M, int d, void* stream);

/* Loss of Reg_MIWAE (mask_p != NULL; VAE.py:3204-3265) or MIWAE (mask_p == NULL; :3078-3100) and, when g_y_q != NULL,
 * its gradients with respect to the decoder heads (rows b*S+s, pitch ldg; raw != 0: the y_* are the raw head GEMM output
 * and the gradients are w.r.t. it, raw == 0: the activated (mean | scale | df)) and the ACTIVATED encoder heads
 * [B][mean L | scale L] (heads_*, g_heads_*).  eps_* [B][S][L] = the fresh draws of loss() (:3087 / :3216 / :3237).
 * pairing VPC_MIW_PAIR_REFERENCE reproduces the reference's [S, B] reshape of the (row, sample)-ordered likelihood sums
 * against the permuted prior / posterior terms (:3078-3091, :3209-3240): slot (i, j) pairs the likelihood of flat row
 * i*B + j with the prior / posterior term of row j, sample i.  VPC_MIW_PAIR_PER_ROW pairs both terms of row j, sample i
 * (equal to B single-row calls; the batched eval_miwae).  out8 (device doubles) = loss, nb_q, nb_p, KL_reg, reg_like,
 * sum logpxobsgivenz_imp / (B * 5000), sum lse_q, sum lse_p.  xm_imp != NULL: [B][d] llh_eval imputation with the q
 * weights (:3096-3098 / :3267-3269).  loss_f32 / accum optional as in vpc_nm_loss.  Three launches (per-row sums, per-slot
 * log-sum-exp, gradients + fixed-order loss reduction) through `scratch` (vpc_miw_loss_scratch bytes, 8-byte aligned). */
#define VPC_MIW_PAIR_REFERENCE 0
#define VPC_MIW_PAIR_PER_ROW 1
long vpc_miw_loss_scratch(long B, int S);
int vpc_miw_loss(const float* x, const float* mask, const float* mask_p, const float* y_q, const float* y_p, long ldy,
                 int raw, const float* heads_q, const float* heads_p, const float* eps_q, const float* eps_p,
                 float* g_y_q, float* g_y_p, long ldg, float* g_heads_q, float* g_heads_p, float* xm_imp,
                 void* scratch, long scratch_bytes, double* out8, float* loss_f32, float* accum, long B, int S, int d,
                 int L, double alpha, int pairing, void* stream);

/* Small-batch step of the family (csrc/vpc_miw_small.hip): the GEMM chains of the training step (VAE.py:3011-3134 /
 * :3137-3301 forward, src/experiment_main/train.py:102-117) as two kernels and a tail, for obs_dim <= 32, latent_dim <= 16,
 * RB = 1 .. 4 data rows per workgroup.  R = rows of the stacked passes ([q ; p] for Reg_MIWAE), S = num_samples; params =
 * the flat parameter buffer in state_dict order; the buffers are MIWTrainer's workspace ([R][128] h1 h2, [R][2L] heads hact
 * gh dht, [R*S][L] z and the sampling planes eps, [R*S][128] g1 g2, [R*S][3d] Y G).  Every entry returns VPC_ERR_ARG before
 * any launch for a shape outside the limits, a NULL pointer or a short partial buffer.
 *   vpc_miw_small_workspace  floats of the partial buffer (one block of all parameters per compute unit); 0 outside the limits
 *   vpc_miw_small_fwd        xin, eps -> h1, h2, heads, hact = (mean | softplus), z = mean + eps * scale, g1, g2, raw heads Y
 *   vpc_miw_small_bwd        G = d loss / d Y and gh = d loss / d hact (vpc_miw_loss, raw = 1) -> dht and one partial block
 *                            of all twelve gradients per workgroup (persistent grid, workgroup g owns row blocks g, g + grid, ..)
 *   vpc_miw_small_tail       partial blocks summed in workgroup order into grad (state_dict order), then flat Adam with
 *                            vpc_adam_step's update (train.py:116) */
long vpc_miw_small_workspace(int d, int L);
int vpc_miw_small_fwd(const float* params, const float* xin, const float* eps, float* h1, float* h2, float* heads,
                      float* hact, float* z, float* g1, float* g2, float* Y, long R, int S, int d, int L, int RB,
                      void* stream);
int vpc_miw_small_bwd(const float* params, const float* xin, const float* eps, const float* h1, const float* h2,
                      const float* heads, const float* z, const float* g1, const float* g2, const float* G,
                      const float* gh, float* dht, float* part, long part_floats, long R, int S, int d, int L, int RB,
                      void* stream);
int vpc_miw_small_tail(const float* part, long part_floats, long R, int RB, int d, int L, float* grad, float* params,
                       float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps, long step,
                       void* stream);

/* The small-batch step for G MIWAE or G Reg_MIWAE members of one (obs_dim <= 32, latent_dim <= 16, num_samples) in the same
 * seven kernels, whatever G: the six reg_MIWAE* / vanilla_MIWAE* lines of Data/imputation_args.json under the drivers' loops
 * `for missing: for alpha:` (src/experiment_main/imputation.py:21-39) as one launch set per batch.  Every multi kernel runs the
 * stand-alone kernel's body (one piece of code for both forms) on member g's slices, so member g computes bit for bit what
 * the stand-alone entries compute for it; no float atomics.
 * Members: G device-resident VpcMiwMember records (24 bytes, ordinary loads) - what may differ from member to member
 * besides parameters and data.  Pointers are member 0's.  Every workspace is the dense stack [G][..] of the stand-alone
 * buffer of that name (xin [G][R][d], eps [G][2 P][B][S][L] with the P sampling planes first, h1 h2 [G][R][128], heads hact gh
 * dht [G][R][2L], z [G][R S][L], g1 g2 [G][R S][128], Y Gy [G][R S][3d], mask_p [G][B][d]); x and mask are [B][d] shared by all
 * members (stride 0) or [G][..] with a member stride >= B d floats; parameters, gradient and the Adam moments are rows of
 * [G][row_stride] stacks, row_stride >= n_params.  partial blocks: [G][blocks_per_member][n_params] floats
 * (vpc_miw_multi_workspace; G = 64, 32 blocks and d = 12, L = 10 (n = 43 320): 355 MB).
 *   vpc_miw_multi_prep         (train.py:102-104 mask_p draw, VAE.py:3059-3061 / :3188-3190 x * mask, the rsample() draws of
 *                              :3066 / :3087 / :3196 / :3216 / :3237) member g: vpc_nm_prep's mask_p, stacked xin and, with draw != 0,
 *                              all 2 P eps planes, with seed_g and keep_prob_g and the counters of an unsharded stand-alone step
 *                              (mask: element index / 4 + offset, eps: group index + offset_eps).  draw == 0: mask_p is read
 *                              (injected), eps is not touched.  mask_p NULL: MIWAE (P = 1).
 *   vpc_miw_small_fwd_multi    (VAE.py:3049-3076 / :3178-3206) vpc_miw_small_fwd per member: grid = ceil(R / RB) x G workgroups
 *   vpc_miw_loss_multi         (VAE.py:3078-3100 / :3208-3265) vpc_miw_loss(raw = 1, ldy = ldg = 3d) per member in the same
 *                              three launches; the pairing stays inside a member; alpha = alpha_g; out8 [G][8], loss_f32 [G],
 *                              accum [G]; scratch = G x vpc_miw_loss_scratch(B, S) bytes
 *   vpc_miw_small_bwd_multi    (the backward of train.py:115) member g gets blocks_per_member workgroups, workgroup j walks its
 *                              row blocks j, j + blocks_per_member, .. and writes partial block (g, j).  blocks_per_member ==
 *                              ceil(R / RB) <= CUs is the stand-alone grid: the same bits; fewer blocks: another summation order
 *   vpc_miw_small_tail_multi   (train.py:116) member g's partial blocks summed in block order into grad[g], flat Adam with lr_g
 * order (fwd, bwd): 0 = grid (blocks, G), member-major; 1 = grid (8 x blocks, ceil(G / 8)), all workgroups of a member on one
 * XCD (its parameters through one L2).  Same bits.
 * VPC_ERR_ARG before any launch: d > 32, L > 16, RB outside 1 .. 4, a NULL pointer, G outside 1 .. VPC_MIW_MULTI_MAX_MEMBERS,
 * a member stride below its slice (x / mask: 0 or >= B d; rows: >= n_params), a partial buffer below
 * G x blocks_per_member x n_params floats, blocks_per_member outside 1 .. min(ceil(R / RB), CUs), a scratch below G members',
 * or blocks x G > VPC_MIW_MULTI_MAX_BLOCKS workgroups in the forward or backward launch. */
#define VPC_MIW_MULTI_MAX_BLOCKS 65536
#define VPC_MIW_MULTI_MAX_MEMBERS 4096
typedef struct VpcMiwMember {
    unsigned long long seed; /* Philox key of the member's draws */
    float alpha;             /* Reg_MIWAE: loss = nb_q + alpha (KL_reg - nb_q + nb_p - reg_like) */
    float keep_prob;         /* 1 - p_missingness / 100 */
    float lr;
    int reserved;
} VpcMiwMember;
long vpc_miw_multi_workspace(int G, int blocks_per_member, int d, int L);
int vpc_miw_multi_prep(const float* x, long x_stride, const float* mask, long mask_stride, float* mask_p, float* xin,
                       float* eps, const VpcMiwMember* members, int G, int draw, long B, int S, int d, int L,
                       unsigned long long offset, unsigned long long offset_eps, void* stream);
int vpc_miw_small_fwd_multi(const float* params, long param_stride, const float* xin, const float* eps, float* h1, float* h2,
                            float* heads, float* hact, float* z, float* g1, float* g2, float* Y, int G, long R, int S, int d,
                            int L, int RB, int order, void* stream);
int vpc_miw_loss_multi(const float* x, long x_stride, const float* mask, long mask_stride, const float* mask_p, const float* Y,
                       const float* hact, const float* eps, float* Gy, float* gh, void* scratch, long scratch_bytes,
                       double* out8, float* loss_f32, float* accum, const VpcMiwMember* members, int G, long B, int S, int d,
                       int L, int pairing, void* stream);
int vpc_miw_small_bwd_multi(const float* params, long param_stride, const float* xin, const float* eps, const float* h1,
                            const float* h2, const float* heads, const float* z, const float* g1, const float* g2,
                            const float* Gy, const float* gh, float* dht, float* part, long part_floats, int G,
                            int blocks_per_member, long R, int S, int d, int L, int RB, int order, void* stream);
int vpc_miw_small_tail_multi(const float* part, long part_floats, int G, int blocks_per_member, int d, int L, float* grad,
                             float* params, float* exp_avg, float* exp_avg_sq, long row_stride, const VpcMiwMember* members,
                             float beta1, float beta2, float eps, long step, void* stream);

/* Streaming importance-weighted imputation of the family (csrc/vpc_miw_impute.hip), for obs_dim <= 32, latent_dim <= 16:
 * what src/experiment_main/evaluate.py:89-113 computes one row at a time through the llh_eval branch of MIWAE.loss /
 * Reg_MIWAE.loss (VAE.py:3078-3099 / :3204-3258) - x_mean of S samples weighted by the softmax of their log-weights - for B
 * rows in two launches and without writing a decoder row: a workgroup owns one row and one chunk of s_chunk samples (rounded
 * up to a multiple of 16 here) and leaves (running max, running sum, weighted sums) in its slot of `part`; the merge
 * combines a row's chunks in chunk order.  Only the q side enters (:3255-3257), so there is no mask_p.  x, mask (0 / 1
 * floats) [B][d]; params = the flat parameter buffer in state_dict order; xm [B][d]; lse [B] or NULL: the per-row
 * log-sum-exp of the log-weights (the per-row pairing's IW bound before the mean).  eps [2][B][S][L] = the sampler's draw
 * and the fresh draw of :3087 / :3216, or NULL: both are drawn in the kernel (Philox; counter = (offset + row0 + row) in the
 * high word, 4 * sample + latent / 4 in the low word, one Philox stream per plane - independent of s_chunk and the grid),
 * and vpc_miw_impute_draws writes exactly those values.  VPC_ERR_ARG before any launch for a shape outside the limits, a
 * NULL required pointer, a short partial buffer or offset + row0 + B > 2^32.
 *   vpc_miw_impute_scratch  floats of the partial buffer, B * ceil(S / s_chunk16) * (2 + d); 0 outside the limits */
long vpc_miw_impute_scratch(long B, int S, int d, int L, int s_chunk);
int vpc_miw_impute(const float* params, const float* x, const float* mask, const float* eps, unsigned long long seed,
                   unsigned long long offset, long row0, float* part, long part_floats, float* xm, float* lse, long B, int S,
                   int d, int L, int s_chunk, void* stream);
int vpc_miw_impute_draws(float* eps_out, long B, int S, int L, unsigned long long seed, unsigned long long offset, long row0,
                         void* stream);

/* Streaming importance-weighted imputation of the MNAR path (csrc/vpc_nm_impute.hip), for obs_dim <= 128, latent_dim <= 16:
 * what src/experiment_main/evaluate.py:13-69 computes one row at a time through the llh_eval branch of
 * REG_notMIWAE_v2.loss / notMIWAE_myversion.loss (VAE.py:2398-2461 / :2774-2813) - xm = sum_k softmax(-l_w_q)_k x_recon_q[:, k]
 * (:2458-2461 / :2810-2813) over S samples, l_w with the self-masking missingness model (:2407-2435 / :2777-2802) - for B rows
 * in two launches and without writing a decoder row: a workgroup owns one row and one chunk of s_chunk samples (rounded up to
 * a multiple of 16 here) and leaves (running max, running sum, weighted sums) in its slot of `part`; the merge combines a
 * row's chunks in chunk order.  Only the q side enters, so there is no mask_p and no alpha.  regularised != 0:
 * REG_notMIWAE_v2 (analytic KL, :2404); 0: notMIWAE_myversion (Monte-Carlo KL on a fresh draw, :2791-2798).  x, mask (0 / 1
 * floats) [B][d]; params = the model's flat parameter buffer ([W b | encoder | decoder], the head pairs adjacent); xm
 * [B][d]; lse [B] or NULL: the per-row log-sum-exp of -l_w.  eps [2][B][S][L] = the sampler's draw and the fresh draw (plane
 * b is not read for the regularised class), or NULL: both are drawn in the kernel by the rule of vpc_miw_impute, and
 * vpc_miw_impute_draws writes exactly those values.  VPC_ERR_ARG before any launch for a shape outside the limits, a NULL
 * required pointer, a short partial buffer or offset + row0 + B > 2^32.
 *   vpc_nm_impute_scratch  floats of the partial buffer, B * ceil(S / s_chunk16) * (2 + d); 0 outside the limits */
long vpc_nm_impute_scratch(long B, int S, int d, int L, int s_chunk);
int vpc_nm_impute(const float* params, const float* x, const float* mask, const float* eps, unsigned long long seed,
                  unsigned long long offset, long row0, float* part, long part_floats, float* xm, float* lse, long B, int S,
                  int d, int L, int s_chunk, int regularised, void* stream);

/* ---- flow path: VAEFlow / REG_VAEFlow (csrc/vpc_flow.hip) -------------------------------------------------------
 * Reference: src/models/VAE.py:1860-1996 and :1999-2124, posterior Flow :1816-1854 (three PiecewiseLinearCDF layers,
 * tails "linear", tail_bound 1, context t.reshape(B, 10, 10), :1781-1813, spline :1680-1774).  Encoder
 * [x*m | m] (2d) -> hid -> hid ELU -> 100 and decoder 10 -> hid x4 ELU -> d Sigmoid run on vpc_linear_fwd / dgrad /
 * wgrad; these entry points add the per-step draws, the flow and the loss.  fp32; masks are float 0/1; the latent
 * dimension is fixed at VPC_FLOW_LATENT (the reference's hard-coded 10 x 10 reshape).  `R` = rows of the stacked
 * passes (R = B or 2 B), `B` = rows of one pass: the reference's torch.any(inside) (:1698) is taken per pass. */
#define VPC_FLOW_LATENT 10
#define VPC_FLOW_TRAIN 0
#define VPC_FLOW_EVAL 1

/* Per-step inputs in one launch (train.py:53-55 + VAE.py:1924-1931): xin[0:B] = [x * mask | mask] ([R][2d]) and, with
 * a second pass, xin[B:2B] = [x * mask_p | mask_p] where mask_p = mask_p_in, or (mask_p_in NULL, mask_p_out != NULL) a
 * fresh draw mask * (U < keep_prob) written to mask_p_out (the Philox counters of vpc_nm_prep's draw: element index / 4
 * + offset).  n_eps > 0: eps_out[0:n_eps] ~ N(0, 1) (counter offset_eps; Flow.forward's rsample, :1824-1827). */
int vpc_flow_prep(const float* x, const float* mask, const float* mask_p_in, float* mask_p_out, float* xin,
                  float* eps_out, long n_eps, long B, int d, float keep_prob, unsigned long long seed,
                  unsigned long long offset, unsigned long long offset_eps, void* stream);
/* z, z_log_prob [R][10] = Flow.forward with the draws eps [R][10] and the contexts t [R][ldt >= 100] (:1816-1831,
 * :1680-1774), the reference's quirks reproduced: context bins masked in place with the latent mask, outside inputs
 * zeroed and splined, the identity when no draw of the pass is inside [-1, 1]. */
int vpc_flow_fwd(const float* t, long ldt, const float* eps, float* z, float* z_log_prob, long R, long B, void* stream);
/* dt [R][lddt >= 100] = d / d t given d / d z = dz + dz2 and d / d z_log_prob (each may be NULL); the forward is
 * recomputed from (t, eps).  dt = 0 on masked bins and in a pass with no inside draw. */
int vpc_flow_bwd(const float* t, long ldt, const float* eps, const float* dz, const float* dz2, const float* dz_log_prob,
                 float* dt, long lddt, long R, long B, void* stream);
/* Loss of REG_VAEFlow (mask_p != NULL; :2075-2111) or VAEFlow (mask_p == NULL; :1950-1969) at `stage`
 * (VPC_FLOW_TRAIN / VPC_FLOW_EVAL, REG only; the evaluate stage reads no p-pass input) and, when g_x_mean_q != NULL,
 * gscale * its gradients w.r.t. x_mean ([B][ldg] per pass; gated != 0: w.r.t. the decoder_mean PRE-activation, already
 * through Sigmoid', so vpc_linear_dgrad / wgrad take y_gate = NULL), z and z_log_prob ([B][10] per pass; p-pass
 * gradients are zero in the evaluate stage).  x_mean_* [B][ldxm] = the decoder's Sigmoid outputs; x_logvar is the
 * constant -8 of :1946-1947.  out8 (device doubles) = loss (the unscaled sum; train_loss = loss / B), RE_q, RE_p, KL_q,
 * KL_p, KL_reg, NLL of x*mask*~mask_p, RE_q_imputed (NLL on ~mask).  loss_f32 / accum (optional): train_loss as a
 * float, and accum[0] += train_loss.  Two launches (per-row terms and gradients, fixed-order reduction of the
 * per-workgroup partials) through `scratch` (vpc_flow_loss_scratch bytes, 8-byte aligned). */
long vpc_flow_loss_scratch(long B);
int vpc_flow_loss(const float* x, const float* mask, const float* mask_p, const float* x_mean_q, const float* x_mean_p,
                  long ldxm, const float* z_q, const float* z_p, const float* z_log_prob_q, const float* z_log_prob_p,
                  float* g_x_mean_q, float* g_x_mean_p, long ldg, float* g_z_q, float* g_z_p, float* g_z_log_prob_q,
                  float* g_z_log_prob_p, void* scratch, long scratch_bytes, double* out8, float* loss_f32, float* accum,
                  long B, int d, int stage, float alpha, float beta, float gscale, int gated, void* stream);

/* ---- an ensemble of G flow models of ONE shape: the few-row step with a member axis ----------------------------------
 * Replaces the drivers' loops around train() (src/experiment_main/imputation.py:21-39: `for missing: for alpha:`) for the
 * runs vanilla_flow1..3 / reg_flow1..3 (Data/imputation_args.json:7-12): the G members step in the launches of ONE
 * stand-alone few-row step (FlowTrainer._step_small: 21 calls, 22 launches), whatever G.  Every entry is its stand-alone
 * entry with a member axis on the grid: workgroup (.., g) runs the stand-alone kernel's body on member g's arrays
 * (base + g * stride floats), so member g computes bit for bit what the stand-alone call on its arrays computes, whatever G
 * and wherever its workgroups run.  No atomics, no traffic between workgroups.
 * Members: G device-resident VpcFlowMember records (32 bytes, ordinary loads) - what may differ from member to member
 * besides the data.  Every entry checks its arguments before any launch and launches nothing on failure: VPC_ERR_ARG for a
 * NULL mandatory pointer, G outside 1 .. VPC_FLOW_MULTI_MAX_MEMBERS, a member stride below the member's slice (the
 * strides of x / mask may be 0: one batch read by every member) and what the stand-alone entry refuses; VPC_ERR_SHAPE
 * for what the stand-alone entry calls an unsupported shape and for a grid past the launch limits. */
#define VPC_FLOW_MULTI_MAX_MEMBERS 4096
#define VPC_ROWS_MULTI_MAX_MEMBERS 4096
typedef struct VpcFlowMember {
    unsigned long long seed; /* Philox seed of the member's mask_p and eps draws (train.py:102-104, VAE.py:1824-1827) */
    float alpha;             /* REG_VAEFlow loss weight (VAE.py:2086-2093) */
    float beta;              /* KL weight (VAE.py:1962, :2084) */
    float keep_prob;         /* 1 - p_missingness / 100 of the mask_p draw (train.py:102-104) */
    float lr;                /* Adam learning rate (train.py:21) */
    int reserved[2];         /* 0 */
} VpcFlowMember;

/* vpc_rows_fwd (nn.Linear + activation, VAE.py:1878-1900) for G members: grid (slabs, row blocks, G).  w / bias are member
 * 0's layer inside the stacked flat parameters, wb_stride the stack's row pitch; x / y member 0's activations.
 * order: 0 = member-major; 1 = all workgroups of a member on one XCD (grid (8 x workgroups, ceil(G / 8)); same bits), so a
 * member's weights are re-read through one L2.  The 16-byte or scalar build is chosen as vpc_rows_fwd chooses it on member
 * 0's operands; EVERY member stride must therefore be a multiple of 4 floats (VPC_ERR_ARG otherwise), and none may be 0. */
int vpc_rows_fwd_multi(const float* x, long ldx, long x_stride, const float* w, const float* bias, long wb_stride, float* y,
                       long ldy, long y_stride, int G, long M, int N, int K, int act, int act_split, int order, void* stream);
/* vpc_rows_bwd (autograd of the same layer) for G members: the 1-D grid of one member x G (blockIdx.y = member under order 0).
 * w, dw and db share wb_stride (the parameter and the gradient stack have one row pitch).  Strides of arrays that are
 * NULL are ignored; the stride rule and `order` as in vpc_rows_fwd_multi. */
int vpc_rows_bwd_multi(const float* dy, long lddy, long dy_stride, const float* y_gate, long ldyg, long yg_stride, int gate,
                       int gate_split, const float* w, const float* x, long ldx, long x_stride, const float* x_out, long ldxo,
                       long xo_stride, int act_prev, float* dx, long lddx, long dx_stride, float* dw, float* db, long wb_stride,
                       int G, long M, int N, int K, int accumulate, int order, void* stream);
/* vpc_flow_prep (train.py:53-55, :102-104 + VAE.py:1924-1931) for G members: member g's xin [R][2d] from its x / mask and,
 * with a second pass (R == 2 B; mask_p mandatory then, NULL otherwise), its mask_p [B][d].  draw != 0: mask_p and eps
 * [R][10] are drawn with seed_g and keep_prob_g at the counters of the stand-alone entry (offset, offset_eps); draw == 0:
 * mask_p is read and eps left alone. */
int vpc_flow_multi_prep(const float* x, long x_stride, const float* mask, long mask_stride, float* mask_p, long mask_p_stride,
                        float* xin, long xin_stride, float* eps, long eps_stride, const VpcFlowMember* members, int G, int draw,
                        long R, long B, int d, unsigned long long offset, unsigned long long offset_eps, void* stream);
/* vpc_flow_fwd / vpc_flow_bwd (Flow.forward, VAE.py:1816-1831, and its autograd) for G members.  stride10: floats between
 * two members' [R][10] arrays (eps, z, z_log_prob, dz, dz2, dz_log_prob).  torch.any(inside) (VAE.py:1698) is taken per
 * (member, pass): over member g's eps rows of that pass only. */
int vpc_flow_fwd_multi(const float* t, long ldt, long t_stride, const float* eps, float* z, float* z_log_prob, long stride10,
                       int G, long R, long B, void* stream);
int vpc_flow_bwd_multi(const float* t, long ldt, long t_stride, const float* eps, const float* dz, const float* dz2,
                       const float* dz_log_prob, long stride10, float* dt, long lddt, long dt_stride, int G, long R, long B,
                       void* stream);
/* vpc_flow_loss (VAE.py:1950-1969 / :2075-2111) for G members, both launches with blockIdx.y = member: alpha_g and beta_g
 * from the member table; out8 [G][8], loss_f32 [G], accum [G]; scratch of vpc_flow_loss_multi_scratch(G, B) bytes.  A
 * member's x_mean, z, z_log_prob and gradient arrays hold its q rows and then its p rows (the *_q / *_p pointers are member
 * 0's), x_mean_stride / g_stride / stride10 apart. */
long vpc_flow_loss_multi_scratch(int G, long B);
int vpc_flow_loss_multi(const float* x, long x_stride, const float* mask, long mask_stride, const float* mask_p,
                        long mask_p_stride, const float* x_mean_q, const float* x_mean_p, long ldxm, long x_mean_stride,
                        const float* z_q, const float* z_p, const float* z_log_prob_q, const float* z_log_prob_p,
                        float* g_x_mean_q, float* g_x_mean_p, long ldg, long g_stride, float* g_z_q, float* g_z_p,
                        float* g_z_log_prob_q, float* g_z_log_prob_p, long stride10, void* scratch, long scratch_bytes,
                        double* out8, float* loss_f32, float* accum, const VpcFlowMember* members, int G, long B, int d,
                        int stage, float gscale, int gated, void* stream);
/* vpc_adam_step (torch.optim.Adam, train.py:21, :116) on the rows of [G][row_stride] stacks in ONE launch: per element the
 * arithmetic of vpc_adam_step with lr_g; the host step count, betas and eps are shared. */
int vpc_adam_step_multi(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long row_stride, int n,
                        const VpcFlowMember* members, int G, float beta1, float beta2, float eps, long step, void* stream);

/* ---- batched evaluation of a flow model (csrc/vpc_floweval.hip) ----------------------------------------------------
 * Replaces the loops of eval_vae's flow branch (src/experiment_main/evaluate.py:189-200 inside :160-245: `for _ in range(M):
 * for data_sample, mask in loader:`): the rows of every batch of every Monte-Carlo pass stand behind each other (R stacked
 * rows), the layers run once over all of them (vpc_linear_fwd), and these entries do what is not row-independent, with a
 * table of batches ("tiles"): tile t = rows [tile_row0[t], tile_row0[t + 1]) of the stacked arrays, tile_row0[0] = 0, strictly
 * ascending, tile_row0[n_tiles] = R.  Every table is given twice: on the HOST (checked before anything is launched; sizes the
 * grids) and as a DEVICE copy of the same int64 values (what the kernels read, clamped to [0, R], so that a copy that differs
 * cannot take a kernel out of bounds).  fp32, no float atomics, every sum in a fixed order.  VPC_ERR_ARG: a NULL mandatory
 * pointer, n_tiles < 1, a host table that is not of that form, short or misaligned scratch, n_tiles > 65535
 * (vpc_flow_eval_tiles), R > 2^26. */
/* Flow.forward (VAE.py:1816-1831) on R stacked rows with torch.any(|eps| <= 1) (:1698) taken per tile: the rows of tile t are,
 * bit for bit, what vpc_flow_fwd(R = B = the tile's rows) writes for them.  One launch: a workgroup takes the predicate of
 * every tile that its 25.6 rows touch. */
int vpc_flow_fwd_tiles(const float* t, long ldt, const float* eps, float* z, float* z_log_prob, long R, const long* tile_row0,
                       const long* tile_row0_dev, long n_tiles, void* stream);
/* The evaluate-stage loss terms (VAEFlow.loss, VAE.py:1950-1969; REG_VAEFlow.loss with stage != 'train', :2099-2104: loss_q,
 * which reads nothing of the p pass) and the RMSE sums of evaluate.py:232-235, per tile.  stats (device doubles)
 * [n_tiles][8] = loss sum RE_q + beta KL_q, RE_q (NLL on mask), KL_q, RE_q_imputed (NLL on 1 - mask),
 * sum((x_mean - x)^2 (1 - mask)), sum(1 - mask), rows, 0.  Columns 0, 1, 3 of tile t equal, bit for bit, out8[0], out8[1],
 * out8[7] of vpc_flow_loss(mask_p = NULL, forward only, the same beta) on the tile's rows: one wave per row, four rows per
 * double partial, the partials of a tile summed as vpc_flow_loss sums them; columns 4 and 5 are summed in the same shape.
 * x, mask [R][d]; x_mean [R][ldxm >= d]; z, z_log_prob [R][10].  Two launches (grid (ceil(max tile rows / 4), n_tiles), then
 * one workgroup per tile) through `scratch` (vpc_flow_eval_tiles_scratch bytes, 8-byte aligned). */
long vpc_flow_eval_tiles_scratch(long max_tile_rows, long n_tiles);
int vpc_flow_eval_tiles(const float* x, const float* mask, const float* x_mean, long ldxm, const float* z,
                        const float* z_log_prob, long R, int d, const long* tile_row0, const long* tile_row0_dev, long n_tiles,
                        float beta, void* scratch, long scratch_bytes, double* stats, void* stream);
/* The estimator of evaluate.py:232-245 from the tile statistics: per tile rmse = sqrt(col4 / col5) (0 / 0 = NaN for a tile
 * with no unobserved entry, as the reference's division gives), elbo = col0 / rows, negll = col1 / rows, negll_imp =
 * col3 / rows; the mean over the tiles [pass_tile0[p], pass_tile0[p + 1]) of every pass, then the mean over the M passes,
 * both in table order (M > 256: thread j sums the passes j, j + 256, .., then the threads in order).  pass_tile0 [M + 1]:
 * pass_tile0[0] = 0, strictly ascending, pass_tile0[M] = n_tiles.  out4 (device doubles) = rmse, elbo, negll, negll_imp.
 * One workgroup. */
int vpc_flow_eval_finalize(const double* stats, long n_tiles, const long* pass_tile0, const long* pass_tile0_dev, long M,
                           double* out4, void* stream);

/* ---- config 5 reward of the flow models (csrc/vpc_flowreward.hip) ------------------------------------------------
 * Replaces the flow branch of active_learning_func's candidate loop (src/experiment_main/evaluate.py:416-422) and the
 * functions it calls: R_lindley_chain_ratio_version (:637-665), chaini_I_ratio_version (:669-684),
 * chaini_II_ratio_version (:688-708).  For every row n and candidate u < d-1 with mask[n][u] == 0
 *     R[n][u] = 1/M sum_m [ sum_l |lp_Ia - lp_Ib| - sum_l |lp_IIa - lp_IIb| ]       (-1e4 where mask[n][u] != 0)
 * where each lp is the z_log_prob [10] of one VAEFlow.encoder call (VAE.py:1924-1931) on the rows loc(u) =
 * {n : mask[n][u] == 0} with its own draw, in the call order Ia, Ib, IIa, IIb inside the m loop; the carry-over of the
 * imputed target between samples (:653-658) and the per-call torch.any(inside) (VAE.py:1698, over loc(u) x 10) are
 * reproduced.  x [n][d], mask [n][d] float 0/1, im [M][n][d]; We1 [hid][2d] .. be3 [100] = seq_encoder.{0,2,4};
 * eps = the draws as a dense [d-1][M][4][n][10] tensor (rows outside loc(u) ignored; 16-byte aligned) or NULL: then
 * they come from Philox(seed), the counter of a value being its index in that tensor.  R [n][d-1].
 * Candidates are processed `chunk` at a time through `scratch` (vpc_flow_reward_scratch floats, 16-byte aligned); R does
 * not depend on `chunk`.  d >= 2, 1 <= hid <= 512, M >= 1, chunk >= 1; anything else returns an error before any launch. */
int vpc_flow_reward_scratch(int n, int d, int hid, int M, int chunk, long* scratch_floats);
int vpc_flow_reward_matrix(const float* x, const float* mask, const float* im, const float* We1, const float* be1,
                           const float* We2, const float* be2, const float* We3, const float* be3, const float* eps,
                           unsigned long long seed, float* scratch, long scratch_floats, float* R, int n, int d, int hid,
                           int M, int chunk, void* stream);
/* eps [d-1][M][4][n][10] ~ N(0, 1): the draws vpc_flow_reward_matrix(eps = NULL, seed) uses (Flow.forward's rsample,
 * VAE.py:1824-1827, one per encoder call of evaluate.py:680-682, 704-706). */
int vpc_flow_reward_draws(float* eps, int n, int d, int M, unsigned long long seed, void* stream);

/* ---- annealed importance sampling with adaptive-step HMC (csrc/vpc_ais.hip) ----------------------------------------
 * Replaces the chain arithmetic of src/utils/AIS.py: the temperature loop of ais_trajectory (:178-217) with log_f_i
 * (:125-140), U / grad_U / normalized_kinetic (:187-204), hmc_trajectory (:237-262) and accept_reject (:265-304), for
 * the decoders that are the latent -> 50 -> 100 -> d sigmoid chain with a constant x_logvar.  B = nb * n_sample chains
 * in safe_repeat order (:28-29, 160): chain c belongs to row c % nb of x [nb][d].  The annealed density is
 *     log f(z, t) = -|z|^2 / 2 + t * sign * NLL(x; decoder(z)),   NLL = sum over all d columns of -log N(x; mean, var)
 * sign = +1: the reference as written (:125 passes neg_gaussian_log_likelihood as the log likelihood); sign = -1: the
 * corrected target p(z) p(x|z)^t.  The step-size adaptation constants (0.65, 1.02, 0.98, [1e-4, 0.5]) are :295-297's. */

/* 1 when vpc_ais_run covers the shape (d <= 128, L <= 15, 1 <= B < 2^30), else 0. */
int vpc_ais_applicable(long B, int d, int L);
/* Floats of the chain state of B chains: z [B][16] (columns >= L are 0) | epsilon [B] | accept_hist [B] | logw [B] |
 * nll_current [B] (NLL at the current z).  16-byte aligned. */
long vpc_ais_state_floats(long B);
/* The schedule pairs (schedule[j-1], schedule[j]) for j = j0 .. j0 + nsteps - 1 (1-based as :178's enumerate;
 * schedule = T device floats) in ONE persistent launch: a wave owns a 16-chain tile, the decoder image sits in LDS, the
 * chain state stays in registers.  init != 0: the state is initialised first (:163-174: epsilon = init_step_size,
 * accept_hist = logw = 0, z = z0), otherwise read from `state`; it is written back at the end, so a schedule may be
 * split over any number of calls with bit-equal results.  Draws: z0 [B][L], v [T-1][B][L] (:185), u [T-1][B] (:289) are
 * read where given; a NULL array is generated from Philox4x32-10 (seed; counter = chain, j, kind - independent of the
 * split and of the launch geometry; vpc_ais_draws writes the same values).  Backward mode (:173) passes the repeated
 * post_z as z0.  dec_img = the decoder image of vpc_pack_weights.  Returns 2 for d > 128 or L > 15. */
int vpc_ais_run(const float* x, const float* dec_img, const float* schedule, int T, int j0, int nsteps, int init,
                float* state, const float* z0, const float* v, const float* u, unsigned long long seed, float sign,
                int leapfrog_steps, float init_step_size, float grad_clip, float x_logvar, long B, long nb, int d, int L,
                void* stream);
/* The draws vpc_ais_run(seed) generates, as dense arrays (each may be NULL): z0 [B][L] ~ N(0, 1) (:171),
 * v [T-1][B][L] ~ N(0, 1) (:185), u [T-1][B] ~ U(0, 1) (:289). */
int vpc_ais_draws(float* z0, float* v, float* u, long B, int L, int T, unsigned long long seed, void* stream);

/* ---- the GEMM-backed AIS engine (csrc/vpc_aisg.hip) ------------------------------------------------------------------
 * The same chain (AIS.py:155-217, 237-304) for every decoder the reference's ais_trajectory can run, which needs only
 * model.decoder(z) -> (mean, logvar) (:125-140): the decoder is an MLP chain of vpc_linear_fwd / vpc_linear_dgrad layers,
 * HOST arrays of n_layers (<= 8) entries: w[i] [N[i]][K[i]], b[i] [N[i]], act[i] (the activation codes above), K[0] = L,
 * K[i+1] = N[i].  The last layer is either N = d (mean; the log-variance is the scalar x_logvar) or N = 2 d with
 * act = 2, last_split = d ([mean | logvar] with Sigmoid | Hardtanh(-10, 0): VAE.py:2359-2363, 2392-2396).
 * NLL = sum over the columns of -log N(x; mean, exp(logvar)) (utils.py:149-151), each term times mask[row][column] when
 * mask [nb][d] (float 0/1) is given.  grad U = z - t * sign * dNLL/dz clamped to +-grad_clip (:196); leapfrog :252-260;
 * accept / reject and the 1.02 / 0.98 adaptation with its clamp :285-297.
 * Same j0 / nsteps / init / draws contract as vpc_ais_run; draws come from the same counters (vpc_ais_draws returns
 * them; latent groups past 16 components use bits 24.. of the counter's high word, so T < 2^24).  Every launch of the
 * block of temperatures is enqueued on `stream`: (leapfrog_steps + 1) * (2 n_layers + 2) + 1 per temperature, + 1 per
 * call; nothing is allocated and nothing synchronises; fp32 GEMMs.  Results are bit-equal however the schedule is split.
 * workspace: vpc_aisg_workspace_floats(B, L, n_layers, N) floats, 16-byte aligned.  With r4(n) = n rounded up to a
 * multiple of 4 it starts with z [B][L] (r4(B L) floats) | epsilon | accept_hist | logw | nll_current (r4(B) each).
 * Returns 2 for obs_dim > 1024, a hidden width > 512, latent_dim > 64 or B >= 2^30. */
long vpc_aisg_workspace_floats(long B, int L, int n_layers, const int* N);
int vpc_aisg_run(const float* x, const float* mask, const float* const* w, const float* const* b, const int* K,
                 const int* N, const int* act, int n_layers, int last_split, float x_logvar, const float* schedule, int T,
                 int j0, int nsteps, int init, float* workspace, long workspace_floats, const float* z0, const float* v,
                 const float* u, unsigned long long seed, float sign, int leapfrog_steps, float init_step_size,
                 float grad_clip, long B, long nb, int d, int L, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPC_H */
