/*
 * fmc_hip.h -- C ABI of libfmc_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * denoising hot path of FMC (FudanCVL/SynFMC).
 *
 * This is the drop-in boundary.  The reference is pure Python and has
 * no FFI of its own; every entry point below replaces a chain of implicit PyTorch/cuDNN/cuBLAS
 * calls at the cited reference site (`path:line` relative to the reference root).  The
 * reference-side binding a maintainer would add is a ctypes stub: see INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless named `h_*`;
 *   - the caller owns every buffer; kernels never allocate, free or synchronise;
 *   - all work is enqueued on `stream` (a hipStream_t; NULL = the default stream);
 *   - every function returns 0 on success or a negative FMC_E_* code; `fmc_last_error()`
 *     returns a thread-local, human readable description of the last failure;
 *   - `dtype` selects the storage type of activations: FMC_BF16 (bf16 storage, fp32
 *     accumulate / statistics) or FMC_F32 (fp32 storage; the attention kernels then run the
 *     matrix products as split-bf16 x3 MFMA so that results agree with an fp32 reference to
 *     ~1e-5 -- this is the parity mode, not the fast mode);
 *   - activations are channels-last: an image batch is `[N, H*W, C]` with C contiguous.
 */
#ifndef FMC_HIP_H
#define FMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMC_VERSION 100 /* 0.1.0 */

enum { FMC_BF16 = 0, FMC_F32 = 1 };

enum {
    FMC_OK = 0,
    FMC_E_SHAPE = -1,  /* unsupported / inconsistent shape      -> Python ValueError          */
    FMC_E_DTYPE = -2,  /* unknown dtype code                    -> Python TypeError           */
    FMC_E_ALIGN = -3,  /* pointer or stride not 16-byte aligned -> Python ValueError          */
    FMC_E_LAUNCH = -4, /* hipLaunchKernel failed                -> Python RuntimeError        */
    FMC_E_NULL = -5    /* NULL where a pointer is required      -> Python ValueError          */
};

int fmc_version(void);
const char* fmc_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * GroupNorm (+ optional SiLU), channels-last.
 * Replaces nn.GroupNorm + SiLU in diffusers' ResnetBlock2D (norm1/norm2; ctor args at
 * fmc/models/unet_blocks.py:306-317), `conv_norm_out` + `conv_act` (fmc/models/unet.py:284-285,
 * 749-752), InflatedGroupNorm of the motion modules (fmc/models/resnet.py:27-37, no activation)
 * and the `norm` of Transformer2DModel (eps 1e-6).
 *   x, y        : [N, HW, C]  (dtype), y may alias x
 *   gamma, beta : [C] fp32
 *   stats       : [N, G, 2] fp32 out (mean, rstd) -- kept for the backward; must not be NULL
 *   workspace   : fp32 scratch of fmc_groupnorm_workspace_bytes(N, C, G) bytes
 *   act         : 0 = none, 1 = SiLU
 *   x2, C1      : two-source input, or NULL / 0.  With x2 the normalised tensor is the channel concat of x [N, HW, C1]
 *                 and x2 [N, HW, C - C1] (C1 % 8 == 0); y is the contiguous [N, HW, C].  The up blocks' `torch.cat([
 *                 hidden, skip], dim=1)` (unet_blocks.py:683,798) is then never materialised.
 * Requires C % 8 == 0 and C % G == 0.
 * ------------------------------------------------------------------------------------------- */
int64_t fmc_groupnorm_workspace_bytes(int N, int C, int G);
int fmc_groupnorm_silu_fwd(const void* x, void* y, const float* gamma, const float* beta, float* stats,
                           void* workspace, int N, int HW, int C, int G, float eps, int act, int dtype,
                           const void* x2, int C1, void* stream);
/* dX of the above (frozen gamma/beta; fmc_groupnorm_silu_bwd_params below also returns their gradients).
 *   dy, x, dx : [N, HW, C]; stats from the forward; act as in the forward. */
int fmc_groupnorm_silu_bwd(const void* dy, const void* x, void* dx, const float* gamma, const float* beta,
                           const float* stats, void* workspace, int N, int HW, int C, int G, int act,
                           int dtype, void* stream);

/* LayerNorm over the last dim of a token matrix [M, C] (eps 1e-5 everywhere on the path:
 * BasicTransformerBlock.norm1-3, TemporalTransformerBlock.norms / ff_norm,
 * fmc/models/motion_module.py:282-285).  Optional fused positional-encoding add for the temporal
 * blocks (`pos_encoder(norm(x))`, motion_module.py:355-356): if `pe` != NULL, token row r gets
 * pe[(r / pe_inner) % pe_frames] added AFTER the normalisation (rows are `[(b f), hw]` ordered:
 * pe_inner = hw, pe_frames = F).   gamma/beta/pe: fp32. */
int fmc_layernorm_fwd(const void* x, void* y, const float* gamma, const float* beta, const float* pe,
                      int64_t M, int C, float eps, int pe_inner, int pe_frames, int dtype, void* stream);
/* The same with the residual add in front: sum_out = x + addend (rounded to the storage type), y = LayerNorm(sum_out) (+ pe).  For
 * `h = attn(...) + h` followed by the next norm (diffusers BasicTransformerBlock, fmc/models/motion_module.py:282-300) where the
 * projection ran on the vendor-library arm and would leave the add to an elementwise launch.  C in {320, 640, 1280}. */
int fmc_layernorm_add_fwd(const void* x, const void* addend, void* sum_out, void* y, const float* gamma, const float* beta,
                          const float* pe, int64_t M, int C, float eps, int pe_inner, int pe_frames, int dtype, void* stream);

/* GEGLU gate of diffusers' FeedForward (`a * gelu_erf(g)` with a,g = chunk(proj(x), 2);
 * fmc/models/motion_module.py:284 and BasicTransformerBlock.ff):  x [M, 2*Cff] -> y [M, Cff]. */
int fmc_geglu_fwd(const void* x, void* y, int64_t M, int Cff, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spatial attention: softmax(Q K^T * scale) V per (batch, head), flash style (no S x S tensor).
 * Replaces head_to_batch_dim + baddbmm + softmax + bmm + batch_to_head_dim in
 * fmc/models/attention_processor.py:61-67 / 148-154 for `attn1` (self, S_kv = S_q) and `attn2`
 * (text cross attention, S_kv = 77).
 *   q : [B, Sq, H*D]  rows `q_row_stride` elements apart, batches `q_batch_stride` apart
 *   k, v : [Bkv, Skv, H*D] likewise; batch b of q reads kv batch  b / kv_batch_div
 *          (kv_batch_div = F lets all frames of a clip share one text K/V)
 *   o : [B, Sq, H*D] with its own strides
 *   lse : optional [B, H, Sq] fp32 (natural-log-sum-exp of the scaled scores), NULL to skip
 *   D must be a multiple of 8 and <= 160.  All strides in ELEMENTS, multiples of 8.
 * ------------------------------------------------------------------------------------------- */
int fmc_spatial_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H,
                         int Sq, int Skv, int D, int64_t q_batch_stride, int64_t q_row_stride,
                         int64_t kv_batch_stride, int64_t kv_row_stride, int64_t o_batch_stride,
                         int64_t o_row_stride, int kv_batch_div, float scale, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Temporal attention: for every pixel and head, softmax(Q K^T * scale) V over the F frames.
 * Replaces the same call chain for the motion-module / camera-encoder attention blocks
 * (fmc/models/attention_processor.py:271-281 and :61-67 reached from
 * fmc/models/motion_module.py:365-389).
 * Token (clip n, frame f, pixel p) lives at  base + n*clip_stride + f*frame_stride + p*pix_stride
 * (elements); the H*D channels of a token are contiguous.  The reference layout `(b h w) f c` is
 * clip_stride = HW*F*C, pix_stride = F*C, frame_stride = C; the native channels-last layout
 * `[(b f), hw, c]` is clip_stride = F*HW*C, frame_stride = HW*C, pix_stride = C -- no transposing
 * copy in either case.  q/k/v share one stride triple (they are slices of one fused QKV row),
 * o has its own.   1 <= F <= 32 (anything else is FMC_E_SHAPE);  D % 8 == 0, D <= 160;  (H*D) % 8 == 0.
 * A clip length that is not a multiple of 16 runs with a partial last 16-frame tile: only the F real frame
 * rows are read and written (frame F of clip n may be frame 0 of clip n + 1), so the launch moves the
 * algorithmic 4 * n_clips * n_pix * F * H * D elements.  The same holds for the three entry points below.
 * ------------------------------------------------------------------------------------------- */
int fmc_temporal_attn_fwd(const void* q, const void* k, const void* v, void* o, int n_clips, int n_pix,
                          int F, int H, int D, int64_t clip_stride, int64_t frame_stride,
                          int64_t pix_stride, int64_t o_clip_stride, int64_t o_frame_stride,
                          int64_t o_pix_stride, float scale, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pluecker-ray embedding.  Replaces `ray_condition` (fmc/data/dataset.py:930-972) + the permutes
 * of `to_plucker_embedding` (train_cam_obj_ctrl.py:80-91, :833), which run on the CPU every step.
 *   K   : [B*F, 4] fp32 (fx, fy, cx, cy)      c2w : [B*F, c2w_rows(3|4), 4] fp32
 *   layout 0: out [B, F, H, W, 6]   (what ray_condition returns)
 *   layout 1: out [B, 6, F, H, W]   (what the trainers feed the pose encoder)
 *   layout 2: out [B*F, H/8, W/8, 384] channels-last, PixelUnshuffle(8) already applied
 *             (channel = c*64 + dy*8 + dx; input of CameraPoseEncoder.encoder_conv_in,
 *              fmc/models/pose_adaptor.py:228-232)
 *   out dtype: FMC_F32 or FMC_BF16.
 * ------------------------------------------------------------------------------------------- */
int fmc_plucker_fwd(const float* K, const float* c2w, void* out, int B, int F, int H, int W, int c2w_rows,
                    int layout, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * OMC rasteriser.  Replaces the Python loops of get_traj_features_v2 (fmc/util.py:158-201).
 *   poses : [BF, n_obj, 12] fp32      masks : [BF, n_obj, H, W] fp32 (Gaussian circle masks)
 *   layout 0: feat [BF, 13, H, W], mask_out [BF, 1, H, W]           (the Adapter's reference inputs)
 *   layout 2: feat [BF, H/8, W/8, 832] channels-last + PixelUnshuffle(8); mask_out [BF, H, W]
 *   Per pixel the LAST object with mask > 0 wins; feat = (pose*mask, mask) * mask.
 * ------------------------------------------------------------------------------------------- */
int fmc_omc_rasterize_fwd(const float* poses, const float* masks, void* feat, float* mask_out, int BF,
                          int n_obj, int H, int W, int layout, int dtype, void* stream);

/* Gaussian circle masks: the analytic part of the reference's sphere-mask synthesis (fmc/data/dataset.py:5365-5380;
 * cv2.minEnclosingCircle stays on the host and supplies the circles).  circles [N,3] fp32 = (cx, cy, radius) in
 * pixels, radius > 0; out [N,H,W] fp32 = [(x-int(cx))^2 + (y-int(cy))^2 <= int(r)^2] * g / max(g),
 * g = exp(-0.5 (d / (r/2))^2) with d the distance to the float centre.  Feeds fmc_omc_rasterize_fwd. */
int fmc_gaussian_circle_mask_fwd(const float* circles, float* out, int N, int H, int W, void* stream);

/* y[n,i,j,:] = x[n,i,j,:] * mask_in[n, si(i), sj(j)] with PyTorch's nearest rule
 * si(i) = min(floor(i * (float)Hin/h), Hin-1); also emits the resampled mask for the next level
 * (the reference cascades: fmc/adapter.py:175-177).  Used for the backward too (dX = mask * dY).
 *   x, y : [N, h*w, C] (dtype)   mask_in : [N, Hin, Win] fp32   mask_out : [N, h, w] fp32 or NULL */
int fmc_mask_modulate_fwd(const void* x, const float* mask_in, void* y, float* mask_out, int N, int h, int w,
                          int C, int Hin, int Win, int dtype, void* stream);

/* OMC injection `hidden + traj_features[idx]` (fmc/modified_modules.py:115-117,172-174) including
 * the classifier-free-guidance zero half (pipeline_animation_cm_om.py:671-676): the first
 * `skip_elems` elements of h get nothing added (just copied when out != h).
 *   h, out : [n_elems] (dtype), out may alias h;   t : [n_elems - skip_elems] (dtype) */
int fmc_feature_add_fwd(const void* h, const void* t, void* out, int64_t n_elems, int64_t skip_elems,
                        int dtype, void* stream);

/* CFG combine + DDIM (eta = 0) update, fused (pipeline_animation_cm_om.py:711-720; diffusers
 * DDIMScheduler.step):  eps = eps_u + g (eps_c - eps_u);  x0 = (x - sqrt(1-a_t) eps)/sqrt(a_t);
 * x' = sqrt(a_prev) x0 + sqrt(1-a_prev) eps.   eps_uc: [2, n] (dtype) (uncond, cond), or [1, n]
 * when guidance <= 1 (then pass has_uncond = 0).   x, x_out: [n] fp32 latents. */
int fmc_cfg_ddim_step(const void* eps_uc, const float* x, float* x_out, int64_t n, int has_uncond,
                      float guidance, float alpha_t, float alpha_prev, int dtype, void* stream);

/* CFG combine + one step of any sampler whose update is linear in (x, eps, history, noise), fused, plus the next step's model
 * input (pipeline_animation_cm_om.py:696-720 with the schedulers the reference's pipelines are typed for: DDIM with eta /
 * clipping / v-prediction, Euler, Euler-ancestral, DPM-Solver++ multistep).  Per element i < n, fp32 arithmetic:
 *     e  = has_uncond ? eu + g (ec - eu) : e0
 *     m  = m_x x + m_e e ;  if (m_clamp > 0) m = clamp(m, -m_clamp, +m_clamp)
 *     x' = c_x x + c_e e + c_m m + sum_{j < n_hist} c_h[j] hist[j] + (noise ? c_n noise : 0)
 *     x_out[i] = x' ;  m_out[i] = m ;  x_in[r][i] = (in_dtype)(in_scale x'),  r < in_reps
 *   eps_uc : [2, n] (dtype) (uncond, cond) with has_uncond, else [1, n];   noise : [n] (dtype) or NULL
 *   x, x_out : [n] fp32, x_out may alias x;   hist0..2 : [n] fp32, the first n_hist (0..3) are read
 *   m_out : [n] fp32 or NULL, may alias any hist[j];   x_in : [in_reps, n] (in_dtype), in_reps 0..2, aliases nothing
 * Pointers need the alignment of their element only: a stream that is not 16-byte aligned where x is (the conditional half
 * of a bf16 eps_uc at odd n) moves element by element.  fmc_sampler_step_elems_per_trip(): elements one trip of the
 * grid-stride loop covers once the grid is at its cap. */
typedef struct fmc_sampler_coef {
    float g;                 /* guidance scale */
    float m_x, m_e, m_clamp; /* the converted model output m (x0 prediction), and its clamp (<= 0: none) */
    float c_x, c_e, c_m, c_n;
    float c_h[3];
    float in_scale;
} fmc_sampler_coef;
int64_t fmc_sampler_step_elems_per_trip(void);
int fmc_sampler_step(const void* eps_uc, const float* x, const void* noise, const float* hist0, const float* hist1,
                     const float* hist2, float* x_out, float* m_out, void* x_in, int64_t n, int has_uncond, int n_hist,
                     int in_reps, fmc_sampler_coef coef, int dtype, int in_dtype, void* stream);

/* Sliding windows ("multidiff", pipeline_animation_cm_om.py:687-720): the average of the windows' guided predictions and the step
 * of fmc_sampler_step, one pass over the full latents x [BC, Ftot, hw] fp32, Ftot = (W - 1) stride + F.  Window w covers frames
 * [w stride, w stride + F); the windows that cover frame f are w_lo = max(0, ceil((f - F + 1) / stride)) .. w_hi = min(W - 1,
 * floor(f / stride)), cnt = w_hi - w_lo + 1 of them.  Per element (bc, f, s), fp32:
 *     e_w = has_uncond ? eu_w + g (ec_w - eu_w) : e0_w        at window w's own frame f - w stride
 *     e   = (sum over w = w_lo .. w_hi, ascending, of e_w) / cnt
 *     m, x' as in fmc_sampler_step from (x, e, hist, noise);   x_out = x', m_out = m
 *     x_in[r][w][bc][f - w stride][s] = (in_dtype)(in_scale x')   for every covering window w and r < in_reps
 *   eps, x_in : one buffer each; element (r, w, bc, f_local, s) sits at base + r stride_r + w stride_w + (bc F + f_local) hw + s
 *               (strides in elements; r = 0 unconditional, 1 conditional for eps with has_uncond, else only r = 0 is read)
 *   noise (dtype), hist0..2, m_out (fp32) : [BC, Ftot, hw] like x;  x_out may alias x, m_out any hist[j]; x_in aliases nothing
 * Refused (FMC_E_SHAPE): stride < 1 or > F, W < 1, F < 1, in_reps > 2, n_hist > 3, 2^31 or more rows or work items (element
 * offsets are 64-bit).  Pointers need the alignment of their element only.  Windows that do not overlap (stride == F, or
 * W = 1) are fmc_sampler_step on every contiguous (bc, window) block of F hw elements: its kernel is launched per block (W = 1: once
 * on all BC F hw elements), and gives each block the plain step's bits. */
int fmc_window_step(const void* eps, int64_t eps_stride_r, int64_t eps_stride_w, const float* x, const void* noise,
                    const float* hist0, const float* hist1, const float* hist2, float* x_out, float* m_out, void* x_in,
                    int64_t in_stride_r, int64_t in_stride_w, int BC, int F, int stride, int W, int hw, int has_uncond,
                    int n_hist, int in_reps, fmc_sampler_coef coef, int dtype, int in_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * bf16 MFMA GEMM with fused epilogue:  out = alpha * (x @ w^T + bias) + residual      (epilogue 0)
 *                                      out = (x @ wa^T + ba) * gelu_erf(x @ wg^T + bg)  (epilogue 1, GEGLU)
 * Replaces nn.Linear of diffusers' Attention / FeedForward / Transformer2D 1x1 proj (call sites
 * fmc/models/attention_processor.py:50-69,255-283, fmc/models/motion_module.py:219,228,284) together with the
 * `+ hidden_states` residual that follows (motion_module.py:289-297) and the Camera-Adapter axpy
 * `qkv_merge(h + pose) * scale + h` (attention_processor.py:257).
 *   x [M, K] rows `ldx` apart, w [N, K] contiguous, bias [N] or NULL, residual [M, N] rows `ldres` apart or NULL,
 *   out [M, N] (epilogue 0) or [M, N/2] (epilogue 1), rows `ldo` apart.  All bf16, fp32 accumulate.
 *   epilogue 1 expects w / bias pre-interleaved per 64 rows: rows [64t, 64t+32) = value rows [32t, 32t+32) of the
 *   GEGLU projection, rows [64t+32, 64t+64) = the matching gate rows.
 *   Requires K % 64 == 0, N % 8 == 0 (N % 64 == 0 for epilogue 1), strides % 8 == 0.
 *   x2 != NULL: two-source A operand -- columns [0, k_split) of every row come from x, [k_split, K) from x2 (rows
 *   `ldx2` apart, k_split % 64 == 0): the 1x1 shortcut conv of an up-block ResNet reads (hidden, skip) without a concat.
 *   residual2 != NULL (needs residual; same row stride; epilogue 0): a second tensor added like residual.  The Camera
 *   Adapter's `qkv_merge(h + pose) * s + h` is linear in pose, and pose is constant over the denoising steps of a clip:
 *   with residual2 = s * (pose @ w^T + bias) computed once per clip the per-step call is alpha = s, no bias,
 *   residual = h, and the `h + pose` pass of attention_processor.py:257 disappears.
 *   tile: workgroup tile geometry, 0 = pick by shape, 1 = 128x128 (4 waves), 2 = 256x128 (8), 3 = 256x256 (16) with
 *   64-deep k-tiles in a 2-stage LDS ring; 4..6 = the same three with 32-deep k-tiles (half the LDS, twice the
 *   workgroups per CU); 7 = 256x128, 64-deep, 3 stages; 8 / 9 / 10 = 256x256 / 128x128 / 256x128, 32-deep, 4 stages
 *   (deeper rings keep more bytes in flight per CU); 11 = 128x320 (10 waves; spans N = 320 / 640 / 960 without padded
 *   columns); 12 = 128x320, 32-deep, 4 stages; 13 / 14 = the 8-phase 256x256 kernel (8 waves of 128x64, the two wave rows
 *   one barrier apart so each SIMD always has one wave on the matrix pipe and one loading; operands by half-tile
 *   `buffer_load ... lds` with a counted vmcnt, 4 / 5 half-tiles ahead; falls back to 3 for a two-source A operand or
 *   operands beyond 2 GiB); 15 = the persistent kernel of the K = 320 token projections (epilogue 0, N % 320 == 0, M % 64 == 0, one
 *   residual at most: 5 waves keep the weights of a 320-column block in registers for the life of the workgroup, 64-row A tiles
 *   arrive by LDS-DMA two tiles ahead, the residual rows are DMA'd into the output staging tile; the bias enters the accumulator
 *   first, so it agrees with the other arms to the last bit or two, not bit for bit; anything else falls back to 5);
 *   16 = 160 x 320 tiles (8 waves of 80 x 80 on the 16x16x32 MFMA, 32-deep sub-tiles in a 5-buffer LDS-DMA ring, one phase per sub-tile;
 *   N % 320 == 0, otherwise falls back to 13; token projections with more tiles than CUs and M % 160 == 0 run its persistent form, in which
 *   the next tile's operands stream in under the epilogue; GEGLU wants weight rows ordered [8 value | 8 gate] per 16);
 *   18 = tile 16 on a weight the caller PRE-PACKED tile-major in the kernel's own sub-tile order -- projections `[N / 320][K / 32][320][32]`,
 *   3x3 filters `[Cout / 320][Cin / 64][9 taps][2][320][32]` (sub-tile = (64-channel chunk, tap, 32-channel half)): every W piece of a sub-tile is
 *   one contiguous KiB; linear LDS-DMA requests move 30-50 % more bytes per CU than 16 rows x 64 B (tools/ubench/dma_mfma); bit-identical
 *   results, -1 .. -5 % per launch.  No fall-back exists for such a weight: N % 320 != 0, a two-source operand or stream-K are FMC_E_SHAPE.  The
 *   `w_tilemajor` flag of the tile-16-only entry points below (fmc_*_gn, fmc_linear_bf16_ln / _lnc / _ffblk) says the same about their weight.
 *   17 = the persistent form on 256 x 320 tiles (5 operand requests per 40 MFMAs and wave instead of 4 per 25), GEGLU epilogue only,
 *   M % 256 == 0 and more tiles than CUs -- anything else falls back to 16; same weight row order and bit-identical results.
 *   19 / 20 = 64 x 128 tiles of the ring kernel for small M (a wave = 32 x 64; 64-deep k-tiles in a 3-stage ring / 32-deep in a 4-stage ring: 2 / 3 workgroups per CU),
 *   21 / 22 = 128 x 128 / 64 x 256 on 8 such waves (two workgroups = 16 waves per CU);
 *   fmc_linear_bf16 without GEGLU only, bit-identical to tiles 1 / 4; split-K, stream-K, two residuals and fp32 storage fall back to tile 1.
 *   Every arm computes the same function -- bit for bit among the plain-grid arms of one k-tile depth
 *   (the 32-deep arms, split-K and stream-K add the same products in another order) -- so callers may time them and keep
 *   the fastest.
 *   split_k > 1 (epilogue 0 only): the k-tiles of every output tile are dealt to split_k workgroups that write fp32
 *   partial sums to `workspace` (>= split_k * M * N * 4 bytes, 16-byte aligned, caller-owned scratch); a second kernel
 *   sums them in a fixed order and applies the epilogue.  For M*N too small to fill 256 CUs (the 5x8 level).
 *   split_k == -3 / split_k <= -16 (arms 13 / 14 only; other arms treat it as -1): the K-LOCKSTEP split.  Every tile's reduction is cut into
 *   S chunks (S = -split_k - 16, or chosen by a cost model for -3); unit (chunk, tile) u runs on workgroup (u mod CUs) of a persistent pass in
 *   such an order that the CUs of one XCD work on the same k-chunk of the same filter column block at the same time (the weight leaves the
 *   Infinity Cache once per XCD and round, not once per tile: 775 -> ~90 MB per launch on the 10x16-level convolutions); fp32 partials in
 *   accumulator layout, one slot per unit (workspace >= 4096 + tiles * S * 256 KiB), summed in chunk order by a bandwidth-shaped finishing
 *   kernel that applies the plain epilogue (GEGLU: by the 8-phase kernel's own finishing launch).  Deterministic; same workspace as -1.
 *   split_k == -2 (arms 13 / 14 only; other arms treat it as -1): the tiles of the whole rounds (tiles / CUs * CUs of them) run on the
 *   plain grid and only the last partial round goes through the two stream-K launches below -- same workspace, same results as -1.
 *   split_k == -1: stream-K.  (On the 8-phase arms 13 / 14: TWO launches -- a persistent pass, one workgroup per CU, every
 *   segment's fp32 accumulators into a workspace slot in accumulator layout, then one workgroup per output tile that sums
 *   the slots covering its tile and runs the epilogue; workspace >= 4096 + CUs * (ceil(tiles / CUs) + 2) * 256 KiB, no
 *   flags.  What follows describes the other arms.)  One persistent workgroup per CU slot; the (tile, k-tile) iteration space is cut into equal
 *   contiguous ranges so every CU does the same number of k-tiles whatever tiles / CUs is; a tile cut by a range
 *   boundary is finished by the workgroup holding its first k-tiles, the others hand over fp32 partials through the
 *   workspace (sc1 accesses + flags, no fences; deterministic summation order).  `workspace` = [4096 bytes of flags,
 *   ZERO on entry and handed back zero | >= workgroups * tile_rows * tile_cols * 4 bytes]; too small a problem or
 *   workspace silently runs the plain grid.  Both epilogues.
 * ------------------------------------------------------------------------------------------- */
int fmc_linear_bf16(const void* x, const void* w, const void* bias, const void* residual, void* out, int64_t M, int N,
                    int K, int64_t ldx, int64_t ldres, int64_t ldo, float alpha, int epilogue, int tile, int split_k,
                    void* workspace, int64_t workspace_bytes, const void* x2, int64_t ldx2, int k_split,
                    const void* residual2, void* stream);

/* Implicit-GEMM 3x3 convolution (stride 1, pad 1) on channels-last bf16 images with the ResNet-block epilogue:
 *   out[i,y,x,:] = conv(x)[i,y,x,:] + bias + temb[i,:] + residual[i,y,x,:]
 * Replaces conv1 / conv2 of diffusers' ResnetBlock2D (ctor args fmc/models/unet_blocks.py:306-317), including
 * `+ time_emb_proj(silu(temb))[:, :, None, None]` and the `input_tensor + hidden_states` residual, and the conv of
 * Upsample2D (unet_blocks.py:625).
 *   x [n_img, H, W, Cin], w [Cout, 3, 3, Cin] (= the filter in torch.channels_last memory format),
 *   bias [Cout] | NULL, residual / out [n_img, H, W, Cout].  Cin % 64 == 0, Cout % 8 == 0.
 *   temb | NULL: image i adds row (i / temb_img_div) of temb, rows `temb_row_stride` elements apart -- [n_img, Cout]
 *   contiguous is (Cout, 1); the U-Net passes a column slice of ONE projection of all 22 ResNet blocks' time embeddings,
 *   [clips, sum Cout], with temb_img_div = frames, so the reference's per-frame repeat never materialises.
 *   upsample2x != 0: x is [n_img, H/2, W/2, Cin] and the convolution reads it through a nearest-neighbour 2x upsample
 *   (diffusers Upsample2D, unet_blocks.py:625: `F.interpolate(scale_factor=2)` then conv) -- the 4x larger tensor is
 *   never written; H, W stay the OUTPUT size.  upsample2x == 2: stride-2 convolution (diffusers Downsample2D,
 *   unet_blocks.py:350: 3x3, stride 2, pad 1): x is [n_img, 2H, 2W, Cin], H, W the OUTPUT size.
 *   tile / split_k / workspace: as for fmc_linear_bf16 (M = n_img*H*W, N = Cout, K = 9*Cin). */
int fmc_conv3x3_bf16(const void* x, const void* w, const void* bias, const void* temb, const void* residual, void* out,
                     int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride, int temb_img_div,
                     int upsample2x, int tile, int split_k, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GroupNorm statistics out of the producing GEMM / conv epilogue (reference sites: the GroupNorms of diffusers'
 * ResnetBlock2D / Transformer2DModel and of the motion module, fmc/models/unet_blocks.py:306-317, fmc/models/motion_module.py:177).
 * fmc_linear_bf16_gn / fmc_conv3x3_bf16_gn = fmc_linear_bf16 (epilogue 0) / fmc_conv3x3_bf16 on tile 16 (160 x 320 tiles; N resp. Cout % 320
 *   == 0, pixels per image gn_hw resp. H W % 160 == 0, M % gn_hw == 0) that ALSO write, per (image, 160-row tile of the image, group of
 *   N / 32 channels), the pair (sum, sum of squares) of the rounded bf16 outputs: gn_partials [M / gn_hw][gn_hw / 160][32][2] fp32.
 * fmc_groupnorm_apply_fwd = the second pass of fmc_groupnorm_silu_fwd alone: combines `partials [N][part_splits][G][2]` (fp64, fixed
 *   order), writes mean / rstd to stats and y = act(GroupNorm(x)).  The first pass (one more read of x) is not launched.
 * ------------------------------------------------------------------------------------------- */
int fmc_linear_bf16_gn(const void* x, const void* w, const void* bias, const void* residual, void* out, int64_t M, int N, int K,
                       int64_t ldx, int64_t ldres, int64_t ldo, float alpha, const void* residual2, float* gn_partials, int gn_hw,
                       int w_tilemajor, void* stream);
/* fmc_linear_bf16_ln = fmc_linear_bf16 (epilogue 0, tile 16, persistent form) for N == 320 that ALSO writes the CONSUMER's LayerNorm of the
 *   rows it produces (diffusers BasicTransformerBlock norm1 / norm2 / norm3 behind proj_in / attn1 / attn2, and the motion module's norms
 *   behind proj_in / the attention blocks: fmc/models/motion_module.py:282-288,355): a 160 x 320 tile holds whole rows, so
 *   ln_out[m, :] = (out[m, :] - mean) * rstd * ln_gamma + ln_beta (+ ln_pe[(m / ln_pe_inner) % ln_pe_frames, :]) is computed from the
 *   bf16-rounded rows in the staging tile (two-pass statistics, as fmc_layernorm_fwd) and out is never read again by a LayerNorm launch.
 *   Needs bf16, N == 320, M % 160 == 0, M / 160 > CUs, ln_pe_inner % 160 == 0 (a tile lies in one frame); ln_out contiguous [M, 320];
 *   gamma / beta / pe fp32.  Anything else is FMC_E_SHAPE (callers fall back to fmc_linear_bf16 + fmc_layernorm_fwd). */
int fmc_linear_bf16_ln(const void* x, const void* w, const void* bias, const void* residual, void* out, int64_t M, int N, int K,
                       int64_t ldx, int64_t ldres, int64_t ldo, float alpha, const void* residual2, void* ln_out, const float* ln_gamma,
                       const float* ln_beta, float ln_eps, const float* ln_pe, int ln_pe_inner, int ln_pe_frames, float* ln_stats, int w_tilemajor,
                       void* stream);
/* ... or, with ln_out == NULL and ln_stats != NULL, only the rows' statistics: ln_stats[M][2] = (mean, rstd) fp32 -- for a consumer that is a
 * GEMM and applies the LayerNorm itself:
 * fmc_linear_bf16_lnc = LayerNorm(x) @ w^T + b computed WITHOUT materialising LayerNorm(x): with w_gamma = w diag(gamma) (bf16),
 *   ln_c[n] = sum_k w_gamma[n, k] and ln_bias = w beta + b (fp32 [N]),   out[m, n] = rstd[m] (x[m, :] . w_gamma[n, :] - mean[m] ln_c[n]) + ln_bias[n]
 *   in the epilogue of tile 16's persistent form (epilogue 0, or 1 = GEGLU on [8 value | 8 gate]-ordered rows, ln_c / ln_bias in the same
 *   order); the products are exact in fp32 (bf16 x bf16), so the only new rounding is that of w gamma to bf16, in place of LayerNorm(x) to
 *   bf16.  Call sites: attn1 / attn2.to_q / the GEGLU projection behind norm1 / norm2 / norm3 of diffusers' BasicTransformerBlock and behind
 *   the motion module's ff_norm (fmc/models/motion_module.py:295-299).  Needs bf16, N % 320 == 0, M % 160 == 0, more 160 x 320 tiles than CUs. */
int fmc_linear_bf16_lnc(const void* x, const void* w_gamma, void* out, int64_t M, int N, int K, int64_t ldx, int64_t ldo, int epilogue,
                        const float* ln_stats, const float* ln_c, const float* ln_bias, int w_tilemajor, void* stream);
/* The feed-forward's intermediate in TILE-MAJOR order (diffusers FeedForward: GEGLU projection -> Linear, fmc call sites as for
 * fmc_linear_bf16): `[M / 160][C / 32][160 rows][32]` instead of `[M][C]`.  The GEGLU projection (epilogue 1, out_blocked = 1) writes its
 * gated 160 x 160 tile as five contiguous 10-KiB blocks, and the second GEMM (epilogue 0, x_blocked = 1) requests each 32-deep A sub-tile as
 * ONE contiguous block: linear 1-KiB LDS-DMA requests and whole DRAM pages instead of 160 row segments of 64 bytes.  The tensor is private to
 * the pair; results are bit-identical to the row-major path.  Tile 16's persistent form only (M % 160 == 0, N % 320 == 0, more tiles than CUs);
 * ln_stats / ln_c / ln_bias != NULL: the GEGLU projection also applies its input's LayerNorm (fmc_linear_bf16_lnc; bias must be NULL then). */
int fmc_linear_bf16_ffblk(const void* x, const void* w, const void* bias, const void* residual, void* out, int64_t M, int N, int K,
                          int64_t ldres, float alpha, int epilogue, int x_blocked, int out_blocked, const float* ln_stats, const float* ln_c,
                          const float* ln_bias, int w_tilemajor, void* stream);
/* The GroupNorm in front of a transformer's proj_in folded INTO the projection (diffusers Transformer2DModel.norm -> proj_in, fmc/models/unet_blocks.py:323-333;
 * TemporalTransformer3DModel.norm -> proj_in, fmc/models/motion_module.py:124-129: no activation between the two):
 *   proj(GN(x))[m, :] = W'_img x[m, :] + bias'_img,   W'_img = W diag(rstd[img, g(c)] gamma[c]),   bias'_img = bias + W beta - W'_img mean[img, g(.)]
 * fmc_groupnorm_fold_linear: partials [n_img, part_splits, G, 2] (sum, sum of squares per image, split and group, as fmc_groupnorm_apply_fwd takes them:
 *   the producer's epilogue wrote them) -> w_out bf16 [n_img][N][C] (each image's matrix tile-major [N / 320][C / 32][320][32] if w_tilemajor) and
 *   bias_out fp32 [n_img][N], computed from the ROUNDED W'_img so that the mean term cancels against W'_img x exactly.
 * fmc_linear_bf16_imgw: out[m, :] = w_img[m / img_rows] x[m, :] + bias_img[m / img_rows] on tile 16's persistent form (M % 160 == 0, img_rows % 160 == 0,
 *   N % 320 == 0, at least as many tiles as CUs); ln_stats != NULL (N == 320): also the rows' LayerNorm (mean, rstd) -> ln_stats[M][2], as fmc_linear_bf16_ln.
 * The normalised tensor is neither written nor read: one HBM pass over x less per transformer. */
int fmc_groupnorm_fold_linear(const float* partials, int part_splits, const float* gamma, const float* beta, const void* w, const void* bias,
                              void* w_out, float* bias_out, int n_img, int HW, int C, int G, int N, float eps, int w_tilemajor, void* stream);
int fmc_linear_bf16_imgw(const void* x, const void* w_img, const float* bias_img, void* out, int64_t M, int N, int K, int64_t ldx, int64_t ldo,
                         int img_rows, float* ln_stats, float ln_eps, int w_tilemajor, void* stream);
/* The feed-forward's output projection and the transformer's proj_out as ONE product (diffusers BasicTransformerBlock `ff(norm3(h)) + h` followed by
 * Transformer2DModel.proj_out + residual, fmc/models/unet_blocks.py:323-333; the motion module's `ff(ff_norm(h)) + h` followed by
 * TemporalTransformer3DModel.proj_out + residual, fmc/models/motion_module.py:130-134,295-299):
 *   proj_out(ff2(g) + b2 + h) + bp + x  =  [g | h] [Wp W2 | Wp]^T + (Wp b2 + bp) + x
 * x_blocked = the gated intermediate g, tile-major [M / 160][k_split / 32][160][32] (fmc_geglu*_ln_bf16 / fmc_geglu_pipe_ln_bf16 with out_blocked);
 * x2 = h, row-major [M, K - k_split] with rows ldx2 apart; w = the folded weight [N, K] (the caller folds it once per weight version, in fp32, and
 * rounds once), tile-major if w_tilemajor; gn_partials (may be NULL) as fmc_linear_bf16_gn.  One launch and two HBM passes less than the pair; the
 * block's output before proj_out is never rounded to bf16.  Tile 16's persistent form only: M % 160 == 0, N % 320 == 0, at least as many tiles as CUs,
 * k_split % 64 == 0. */
int fmc_linear_bf16_fftail(const void* x_blocked, const void* x2, const void* w, const void* bias, const void* residual, void* out, int64_t M,
                           int N, int K, int k_split, int64_t ldx2, int64_t ldres, float* gn_partials, int gn_hw, int w_tilemajor, void* stream);
/* The two consumers of the tile-major intermediate at any row count (gemm160p_kernel<..., PARTIAL>): x_blocked = ceil(M / 160) WHOLE tiles
 * [K' / 32][160][32] as fmc_geglu_pipe_ln_partial_bf16 leaves them (pad rows of the last tile: anything, NaN included -- they reach no valid row);
 * out / residual / x2 are row-major with M rows.  fmc_linear_bf16_ffblk_partial: out = alpha (x W^T + bias) + residual (the x_blocked form of
 * fmc_linear_bf16_ffblk, plain epilogue); fmc_linear_bf16_fftail_partial: fmc_linear_bf16_fftail, gn_partials must be NULL and gn_hw 0.  N % 320 == 0,
 * ceil(M / 160) * (N / 320) >= CUs, K (and k_split) % 64 == 0.  Valid rows are bit-identical to the whole-tile entry points on padded tokens. */
int fmc_linear_bf16_ffblk_partial(const void* x_blocked, const void* w, const void* bias, const void* residual, void* out, int64_t M, int N, int K,
                                  int64_t ldres, float alpha, int w_tilemajor, void* stream);
int fmc_linear_bf16_fftail_partial(const void* x_blocked, const void* x2, const void* w, const void* bias, const void* residual, void* out, int64_t M,
                                   int N, int K, int k_split, int64_t ldx2, int64_t ldres, float* gn_partials, int gn_hw, int w_tilemajor, void* stream);
int fmc_conv3x3_bf16_gn(const void* x, const void* w, const void* bias, const void* temb, const void* residual, void* out, int n_img,
                        int H, int W, int Cin, int Cout, int64_t temb_row_stride, int temb_img_div, int upsample2x,
                        float* gn_partials, int w_tilemajor, void* stream);
int fmc_groupnorm_apply_fwd(const void* x, void* y, const float* gamma, const float* beta, float* stats, const float* partials,
                            int part_splits, int N, int HW, int C, int G, float eps, int act, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 3x3 convolution with the input halo tile resident in LDS and GroupNorm + SiLU applied while it is staged (SURVEY.md section 8 f1;
 * csrc/conv_halo.hip).  Replaces `conv(nonlinearity(norm(x)))` of diffusers' ResnetBlock2D (ctor args fmc/models/unet_blocks.py:306-317:
 * norm1 -> SiLU -> conv1 (+ time_emb_proj) and norm2 -> SiLU -> conv2 (+ input_tensor)), `InflatedConv3d` / `InflatedGroupNorm`
 * (fmc/models/resnet.py:16-37) and Upsample2D's conv (unet_blocks.py:625) -- the normalised tensor is never written.
 *   x [n_img, Hs, Ws, Cin1] (+ x2 [n_img, Hs, Ws, Cin - Cin1] | NULL: the up blocks' `cat([hidden, skip], 1)`, unet_blocks.py:683,798, read in place);
 *   Hs, Ws = H, W, or H / 2, W / 2 with upsample2x (nearest 2x upsample folded into the halo addressing); H, W = OUTPUT size, W % 32 == 0;
 *   w_packed = fmc_conv3x3_halo_pack_weight(filter [Cout][3][3][Cin]): Cin (both sources) % 64 == 0, Cout % 160 == 0;
 *   bias [Cout] | NULL, temb / temb_row_stride / temb_img_div and residual [n_img, H, W, Cout] | NULL as for fmc_conv3x3_bf16;
 *   gn_coef [n_img, Cin, 2] fp32 | NULL: the operand is act(x * gn_coef[i, c, 0] + gn_coef[i, c, 1]) rounded to bf16 (act = SiLU when gn_act),
 *     zero outside the image (the reference pads the NORMALISED tensor); produced by fmc_groupnorm_coef;
 *   gn_partials [n_img, fmc_conv3x3_halo_tiles_per_image(H, W), 32, 2] fp32 | NULL: (sum, sum of squares) of the bf16-rounded outputs per image,
 *     pixel tile and group of Cout / 32 channels -- the statistics pass of the GroupNorm that consumes `out` (fmc_groupnorm_coef /
 *     fmc_groupnorm_apply_fwd take them as `partials` with part_splits = tiles per image).
 * fmc_groupnorm_coef: partial sums [N, part_splits, G, 2] -> coef [N, C, 2] = (rstd gamma_c, beta_c - mean rstd gamma_c) and, when stats != NULL,
 *   stats [N, G, 2] = (mean, rstd); HW = pixels per image (count per group = HW * C / G); fp64 combination, deterministic. */
/* ---------------------------------------------------------------------------------------------
 * Token GEMM for the small-M projections of the 10x16 / 5x8 levels (csrc/gemm4.hip, round 5): nn.Linear of diffusers' Attention / Transformer2D / the
 * motion module there (fmc/models/attention_processor.py:50-69,255-283, fmc/models/motion_module.py:219,228,284) with what follows it,
 *   out = alpha * (x W^T + bias) + residual + residual2          (bf16; any of bias / residual / residual2 NULL; residual2 needs residual),
 * on 160 x 160 tiles, 4 waves, software-pipelined fragment reads and operand requests.  x rows ldx apart, residual(s) ldres, out ldo; W [N, K] row-major.
 * K % 64 == 0, N % 8 == 0, strides % 8 == 0, operands < 2 GiB; edge tiles are masked.  An arm of `hip_ops.linear`'s per-shape choice (700). */
int fmc_linear4_supported(int64_t M, int N, int K, int64_t ldx);
int fmc_linear4_bf16(const void* x, const void* w, const void* bias, const void* residual, const void* residual2, void* out, int64_t M, int N, int K,
                     int64_t ldx, int64_t ldres, int64_t ldo, float alpha, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The vendor arm of the token projections, called directly (csrc/vendor_gemm.hip, round 5): out = x W^T + bias + residual as ONE hipBLASLt launch
 * (D = A B + beta C with the bias epilogue) -- nn.Linear + the residual add of attention to_out / the feed-forward output / proj_out
 * (fmc/models/attention_processor.py:69, fmc/models/motion_module.py:228,299) where the per-shape choice is the library.  torch's F.linear cannot pass C and
 * bias together and followed the GEMM with an elementwise add.  bf16; bias [N] | NULL; residual rows ldres apart | NULL; x rows ldx, out rows ldo apart;
 * W [N, K] row-major.  `algo` indexes the heuristic's candidate list, 0 <= algo < fmc_vendor_linear_candidates(...) (0 = the library's first choice).
 * Ownership (round 6): nothing here allocates device memory.  fmc_vendor_init() creates the library handle of the CURRENT device (idempotent),
 * fmc_vendor_destroy() drops it together with the device's cached plans; every other entry point fails with FMC_E_NULL before init.  Split-K / stream-K
 * candidates need scratch: the caller passes `workspace` (16-byte aligned, >= fmc_vendor_workspace_bytes() = the size candidates are planned for; one buffer
 * per stream that issues these calls, NULL / 0 allowed for candidates that need none).  The first call for a problem queries the heuristic (host work):
 * make it outside stream capture.  fmc_vendor_version() = hipblasLtGetVersion (candidate indices are only meaningful within one library version). */
int fmc_vendor_init(void);
int fmc_vendor_destroy(void);
int fmc_vendor_version(void);
int64_t fmc_vendor_workspace_bytes(void);
int fmc_vendor_linear_candidates(int64_t M, int N, int K, int64_t ldx, int64_t ldres, int64_t ldo, int has_bias, int has_residual);
int fmc_vendor_linear_bf16(const void* x, const void* w, const void* bias, const void* residual, void* out, int64_t M, int N, int K,
                           int64_t ldx, int64_t ldres, int64_t ldo, int algo, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-head attention for the steps either side of the denoising loop (csrc/attn_generic.hip, round 6): softmax(q k^T scale + mask) v
 * for the shapes the hot-path kernels above do not take -- the VAE mid block's single head of width 512 (diffusers AutoencoderKL; reached from
 * `decode_latents`, fmc/pipelines/pipeline_animation_cm_om.py:465-478, and `vae.encode`, train_cam_obj_ctrl.py:786) and CLIP's causal text self-attention
 * (`_encode_prompt`, pipeline_animation_cm_om.py:480-568).  q [B, Sq, H D], k / v [B, Skv, H D] with batch / row strides in elements (slices of a fused
 * projection are fine), o [B, Sq, H D]; D in {32, 64, 128, 256, 512}; `causal`: key j attends to query i only when j <= i; `key_keep` [B][Skv] bytes
 * (1 = attend) or NULL; dtype FMC_BF16 or FMC_F32 (split-bf16 x3 products).  A fully masked row yields zeros. */
int fmc_attention_supported(int D);
int fmc_attention_fwd(const void* q, const void* k, const void* v, void* o, const unsigned char* key_keep, int B, int H, int Sq, int Skv, int D,
                      int64_t q_batch_stride, int64_t q_row_stride, int64_t kv_batch_stride, int64_t kv_row_stride, int64_t o_batch_stride,
                      int64_t o_row_stride, float scale, int causal, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm + GEGLU projection with the gate software-pipelined under the matrix work (csrc/geglu_pipe.hip, round 6): diffusers FeedForward's
 * `GEGLU(norm(h))` (fmc/models/motion_module.py:295-299; BasicTransformerBlock.norm3 / ff) at C = 320 | 640 -- same function as fmc_geglu320_ln_bf16 /
 * fmc_geglu640_ln_bf16: out [M, cff] = (n W_v^T + b_v) * gelu(n W_g^T + b_g), n = LayerNorm(h).  One wave per SIMD keeps two accumulator sets and gates
 * chunk c - 1 in the shadow of chunk c's MFMAs; no staging tile, no barrier after the LayerNorm.  variant 0: 80-row tiles, 4 waves x 32 gated columns
 * (C = 320 | 640, M % 80 == 0); variant 1: 160-row tiles, 8 waves x 16 gated columns (C = 320, M % 160 == 0: every weight fragment serves twice the rows).
 * w_packed: `hip_ops.pack_geglu_frag(w, G)`, G = 32 (variant 0) | 16 (variant 1): [cff / G column groups][C / 32 k-steps][G / 8 blocks: value blocks, then gate
 * blocks][lane][8]; bias [2 cff] (value | gate) or NULL; cff % 128 == 0; out_blocked: tile-major [M / 160][cff / 32][160][32] (the operand layout of the
 * feed-forward's second GEMM; M % 160 == 0). */
int fmc_geglu_pipe_supported(int64_t M, int cff, int C, int variant);
int fmc_geglu_pipe_ln_bf16(const void* h, void* out, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w_packed, const void* bias,
                           int64_t M, int cff, int C, int out_blocked, int variant, void* stream);
/* The same with a partly filled last tile: any M >= 1, ceil(M / 80 | 160) workgroups.  Pad rows read the tile's last valid row again and are not stored.
 * out_blocked: out is ceil(M / 160) WHOLE tiles [cff / 32][160][32] -- the caller allocates the padded size, the pad rows of the last tile are left as they
 * were.  Valid rows are bit-identical to fmc_geglu_pipe_ln_bf16 on the same tokens padded to whole tiles. */
int fmc_geglu_pipe_partial_supported(int64_t M, int cff, int C, int variant);
int fmc_geglu_pipe_ln_partial_bf16(const void* h, void* out, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w_packed, const void* bias,
                                   int64_t M, int cff, int C, int out_blocked, int variant, void* stream);

/* The statistics pass of fmc_groupnorm_silu_fwd alone (x read once, nothing written but the sums): partials [N][splits][G][2] fp32 with
 * splits = fmc_groupnorm_partial_splits(HW, C); x2 / C1: two-source channel concat as for fmc_groupnorm_silu_fwd. */
int fmc_groupnorm_partial_splits(int HW, int C);
int fmc_groupnorm_partials(const void* x, const void* x2, int C1, float* partials, int N, int HW, int C, int G, int dtype, void* stream);
int fmc_conv3x3_halo_supported(int n_img, int H, int W, int Cin, int Cin1, int Cout, int upsample2x);
int64_t fmc_conv3x3_halo_packed_bytes(int Cin, int Cout);
int fmc_conv3x3_halo_pack_weight(const void* w, void* dst, int Cin, int Cout, void* stream);
int fmc_conv3x3_halo_tiles_per_image(int H, int W);
int fmc_conv3x3_halo_bf16(const void* x, const void* x2, int Cin1, const void* w_packed, const void* bias, const void* temb, const void* residual,
                          void* out, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride, int temb_img_div, int upsample2x,
                          const float* gn_coef, int gn_act, float* gn_partials, void* stream);
/* Shortcut mode (inference): conv2 of diffusers' ResnetBlock2D with the block's 1x1 `conv_shortcut` in the same reduction (unet_blocks.py:306-317 with
 * in_channels != out_channels): out = conv3x3(x) + w_sc . [xs | xs2] + bias + temb, one sum over K = 9 Cin + Cin_sc whose last Cin_sc channels are
 * multiplied at the centre tap only -- no shortcut GEMM, no [M, Cout] round trip, the shortcut product is not rounded.  Plain convolution of ONE source
 * (no GroupNorm operand path, no upsample, no residual).  xs [n_img, H, W, Cin_sc1] (+ xs2 [n_img, H, W, Cin_sc - Cin_sc1] | NULL), raw, read in place;
 * both % 64 channels, 16-byte aligned, < 2 GiB.  w_packed = fmc_conv3x3_halo_sc_pack_weight(filter [Cout][3][3][Cin], w_sc [Cout][Cin_sc]):
 * [Cout / tile_channels][(Cin / 64) * 18 + (Cin_sc / 64) * 2 sub-tiles][tile_channels rows][32], the 1x1 filter's sub-tiles [Cin_sc / 64][2 halves]
 * behind the 3x3 ones, chunk-swizzled like them; tile_channels = 160 for fmc_conv3x3_halo_sc_bf16 (80: the 4-wave tile, packed but not launched yet).
 * The shortcut's bias goes in as `temb` (one row, temb_img_div = n_img): bias + temb are summed in fp32.  gn_partials as fmc_conv3x3_halo_bf16. */
int fmc_conv3x3_halo_sc_supported(int n_img, int H, int W, int Cin, int Cout, int Cin_sc, int Cin_sc1);
int64_t fmc_conv3x3_halo_sc_packed_bytes(int Cin, int Cout, int Cin_sc);
/* (host only, no launch) 16-byte chunk `chunk` of the packed filter = the eight elements from the returned index on of the 3x3 filter, or of
 * w_sc when *from_shortcut: the pack kernel's index map. */
int64_t fmc_conv3x3_halo_sc_pack_source(int64_t chunk, int Cin, int Cin_sc, int tile_channels, int* from_shortcut);
int fmc_conv3x3_halo_sc_pack_weight(const void* w, const void* w_sc, void* dst, int Cin, int Cout, int Cin_sc, int tile_channels, void* stream);
int fmc_conv3x3_halo_sc_bf16(const void* x, const void* w_packed, const void* bias, const void* temb, void* out, const void* xs, const void* xs2,
                             int Cin_sc1, int Cin_sc, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride, int temb_img_div,
                             float* gn_partials, void* stream);
/* The same convolution for the SMALL feature maps (csrc/conv_halo4.hip): image width a multiple of 8; the image is cut into row blocks of 10 x 16
 * pixels (W % 16 == 0) or 5 x 8; a tile is 320 pixels = 2 / 8 row blocks x 80 output channels, 4 waves with software-pipelined fragment reads.  Arguments as
 * fmc_conv3x3_halo_bf16 without the GroupNorm operand path; Cout % 80 == 0; w_packed = fmc_conv3x3_halo4_pack_weight(filter);
 * gn_partials [n_img, fmc_conv3x3_halo4_row_blocks_per_image(H, W), 32, 2].  fmc_conv3x3_halo4_tiles: workgroups an un-split launch has.
 * split_k > 1 (5x8-pixel images: 64 tiles on 256 CUs otherwise): the 64-channel chunks of the reduction are dealt to split_k workgroups per tile, fp32
 * partials in `workspace` (>= split_k * n_img * H * W * Cout * 4 bytes), summed in a fixed order by a second launch that runs the epilogue.
 * wide != 0 (W % 16 == 0, Cout % 160 == 0; its own packed filter): 8 waves, two per SIMD, 320 pixels x 160 channels per tile -- the same software-pipelined
 * loop where that many tiles fill the chip (the 40x64 / 20x32 levels). */
int fmc_conv3x3_halo4_supported(int n_img, int H, int W, int Cin, int Cin1, int Cout, int upsample2x, int wide);
int fmc_conv3x3_halo4_pack_weight(const void* w, void* dst, int Cin, int Cout, int wide, void* stream);
int fmc_conv3x3_halo4_row_blocks_per_image(int H, int W);
int fmc_conv3x3_halo4_tiles(int n_img, int H, int W, int Cout, int wide);
int fmc_conv3x3_halo4_bf16(const void* x, const void* x2, int Cin1, const void* w_packed, const void* bias, const void* temb, const void* residual,
                           void* out, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride, int temb_img_div, int upsample2x,
                           float* gn_partials, int split_k, void* workspace, int64_t workspace_bytes, int wide, void* stream);
/* Phase mode of the nearest-2x upsample convolutions (inference, frozen filter).  conv3x3(upsample2x(src)) is four 2x2-tap convolutions of src, one
 * per output parity (py, px): out[2i+py, 2j+px] = sum_{a,b} Wf[py][px][a][b] . src[i+py-1+a, j+px-1+b], src zero-padded by one pixel, with
 * Wf[0][.][0] = w[0], Wf[0][.][1] = w[1] + w[2], Wf[1][.][0] = w[0] + w[1], Wf[1][.][1] = w[2] over the filter's rows (columns likewise with px, b):
 * 4 taps per output instead of 9.  fmc_conv3x3_upfold_pack_weight folds the bf16 filter [Cout][3][3][Cin] (sums in fp32, rounded to bf16 once) into
 * the consuming kernel's sub-tile order, `dst` = fmc_conv3x3_upfold_packed_bytes = 16 / 9 of the filter; tile_channels = 160 for
 * fmc_conv3x3_halo_fold_bf16 and the wide halo4 form, 80 for the 4-wave halo4 form.  The *_fold_bf16 launches take the SOURCE size Hs x Ws (halo:
 * Ws % 32 == 0; halo4: Ws % 8 == 0), write out [n_img, 2 Hs, 2 Ws, Cout] with bias in the epilogue (no temb / residual / GroupNorm operand path /
 * split-K), and leave gn_partials [n_img, 4 * tiles (row blocks) per SOURCE image, 32, 2] of the rounded outputs.  Results differ from
 * upsample2x = 1 of the launches above only by the one re-rounding of the folded filter; those stay the path for training and raw filters. */
int64_t fmc_conv3x3_upfold_packed_bytes(int Cin, int Cout);
int fmc_conv3x3_upfold_pack_weight(const void* w, void* dst, int Cin, int Cout, int tile_channels, void* stream);
int fmc_conv3x3_halo_fold_supported(int n_img, int Hs, int Ws, int Cin, int Cout);
int fmc_conv3x3_halo_fold_bf16(const void* x, const void* w_folded, const void* bias, void* out, int n_img, int Hs, int Ws, int Cin, int Cout,
                               float* gn_partials, void* stream);
int fmc_conv3x3_halo4_fold_supported(int n_img, int Hs, int Ws, int Cin, int Cout, int wide);
int fmc_conv3x3_halo4_fold_bf16(const void* x, const void* w_folded, const void* bias, void* out, int n_img, int Hs, int Ws, int Cin, int Cout,
                                float* gn_partials, int wide, void* stream);
/* The halo convolutions at ANY image width: partly filled column tiles.  Each *_partial_* entry is the entry of the same name above with its width
 * rule dropped (W >= 1; every other condition, every operand and the packed filters -- there are no new pack routines -- are the same).  The column
 * tile count is a ceiling, ceil(W / 32) for conv_halo and ceil(W / tw) for conv_halo4; the last tile of an image row holds the W - x0 columns that
 * exist: a pad column is multiplied on zeros-padded input like any other and never fetched from (shortcut sources, residual), stored to, summed
 * into the statistics or written to the split-K workspace.  A whole-tile shape gives the bits, output and statistics, of the whole-tile entry (for
 * conv_halo4 at the geometry that entry picks: tw = 16 where W % 16 == 0, else 8).
 *   conv_halo: gn_partials is [n_img, ceil(H / 10) * ceil(W / 32), 32, 2] (fold: 4 x as many splits, [source tile][phase]);
 *     fmc_conv3x3_halo_partial_tiles_per_image returns the middle extent.
 *   conv_halo4: the caller names the row-block geometry `tw`, 16 (10 x 16 pixels; the only one of the wide form) or 8 (5 x 8);
 *     fmc_conv3x3_halo4_partial_tw returns the default -- the whole-tile entry's where W % 8 == 0, else the one with fewer pad pixels over the image,
 *     ceil(H / TH) TH ceil(W / tw) tw, ties to 16.  gn_partials is [n_img, ceil(H / TH) * ceil(W / tw), 32, 2] with TH = 10 (tw 16) or 5 (tw 8):
 *     fmc_conv3x3_halo4_partial_row_blocks_per_image; fmc_conv3x3_halo4_partial_tiles counts the workgroups of one split.
 * The whole-tile entries keep refusing ragged widths. */
int fmc_conv3x3_halo_partial_supported(int n_img, int H, int W, int Cin, int Cin1, int Cout, int upsample2x);
int fmc_conv3x3_halo_partial_tiles_per_image(int H, int W);
int fmc_conv3x3_halo_partial_bf16(const void* x, const void* x2, int Cin1, const void* w_packed, const void* bias, const void* temb,
                                  const void* residual, void* out, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride,
                                  int temb_img_div, int upsample2x, const float* gn_coef, int gn_act, float* gn_partials, void* stream);
int fmc_conv3x3_halo_sc_partial_supported(int n_img, int H, int W, int Cin, int Cout, int Cin_sc, int Cin_sc1);
int fmc_conv3x3_halo_sc_partial_bf16(const void* x, const void* w_packed, const void* bias, const void* temb, void* out, const void* xs,
                                     const void* xs2, int Cin_sc1, int Cin_sc, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride,
                                     int temb_img_div, float* gn_partials, void* stream);
int fmc_conv3x3_halo_fold_partial_supported(int n_img, int Hs, int Ws, int Cin, int Cout);
int fmc_conv3x3_halo_fold_partial_bf16(const void* x, const void* w_folded, const void* bias, void* out, int n_img, int Hs, int Ws, int Cin,
                                       int Cout, float* gn_partials, void* stream);
int fmc_conv3x3_halo4_partial_supported(int n_img, int H, int W, int Cin, int Cin1, int Cout, int upsample2x, int wide);
int fmc_conv3x3_halo4_partial_tw(int H, int W, int wide);
int fmc_conv3x3_halo4_partial_row_blocks_per_image(int H, int W, int tw);
int fmc_conv3x3_halo4_partial_tiles(int n_img, int H, int W, int Cout, int wide, int tw);
int fmc_conv3x3_halo4_partial_bf16(const void* x, const void* x2, int Cin1, const void* w_packed, const void* bias, const void* temb,
                                   const void* residual, void* out, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride,
                                   int temb_img_div, int upsample2x, float* gn_partials, int split_k, void* workspace, int64_t workspace_bytes,
                                   int wide, int tw, void* stream);
int fmc_conv3x3_halo4_fold_partial_supported(int n_img, int Hs, int Ws, int Cin, int Cout, int wide);
int fmc_conv3x3_halo4_fold_partial_bf16(const void* x, const void* w_folded, const void* bias, void* out, int n_img, int Hs, int Ws, int Cin,
                                        int Cout, float* gn_partials, int wide, int tw, void* stream);
/* Backward-data of the two resampling convolutions (training, frozen filter; csrc/conv_resample_bwd.hip).  The filter is the forward's
 * [Cout][3][3][Cin] (channels-last), Cin % 64 == 0 and Cout % 64 == 0, any n_img >= 1, every tensor below 2^31 bytes; dY and dX are channels-last bf16,
 * fp32 accumulation on v_mfma_f32_16x16x32_bf16, bias-free (a bias has no data gradient).  No W % 8 / W % 32 rule: the tiles run over a flat pixel list.
 *   down (3x3, stride 2, pad 1; the forward's input H x W even, >= 2; dY [n_img, H/2, W/2, Cout] -> dX [n_img, H, W, Cin]):
 *     dX[2i+py, 2j+px] = sum over (ky, di) in T[py], (kx, dj) in T[px] of W[.][.][ky][kx]^T dY[i+di, j+dj], T[0] = {(1, 0)}, T[1] = {(2, 0), (0, +1)},
 *     zero outside dY: four launches' worth of 1 / 2 / 2 / 4 taps in one grid, stored pixel-shuffled -- 2.25 taps per output on average, not 9.
 *   up (conv3x3(nearest2x(src)), src Hs x Ws >= 1; dY [n_img, 2 Hs, 2 Ws, Cout] -> dX [n_img, Hs, Ws, Cin]):
 *     dX[u, v] = sum_{r,c=0..3} G[r][c]^T dY[2u-1+r, 2v-1+c] with the rows of G from the rows of W: w[2], w[1] + w[2], w[0] + w[1], w[0] (columns
 *     likewise) -- the transpose of the fold of fmc_conv3x3_upfold_pack_weight, summed in fp32 in the same order and rounded to bf16 once: 16 taps
 *     per output against 36 of a full-resolution convolution followed by a 2x2 sum.
 * `tile`: 0 = the launcher's choice by how many tiles fill the chip (what *_bwd_tile returns for the shape on the current device); down 1 / 2 / 3 = 32 x 64,
 * 16 x 64, 16 x 32 (pixels x input channels) per wave; up 1 = 32 x 64 with all 16 taps per wave, 2 = the four rows of G on the four waves of a workgroup,
 * summed in a fixed order.  Every choice computes every shape of the domain; another value is FMC_E_SHAPE.
 * *_pack_weight writes `dst` = *_packed_bytes (9 resp. 16 x Cin x Cout x 2) in MFMA fragment order, once per weight version; the launches allocate nothing,
 * use no atomics and no workspace (bit-reproducible) and never read outside dY.  Anything outside the domain: FMC_E_SHAPE (ask *_supported). */
int fmc_conv3x3_down_bwd_supported(int n_img, int H, int W, int Cin, int Cout);
int64_t fmc_conv3x3_down_bwd_packed_bytes(int Cin, int Cout);
int fmc_conv3x3_down_bwd_pack_weight(const void* w, void* dst, int Cin, int Cout, void* stream);
int fmc_conv3x3_down_bwd_tile(int n_img, int H, int W, int Cin, int Cout);
int fmc_conv3x3_down_bwd_bf16(const void* dy, const void* w_packed, void* dx, int n_img, int H, int W, int Cin, int Cout, int tile, void* stream);
int fmc_conv3x3_up_bwd_supported(int n_img, int Hs, int Ws, int Cin, int Cout);
int64_t fmc_conv3x3_up_bwd_packed_bytes(int Cin, int Cout);
int fmc_conv3x3_up_bwd_pack_weight(const void* w, void* dst, int Cin, int Cout, void* stream);
int fmc_conv3x3_up_bwd_tile(int n_img, int Hs, int Ws, int Cin, int Cout);
int fmc_conv3x3_up_bwd_bf16(const void* dy, const void* w_packed, void* dx, int n_img, int Hs, int Ws, int Cin, int Cout, int tile, void* stream);
int fmc_groupnorm_coef(const float* partials, int part_splits, const float* gamma, const float* beta, float* coef, float* stats, int N, int HW,
                       int C, int G, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp32-storage ("parity") mode of the two GEMMs above: split-bf16 x3 on the SAME kernels.
 * The reference's CPU path is fp32 (north_star: outputs within 1e-3 rel-inf of it); the bf16 product path can only be held
 * to bf16's own rounding against it.  To check the hand-written tile maps, operand loaders (token / implicit 3x3 conv /
 * upsample / stride 2), fragment layouts, split-K order and epilogue arithmetic at fp32 accuracy, every fp32 operand is
 * split into bf16 `hi` and bf16 `lo = bf16(x - hi)` (x = hi + lo to ~2^-17 relative) and laid out along the reduction:
 *     activation rows  [hi | hi | lo]      weight rows  [hi | lo | hi]       (three blocks of K columns each)
 * so that ONE bf16 MFMA GEMM over K3 = 3 K accumulates hi hi' + hi lo' + lo hi' in fp32 -- the fp32 product up to the
 * dropped lo lo' term (2^-18).  Same call sites as fmc_linear_bf16 / fmc_conv3x3_bf16 when the model is held in fp32
 * (fmc/models/attention_processor.py:50-69,255-283, motion_module.py:219,228,284, unet_blocks.py:306-317,625).
 *
 * fmc_split_bf16x3: src fp32 [rows, C] (rows `ld_src` floats apart) -> dst bf16 [rows, 3 K] (rows `ld_dst` apart), columns
 *   [col0, col0 + C) of each of the three K-blocks; role 0 = activation pattern, 1 = weight pattern.  col0 / K let a
 *   two-source operand (`x2` of fmc_linear_bf16) be written into one buffer.  For the convolution the rows are pixels
 *   (C = K = Cin: x3 is [n, H, W, 3 Cin]) resp. (Cout, tap) pairs (w3 is [Cout, 3, 3, 3 Cin]).  C, K, col0 % 8 == 0.
 * fmc_linear_x3_f32 / fmc_conv3x3_x3_f32: as fmc_linear_bf16 / fmc_conv3x3_bf16 on such operands (K3 = 3 K, Cin3 = 3 Cin),
 *   with bias / temb / residual(s) / out in FP32 (strides in floats, % 4 == 0) and the whole epilogue (bias, alpha, temb,
 *   residuals, exact-erf GEGLU) in fp32 straight from the accumulator registers.  tile: arms 1..14 (15 falls back to 5);
 *   split_k >= 1 only (no stream-K); no two-source operand (split both sources into one x3).
 * ------------------------------------------------------------------------------------------- */
int fmc_split_bf16x3(const float* src, void* dst, int64_t rows, int C, int64_t ld_src, int64_t ld_dst, int col0, int K,
                     int role, void* stream);
int fmc_linear_x3_f32(const void* x3, const void* w3, const float* bias, const float* residual, float* out, int64_t M, int N,
                      int K3, int64_t ldx, int64_t ldres, int64_t ldo, float alpha, int epilogue, int tile, int split_k,
                      void* workspace, int64_t workspace_bytes, const float* residual2, void* stream);
int fmc_conv3x3_x3_f32(const void* x3, const void* w3, const float* bias, const float* temb, const float* residual, float* out,
                       int n_img, int H, int W, int Cin3, int Cout, int64_t temb_row_stride, int temb_img_div,
                       int upsample2x, int tile, int split_k, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward entry points (training stages 2/3 of the reference: the U-Net is frozen but the activation gradient
 * flows through every layer back to the OMC / CMC injection points, train_cam_obj_ctrl.py:917-929,
 * train_cam_ctrl.py:626-650; in the reference this is PyTorch autograd through the same call sites as the forwards).
 * ------------------------------------------------------------------------------------------- */
/* dX (and optionally dgamma / dbeta, fp32 [C], ACCUMULATED into: zero them first) of fmc_layernorm_fwd. */
int fmc_layernorm_bwd(const void* dy, const void* x, const float* gamma, void* dx, float* dgamma, float* dbeta,
                      int64_t M, int C, float eps, int dtype, void* stream);
/* The same two backward passes with an ADDEND (shape of dx, may be NULL): dx = addend + dX(norm).  In `h + f(norm(h))` -- every residual
 * connection of the U-Net (diffusers ResnetBlock2D / BasicTransformerBlock, fmc/models/motion_module.py:282-300) -- h receives a gradient
 * along the skip and one through the norm; autograd sums them with an elementwise kernel per connection (303 launches per training step,
 * train_cam_obj_ctrl.py:915); a norm node that owns both uses of h takes the skip gradient here instead. */
int fmc_layernorm_bwd_add(const void* dy, const void* x, const float* gamma, void* dx, float* dgamma, float* dbeta, const void* addend,
                          int64_t M, int C, float eps, int dtype, void* stream);
int fmc_groupnorm_silu_bwd_add(const void* dy, const void* x, void* dx, const float* gamma, const float* beta, const float* stats,
                               void* workspace, int N, int HW, int C, int G, int act, const void* addend, int dtype, void* stream);
/* GroupNorm(+SiLU) backward WITH the affine gradients (the motion modules' `norm` under `train_mm`, train_cam_ctrl.py:289-302).  With
 * z = gamma * xh + beta, xh = (x - mean) * rstd, dz = dy * act'(z):
 *     dgamma[c] = sum_{n, s} dz * xh,   dbeta[c] = sum_{n, s} dz          (fp32 [C]; accumulate != 0 adds to what is there)
 *   dx : as fmc_groupnorm_silu_bwd_add (same addend, SAME BITS), or NULL: the dX pass is skipped (a norm whose input needs no gradient).
 *   The statistics pass of the dX-only backward also emits per-(sample, split, channel) partials of (dz, dz * xh) from the registers
 *   it already holds -- x and dy are read once, as there -- and a second kernel sums them in a fixed order: bit-reproducible.
 *   workspace: fp32 scratch of fmc_groupnorm_silu_bwd_params_workspace_bytes(N, HW, C, G) bytes, 16-byte aligned.  bf16 / fp32. */
int64_t fmc_groupnorm_silu_bwd_params_workspace_bytes(int N, int HW, int C, int G);
int fmc_groupnorm_silu_bwd_params(const void* dy, const void* x, void* dx, float* dgamma, float* dbeta, const float* gamma,
                                  const float* beta, const float* stats, const void* addend, int accumulate, void* workspace,
                                  int N, int HW, int C, int G, int act, int dtype, void* stream);
/* Column sum of a token matrix (bias gradients of trainable projections):
 *     out[n] = alpha * sum_{m < M} x[m][n]   (+ out[n] when accumulate != 0),   out fp32 [N]
 *   x bf16 / fp32 [M, N] with rows `ld` >= N elements apart (a column slice of a wider tensor is fine), no alignment requirement.
 *   The rows are split over workgroups by a rule that depends on (M, N) alone; the fp32 partials go to `workspace`
 *   (fmc_column_sum_workspace_bytes(M, N) bytes) and a second kernel sums them in a fixed order: bit-reproducible. */
int64_t fmc_column_sum_workspace_bytes(int64_t M, int N);
int fmc_column_sum(const void* x, float* out, int64_t M, int N, int64_t ld, float alpha, int accumulate, void* workspace, int dtype,
                   void* stream);
/* dX [M, 2*Cff] of fmc_geglu_fwd from dy [M, Cff] and the forward input x. */
int fmc_geglu_bwd(const void* dy, const void* x, void* dx, int64_t M, int Cff, int dtype, void* stream);
/* dQ, dK, dV of fmc_spatial_attn_fwd.  o / lse are the forward's outputs, d_o has o's strides, dvec is a
 * [B, H, Sq] fp32 scratch (receives rowsum(dO .* O)).  dk / dv are [B / kv_batch_div, Skv, H*D]: frames sharing one
 * text K/V are summed inside the kernel.  dk and dv may be NULL together (frozen text projections: the key/value
 * side needs no gradient); the dK/dV kernel is then not launched. */
int fmc_spatial_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                         float* dvec, void* dq, void* dk, void* dv, int B, int H, int Sq, int Skv, int D,
                         int64_t q_batch_stride, int64_t q_row_stride, int64_t kv_batch_stride, int64_t kv_row_stride,
                         int64_t o_batch_stride, int64_t o_row_stride, int64_t dq_batch_stride, int64_t dq_row_stride,
                         int64_t dkv_batch_stride, int64_t dkv_row_stride, int kv_batch_div, float scale, int dtype,
                         void* stream);
/* dQ, dK, dV of fmc_temporal_attn_fwd (probabilities are recomputed; nothing saved by the forward).
 * q/k/v share (clip, frame, pix) strides, d_o has its own, dq/dk/dv share a third triple.  1 <= F <= 32. */
int fmc_temporal_attn_bwd(const void* q, const void* k, const void* v, const void* d_o, void* dq, void* dk, void* dv,
                          int n_clips, int n_pix, int F, int H, int D, int64_t clip_stride, int64_t frame_stride,
                          int64_t pix_stride, int64_t do_clip_stride, int64_t do_frame_stride, int64_t do_pix_stride,
                          int64_t dq_clip_stride, int64_t dq_frame_stride, int64_t dq_pix_stride, float scale,
                          int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp8 temporal attention (BASELINE.json configs[4]).  Same chain as fmc_temporal_attn_fwd (attention_processor.py:267-281
 * reached from motion_module.py:365-389), with Q, K, V stored as OCP e4m3 bytes + one fp32 scale per tensor
 * (value = byte * scale).
 *
 * fmc_linear_fp8_qkv: the fused q | k | v projection `x @ w^T` (x [M, K] bf16 rows ldx apart, w [N = 3C, K] bf16, no bias:
 *   to_q / to_k / to_v have none) on the 8-phase bf16 MFMA kernel with an e4m3 epilogue: column block b = n / C is written as
 *   sat(acc * inv_scales[b]) to out_fp8 [M, N] bytes.  inv_scales: 3 device floats (1 / scale).  amax_bits (3 device words,
 *   may be NULL): running max |acc| per block as float bit patterns (atomicMax) -- what a delayed-scaling policy derives the
 *   next call's scales from.
 * fmc_temporal_attn_fp8_fwd: S^T = K Q^T on v_mfma_f32_16x16x32_fp8_fp8, softmax in fp32, P V on the bf16 MFMA with V
 *   converted e4m3 -> bf16 (exact); o is bf16.  q/k/v strides in bytes (multiples of 16), o strides in elements; scales = 3
 *   device floats {scale_q, scale_k, scale_v}.  1 <= F <= 32.
 * fmc_temporal_attn_fp8_bwd: fmc_temporal_attn_bwd with e4m3 q, k, v (dequantised while staged; d_o, dq, dk, dv bf16).  1 <= F <= 32.
 * fmc_fp8_scales_roll: the delayed-scaling update, one tiny launch: scale[b] = max(margin * amax[b] / 448, 1e-12),
 *   inv_scale[b] = 1 / scale[b], amax[b] = 0 for the three blocks (all fp32 device words; amax as written by the atomicMax of
 *   non-negative float bit patterns).
 * ------------------------------------------------------------------------------------------- */
int fmc_fp8_scales_roll(void* amax, void* scale, void* inv_scale, float margin, void* stream);
int fmc_linear_fp8_qkv(const void* x, const void* w, void* out_fp8, int64_t M, int N, int K, int64_t ldx,
                       const void* inv_scales, void* amax_bits, void* stream);
int fmc_temporal_attn_fp8_fwd(const void* q, const void* k, const void* v, void* o, const void* scales, int n_clips,
                              int n_pix, int F, int H, int D, int64_t clip_stride, int64_t frame_stride,
                              int64_t pix_stride, int64_t o_clip_stride, int64_t o_frame_stride, int64_t o_pix_stride,
                              float scale, void* stream);
int fmc_temporal_attn_fp8_bwd(const void* q, const void* k, const void* v, const void* scales, const void* d_o, void* dq,
                              void* dk, void* dv, int n_clips, int n_pix, int F, int H, int D, int64_t clip_stride,
                              int64_t frame_stride, int64_t pix_stride, int64_t do_clip_stride, int64_t do_frame_stride,
                              int64_t do_pix_stride, int64_t dq_clip_stride, int64_t dq_frame_stride,
                              int64_t dq_pix_stride, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Layout pass of the 3x3-convolution WEIGHT gradient (the trainable convs of the OMC Adapter / camera encoder;
 * `loss.backward()` at train_cam_obj_ctrl.py:915).  dW[co][dy][dx][ci] = sum_pixels dY[pixel, co] * X[pixel + tap, ci] is a GEMM
 * whose reduction index is the pixel; this pass writes a [n, H, W, C] bf16 tensor channel-major over a zero-padded pixel index
 * p = (img * (H + 2) + y + 1) * Wp + x + 1, Wp = round_up(W + 2, 8):
 *     dst[s][c][guard + p] = src[img][y][x + s - shifts / 2]   (0 in the padding and up to row_len),
 * shifts = 3 copies (dx = -1, 0, +1) for X, 1 for dY.  dW of one kernel row dy is then ONE
 * fmc_linear_bf16(x = dst_X viewed as [3 Cin, row_len] + guard + (dy - 1) * Wp, w = dst_dY [Cout, K], K = row_len of dY)
 * with split_k over the pixels: out[dx * Cin + ci][co].  (`hip_ops.conv3x3_weight_grad`)
 * ------------------------------------------------------------------------------------------- */
int fmc_nhwc_to_cmajor_padded(const void* src, void* dst, int n_img, int H, int W, int C, int64_t row_len, int guard,
                              int shifts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight gradient of a token matrix (csrc/lora_wgrad.hip): the gradients of the trainable LoRA factors of the spatial attention
 * (FMC stage 1 and stage 3 with `train_image_lora`), dU = s dY^T P and dD = s Q^T X, as reductions over the tokens of a batch
 * with both operands row-major.  Per problem:
 *     out[n][k] = alpha * sum_{m < M} a[m][n] * b[m][k]            (accumulate == 0)
 *     out[n][k] = out[n][k] + alpha * sum_{m < M} a[m][n] * b[m][k] (accumulate != 0)
 *   a bf16 [M, N] rows `lda` apart, b bf16 [M, K] rows `ldb` apart (often column slices of a fused [M, 3C] tensor), out fp32 [N, K]
 *   rows `ldo` apart.  M >= 1, N % 16 == K % 16 == 0, lda >= N, ldb >= K, ldo >= K; lda % 8 == ldb % 8 == 0, ldo % 4 == 0 and
 *   16-byte aligned pointers (FMC_E_ALIGN otherwise).  fp32 accumulate on v_mfma_f32_32x32x16_bf16, operands staged row-major into
 *   LDS and read transposed with ds_read_b64_tr_b16.
 *   One launch takes 1 .. 8 problems.  Long reductions are split over several workgroups by a rule that depends on (M, N, K) alone;
 *   their fp32 partials go to `workspace` (caller-owned, 16-byte aligned, at least the bytes `fmc_linear_wgrad_workspace_bytes`
 *   returns for the same list; NULL when that is 0) and a second kernel sums them in a fixed order: results are bit-reproducible,
 *   and a problem gives the same bits in any group.  (`hip_ops.linear_wgrad`)
 * fmc_linear_wgrad_workspace_bytes: the workspace the list needs, or -1 (with the error message set) when the list is invalid.
 * ------------------------------------------------------------------------------------------- */
typedef struct fmc_wgrad_problem {
    const void* a;
    const void* b;
    float* out;
    int64_t M, lda, ldb, ldo;
    int N, K;
    float alpha;
    int accumulate;
} fmc_wgrad_problem;
int64_t fmc_linear_wgrad_workspace_bytes(const fmc_wgrad_problem* problems, int n_problems);
int fmc_linear_wgrad_bf16(const fmc_wgrad_problem* problems, int n_problems, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight gradient of a trainable 3x3 / pad 1 convolution, straight into fp32 (csrc/conv_wgrad.hip): the same row-reduction product as
 * fmc_linear_wgrad_bf16 with an implicit-GEMM loader for the input,
 *     dw[co][ky][kx][ci] = alpha * sum_{n, yo, xo} dy[n, yo, xo, co] * x[n, s yo + ky - 1, s xo + kx - 1, ci]   (+ dw when accumulate != 0)
 *   x  [n_img, H, W, Cin]  bf16 NHWC, dy [n_img, Ho, Wo, Cout] bf16 NHWC, Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1, stride s = 1 or 2;
 *   taps outside the image contribute zero and no address outside x or dy is formed.
 *   dw fp32, dense: dw_layout = FMC_DW_OIHW is [Cout][Cin][3][3] (a contiguous nn.Conv2d weight), FMC_DW_OHWI is [Cout][3][3][Cin]
 *   (channels-last).  With accumulate the old value is added unscaled: dw = fma(alpha, sum, dw).
 *   Domain (ask fmc_conv3x3_wgrad_supported; FMC_E_SHAPE otherwise): n_img, H, W >= 1, Cin % 16 == Cout % 16 == 0, fewer than 2^31 output
 *   pixels and filter elements.  x and dy 16-byte aligned (FMC_E_ALIGN).
 *   Long reductions are split over several workgroups by a rule that depends on the shape alone; their fp32 partials go to `workspace`
 *   (caller-owned, at least fmc_conv3x3_wgrad_workspace_bytes of the same shape; NULL when that is 0) and a second kernel adds them in
 *   split order: no atomics, no allocation, bit-reproducible.  (`hip_ops.conv3x3_wgrad`)
 * fmc_conv3x3_wgrad_workspace_bytes: the workspace the shape needs, or -1 (with the error message set) outside the domain.
 * ------------------------------------------------------------------------------------------- */
#define FMC_DW_OIHW 0
#define FMC_DW_OHWI 1
int fmc_conv3x3_wgrad_supported(int n_img, int H, int W, int Cin, int Cout, int stride);
int64_t fmc_conv3x3_wgrad_workspace_bytes(int n_img, int H, int W, int Cin, int Cout, int stride);
int fmc_conv3x3_wgrad_bf16(const void* x, const void* dy, float* dw, int n_img, int H, int W, int Cin, int Cout, int stride, int dw_layout,
                           float alpha, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The fused temporal attention block of the motion modules at the 40x64 level (round 4; csrc/temporal_block.hip).
 * Replaces, for one attention block of `TemporalTransformerBlock.forward` (fmc/models/motion_module.py:287-300) as driven by
 * `TemporalSelfAttention.forward` (:349-389) and `PoseAdaptorAttnProcessor.forward` / `AttnProcessor.__call__`
 * (fmc/models/attention_processor.py:202-293 / :20-82):
 *     n = LayerNorm(h) + pe[frame];   m = merge_scale * (n W_m^T) + pose_term + n   (only with w_merge_tm);   q | k | v = m W_qkv^T;
 *     o = softmax(q k^T * scale) v per (pixel, head) over the frames;   out = o W_out^T + b_out + h
 * in ONE launch: a 160-row tile (10 pixels x 16 frames) stays in LDS from h to out, q / k / v / scores / o live in registers.
 *   h, out, pose_term: bf16 [n_clips, frames, hw, channels] (channels-last video tokens; out may not alias h);
 *   ln_gamma fp32 [C]; ln_bpe fp32 [frames][C] = LayerNorm beta + positional-encoding row (pe zero when the block has none);
 *   w_merge_tm / w_out_tm: the [C, C] weights tile-major [C / 32][C][32] (`hip_ops._w_tilemajor`); pose_term = merge_scale * (W_m pose + b_m);
 *   w_qkv_packed: the fused [3 C, C] projection in MFMA-fragment order per head (`hip_ops.pack_temporal_qkv`);
 *   ln_stats (optional): fp32 [rows][2] = (mean, rstd) of every out row with eps ln_stats_eps, for a consumer GEMM that applies the next
 *   LayerNorm itself (fmc_linear_bf16_lnc).
 * Shapes: frames == 16, channels == 320, heads == 8, hw % 10 == 0 (the 40x64 level of the 16x320x512 configurations); anything else is
 * FMC_E_SHAPE -- callers keep the un-fused chain there.  bf16 only.  MFMA bound: 2 rows C (C [merge] + 4 C) + 4 rows F C flops.
 * ------------------------------------------------------------------------------------------- */
int fmc_temporal_block_bf16(const void* h, void* out, const float* ln_gamma, const float* ln_bpe, float ln_eps, const void* w_merge_tm,
                            const void* pose_term, float merge_scale, const void* w_qkv_packed, const void* w_out_tm, const void* b_out,
                            float* ln_stats, float ln_stats_eps, int n_clips, int frames, int hw, int channels, int heads, float scale,
                            void* stream);
/* ---- fused text cross-attention block of the spatial transformer at the 20x32 level (round 4) ----------------------------------------------------
 * Replaces, for `attn2` of diffusers' BasicTransformerBlock as the reference U-Net builds it (fmc/models/unet_blocks.py:323-333; Attention /
 * AttnProcessor: fmc/models/attention_processor.py:20-82, :148-154 with LoRA):
 *     out = to_out(softmax(to_q(LayerNorm(h)) k^T * scale) v) + b_out + h        (k | v = the text's fused to_k / to_v projection)
 * in ONE launch (was LayerNorm + to_q GEMM + cross-attention kernel + to_out GEMM): the skeleton of the C = 640 temporal block (80-row tiles resident
 * in LDS, weights in fragment order straight into registers, wave = head), k / v fragments of the <= 80 text tokens held in registers.
 *   h, out: bf16 [n_images][hw][640] tokens, hw % 80 == 0; ln_gamma fp32 [640]; ln_bpe fp32 [16][640], every row = the LayerNorm beta;
 *   w_q_packed / w_out_frag: `hip_ops.pack_w_frag80` of the [640, 640] weights; kvfrag: fmc_xattn_pack_kv of the text k | v (one per text row);
 *   images_per_text: images that share a text row (frames of a clip).
 * fmc_xattn_pack_kv: kv bf16 [batch][S <= 80][1280] (batch stride ld_batch elements) -> bf16 [batch][8 heads][12800] MFMA fragments. */
int fmc_xattn_block640_bf16(const void* h, void* out, const float* ln_gamma, const float* ln_bpe, float ln_eps, const void* w_q_packed,
                            const void* kvfrag, const void* w_out_frag, const void* b_out, int n_images, int hw, int n_keys, int images_per_text,
                            float scale, void* stream);
int fmc_xattn_pack_kv(const void* kv, void* out, int batch, int S, int64_t ld_batch, void* stream);
/* The same block at the 40x64 level (C = 320, 8 heads x 40) on the skeleton of fmc_temporal_block_bf16 (160-row tiles, persistent): hw % 160 == 0;
 * w_q_packed = `hip_ops.pack_xattn_q40` (per head [10 k-steps][q0 | q1 | (q tail, zeros)][lane][8]), w_out_tm tile-major (`_w_tilemajor`),
 * kvfrag = fmc_xattn_pack_kv40 (kv bf16 [batch][S <= 80][640] -> [batch][8][7680]); ln_stats (optional): (mean, rstd) of every out row. */
int fmc_xattn_block320_bf16(const void* h, void* out, const float* ln_gamma, const float* ln_bpe, float ln_eps, const void* w_q_packed,
                            const void* kvfrag, const void* w_out_tm, const void* b_out, float* ln_stats, float ln_stats_eps, int n_images, int hw,
                            int n_keys, int images_per_text, float scale, void* stream);
int fmc_xattn_pack_kv40(const void* kv, void* out, int batch, int S, int64_t ld_batch, void* stream);
/* ---- the three fused attention blocks above at ANY feature-map size (hw >= 1): partly filled last tiles ------------------------------------------
 * Same arguments, tensors, weight formats and checks (NULL, alignment, 2 GiB, 1 <= n_keys <= 80, n_images % images_per_text == 0, F = 16, 8 heads,
 * C = 320 | 640) as fmc_temporal_block_bf16 / fmc_xattn_block640_bf16 / fmc_xattn_block320_bf16; only the divisibility of hw is not asked for.
 *   temporal: a clip is ceil(hw / 10) tiles of 10 pixels x 16 frames at C = 320, ceil(hw / 5) tiles of 5 pixels at C = 640; the last tile of a clip
 *     holds hw % 10 (hw % 5) pixels.
 *   text cross-attention: a segment = the images_per_text * hw consecutive rows that share a text; it is ceil(rows / 160) tiles at C = 320,
 *     ceil(rows / 80) at C = 640; tile j of segment s starts at row s * rows + 160 j (80 j) and never holds rows of two texts.
 * The pad rows of a last tile read that tile's last valid pixel / row again (every address stays inside the tensors), are computed, and are never
 * stored: not to out, not to ln_stats.  Valid rows go through exactly the operations of the whole-tile kernels: padded to whole tiles and run through
 * the entry points above, the same tokens give the same bits.  The whole-tile entry points keep refusing ragged sizes (FMC_E_SHAPE); callers opt in
 * (`hip_ops.PARTIAL_TILES`, default off). */
int fmc_temporal_block_partial_bf16(const void* h, void* out, const float* ln_gamma, const float* ln_bpe, float ln_eps, const void* w_merge_tm,
                                    const void* pose_term, float merge_scale, const void* w_qkv_packed, const void* w_out_tm, const void* b_out,
                                    float* ln_stats, float ln_stats_eps, int n_clips, int frames, int hw, int channels, int heads, float scale,
                                    void* stream);
int fmc_xattn_block640_partial_bf16(const void* h, void* out, const float* ln_gamma, const float* ln_bpe, float ln_eps, const void* w_q_packed,
                                    const void* kvfrag, const void* w_out_frag, const void* b_out, int n_images, int hw, int n_keys, int images_per_text,
                                    float scale, void* stream);
int fmc_xattn_block320_partial_bf16(const void* h, void* out, const float* ln_gamma, const float* ln_bpe, float ln_eps, const void* w_q_packed,
                                    const void* kvfrag, const void* w_out_tm, const void* b_out, float* ln_stats, float ln_stats_eps, int n_images, int hw,
                                    int n_keys, int images_per_text, float scale, void* stream);
/* ---- LayerNorm + GEGLU projection of a feed-forward at the 20x32 level, A operand resident (round 4) ----------------------------------------------
 * out[M][cff] = (n W_v^T + b_v) * gelu(n W_g^T + b_g), n = LayerNorm(h): `GEGLU.forward` of diffusers' FeedForward behind norm3 / ff_norm
 * (fmc/models/motion_module.py:295-299; BasicTransformerBlock).  A workgroup keeps its 80 normalised rows in LDS and walks the cff / 320 column chunks
 * with the chunk's weight rows streamed in MFMA-fragment order (`hip_ops.pack_geglu_frag80`) -- replaces fmc_layernorm_fwd + fmc_linear_bf16(GEGLU).
 *   h bf16 [M][640], M % 80 == 0; out bf16 [M][cff] row-major, cff % 320 == 0; bias bf16 [2 cff] (value | gate) or NULL.
 *   out_blocked != 0 (M % 160 == 0): out is written tile-major, [M / 160][cff / 32][160][32] -- the layout fmc_linear_bf16_ffblk reads with x_blocked
 *   (the intermediate is private to the feed-forward; its second GEMM then requests contiguous 10-KiB operand blocks). */
int fmc_geglu640_ln_bf16(const void* h, void* out, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w_packed, const void* bias,
                         int64_t M, int cff, int out_blocked, void* stream);
/* The same at the 40x64 level: h bf16 [M][320], cff % 160 == 0; 4 waves and 77 KiB of LDS per workgroup, two workgroups per CU. */
int fmc_geglu320_ln_bf16(const void* h, void* out, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* w_packed, const void* bias,
                         int64_t M, int cff, int out_blocked, void* stream);
/* Diagnostic: `buf` = device buffer of [workgroups][4][8] int64 that receives s_memrealtime stamps (100 MHz) of wave 0 at the phase boundaries of
 * its first four tiles (tools/scratch/r04/probe_tb.py); NULL switches the stamps off (default). */
int fmc_temporal_block_set_debug(void* buf);

/* ---------------------------------------------------------------------------------------------
 * The parameter update of the training step (csrc/optim.hip): gradient clipping per group, AdamW, the bf16 shadows of the fp32 masters
 * and the zeroing of the gradients, for MANY tensors in two passes.  Replaces `clip_grad_norm_` + `optimizer.step()` +
 * `optimizer.zero_grad()` of the reference's trainers (train_cam_obj_ctrl.py:917-943, train_cam_ctrl.py:647-665,
 * train_image_lora.py:365-381; torch.optim.AdamW with amsgrad = maximize = False).  (`hip_ops.optim_grad_norm`, `hip_ops.optim_adamw_step`,
 * `training.FusedAdamW`)
 *
 * The caller owns two tables in DEVICE memory (plus a host copy to have them checked once) and a workspace:
 *   fmc_optim_tensor, one per tensor: p, g, m, v fp32 [n]; p, m, v 16-byte aligned, g 4-byte aligned (a gradient is usually a view into a
 *     flat bucket; it is read and zeroed in 16-byte accesses all the same).  shadow_bf16 (bf16 [n]) / shadow_f32 (fp32 [n]), 16-byte
 *     aligned or NULL: receive the NEW p rounded to nearest even to bf16, and that value widened.  step: the tensor's fp32 step counter.
 *     clip_group: index of the group whose norm clips g, -1 = not clipped.  hyper_group: index of its hyper-parameter record.
 *     flags: FMC_OPTIM_ZERO_GRAD = g is zeroed after use.
 *   fmc_optim_chunk, one per workgroup: (tensor, chunk) = elements [chunk * E, min(n, (chunk + 1) * E)) of that tensor,
 *     E = fmc_optim_chunk_elems() (8192).  Every chunk of every tensor appears exactly once, in any order.
 *   hyper: fp32 [n_hyper][8] device records {lr, beta1, beta2, eps, weight_decay, max_grad_norm, 1 - beta1, 1 - beta2} (the last two
 *     rounded from double by the host: 1 - (float)0.999 is 5e-5 off).  The kernels read them from memory: a captured graph replays with
 *     whatever the host copied there last.  A clip group takes max_grad_norm from the record of its first tensor in map order.
 *   workspace: fmc_optim_workspace_bytes(...) bytes, 16-byte aligned.  After pass 1 its first n_clip_groups floats are the groups'
 *     gradient norms and the n_clip_groups floats from float index round_up(n_clip_groups, 4) the coefficients: readable by the host
 *     after its own synchronisation (logging).
 * fmc_optim_check_tables: HOST-side check of host copies of the two tables (no device access): NULL p / g / m / v / step -> FMC_E_NULL, a
 *   misaligned p / m / v / shadow -> FMC_E_ALIGN, a group index out of range or a map that does not cover every chunk exactly once ->
 *   FMC_E_SHAPE.  The launches below cannot read device tables; they check their own arguments and rely on this call for the tables.
 * fmc_optim_grad_norm (pass 1, always before pass 2): per-chunk fp32 tree sums of g^2 (depth 13 over the squares), added per clip group
 *   in a fixed order in fp64: norm = sqrt(sum), coefficient = min(1, max_grad_norm / (norm + 1e-6)) -- `clip_grad_norm_` with
 *   error_if_nonfinite=False; a non-finite norm propagates as there.  The same small kernel advances the step counter of EVERY tensor of
 *   the table and writes its bias corrections 1 - beta1^t and sqrt(1 - beta2^t), computed in fp64 once per tensor.  No atomics: equal
 *   inputs give equal bits.  With n_clip_groups == 0 only the counters and corrections are written.
 * fmc_optim_adamw_step (pass 2, one launch), per element in fp32, gc = g * coefficient[clip_group]:
 *     p <- p (1 - lr wd);  m <- m + (gc - m)(1 - beta1);  v <- beta2 v + (1 - beta2) gc^2;
 *     p <- p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps);  then the shadows and g <- 0 where asked.
 *   HBM bound: 16 bytes read and 12 (+2 +4 +4) written per element; pass 1 reads 4.
 * ------------------------------------------------------------------------------------------- */
enum { FMC_OPTIM_ZERO_GRAD = 1 };
typedef struct fmc_optim_tensor {
    float* p;
    float* g;
    float* m;
    float* v;
    uint16_t* shadow_bf16;
    float* shadow_f32;
    float* step;
    int64_t n;
    int32_t clip_group;
    int32_t hyper_group;
    int32_t flags;
    int32_t reserved;
} fmc_optim_tensor;
typedef struct fmc_optim_chunk {
    int32_t tensor;
    int32_t chunk;
} fmc_optim_chunk;
int fmc_optim_chunk_elems(void);
int64_t fmc_optim_workspace_bytes(int n_tensors, int n_chunks, int n_clip_groups);
int fmc_optim_check_tables(const fmc_optim_tensor* h_tensors, int n_tensors, const fmc_optim_chunk* h_chunks, int n_chunks, int n_hyper,
                           int n_clip_groups);
int fmc_optim_grad_norm(const fmc_optim_tensor* tensors, int n_tensors, const fmc_optim_chunk* chunks, int n_chunks, const float* hyper,
                        int n_hyper, int n_clip_groups, void* workspace, int64_t workspace_bytes, void* stream);
int fmc_optim_adamw_step(const fmc_optim_tensor* tensors, int n_tensors, const fmc_optim_chunk* chunks, int n_chunks, const float* hyper,
                         int n_hyper, int n_clip_groups, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The small bf16 passes of a Camera-Encoder / OMC-Adapter training step (csrc/train_elementwise.hip): what the chain of
 * trainable ResNet blocks and the Camera-Adapter merge needs next to its GEMMs and convolutions.  bf16 only; pure HBM passes; every
 * output element is written once by one thread (no atomics, no workspace, bit-reproducible).  Pointers need the alignment of their
 * element (2 bytes; FMC_E_ALIGN otherwise): a tensor that is 16-byte aligned moves as 16-byte vectors, any other element by element
 * (the flat kernels bring the OUTPUT to a 16-byte boundary with up to 7 leading scalar elements first).  An output may alias an input.
 *
 * fmc_avgpool2x2_fwd: AvgPool2d(kernel 2, stride 2) on NHWC.  x [n_img, H, W, C] -> y [n_img, H / 2, W / 2, C] (floor: the last row /
 *   column of an odd size is not read); C % 8 == 0 (FMC_E_SHAPE otherwise).  y = bf16(0.25f * (((x00 + x01) + x10) + x11)), the sum in
 *   fp32, rounded once.  H or W of 1: an empty output, nothing is launched (y may be NULL).
 * fmc_avgpool2x2_bwd: dy [n_img, H / 2, W / 2, C] -> dx [n_img, H, W, C], ALL of it: dx = bf16(0.25f * dy) under a window, +0 in the
 *   last row / column of an odd size (dy may be NULL where it is empty).
 * fmc_relu_fwd: y = x < 0 ? +0 : x  (std::max(x, 0): -0 and NaN pass through);  fmc_relu_bwd: dx = y > 0 ? dy : +0.
 * fmc_add_bf16: out = bf16(float(a) + float(b)).   n >= 1 elements each. */
int fmc_avgpool2x2_fwd(const void* x, void* y, int n_img, int H, int W, int C, void* stream);
int fmc_avgpool2x2_bwd(const void* dy, void* dx, int n_img, int H, int W, int C, void* stream);
int fmc_relu_fwd(const void* x, void* y, int64_t n, void* stream);
int fmc_relu_bwd(const void* dy, const void* y, void* dx, int64_t n, void* stream);
int fmc_add_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MXFP8 feed-forward GEMMs (csrc/gemm_mxfp8.hip; opt-in through hip_ops.FP8_FF, inference only).  OCP MXFP8: e4m3fn elements, one E8M0
 * scale byte per 32 consecutive elements of the reduction axis: byte = clamp(floor(log2 amax) - 8 + 127, 0, 254) (0 for an all-zero block),
 * elements x * 2^(127 - byte) clamped to +-448 and rounded to nearest even.  Inputs are finite.  No allocation, no host synchronisation.
 *
 * fmc_mxfp8_pack_weight: w [N, K] bf16 -> wq [N, K] e4m3, ws [N, K / 32] E8M0.  geglu_inner == 0: rows in order; geglu_inner = inner
 *   (N == 2 inner, inner % 64 == 0): packed row 64 t + 32 g + c is source row g * inner + 32 t + c (value and gate rows of a column
 *   in one wave's tile).  N % 64 == 0, K % 64 == 0.
 * fmc_layernorm_mxfp8_fwd: xq [M, C], xs [M, C / 32] of LayerNorm(h) (h bf16, rows ldh apart; gamma / beta fp32; fp32 statistics); h is
 *   read once.  gamma == beta == NULL: the rows of h are quantised with no normalisation, bit for bit the format above.  C % 64 == 0
 *   (C <= 2048 with gamma), ldh % 8 == 0.
 * fmc_linear_mxfp8: geglu == 0: out[m, n] = bf16(sum_k dq(x)[m, k] dq(w)[n, k] + bias[n] + residual[m, n]) (out rows ldo, residual rows
 *   ldres apart, out_scales unused); geglu == 1 (N = inner, weights packed with geglu_inner = N, bias [2 N] value | gate, no residual):
 *   (value + b_v) * gelu(gate + b_g) written as MXFP8, out = [M, N] e4m3 bytes and out_scales = [M, N / 32] E8M0 (blocks along n).
 *   fp32 accumulation on v_mfma_scale_f32_32x32x64_f8f6f4; any M >= 1 (a partly filled last row tile reads clamped rows and stores
 *   nothing past M); K % 64 == 0, N % 64 == 0, operands below 2 GiB, pointers 16-byte aligned (bias 8): fmc_linear_mxfp8_supported.
 *   Anything else is FMC_E_SHAPE / FMC_E_ALIGN and nothing is written.
 * fmc_mxfp8_tile_rows / _cols: the output tile of a workgroup (tests reach the ragged tile through them). */
int fmc_mxfp8_tile_rows(void);
int fmc_mxfp8_tile_cols(void);
int fmc_linear_mxfp8_supported(int64_t M, int N, int K, int geglu);
int fmc_mxfp8_pack_weight(const void* w, void* wq, void* ws, int N, int K, int geglu_inner, void* stream);
int fmc_layernorm_mxfp8_fwd(const void* h, const void* gamma, const void* beta, void* xq, void* xs, int64_t M, int C, int64_t ldh, float eps,
                            void* stream);
int fmc_linear_mxfp8(const void* xq, const void* xs, const void* wq, const void* ws, const void* bias, const void* residual, void* out,
                     void* out_scales, int64_t M, int N, int K, int64_t ldres, int64_t ldo, int geglu, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FMC_HIP_H */
