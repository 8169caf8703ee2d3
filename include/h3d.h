/*
 * h3d.h -- C ABI of libh3d_hip.so: the MI355X (gfx950) implementation of the multi_pose
 * inference hot path of Aaron20127/human-3d-reconstruction.
 *
 * Plain C: raw DEVICE pointers, sizes, an explicit hipStream_t (passed as void*), int error
 * codes.  No torch types.  Every entry point is asynchronous on `stream`, allocates nothing,
 * keeps no global state and is re-entrant (the reference launches on the current stream and
 * keeps a global THCState, DCNv2/src/cuda/dcn_v2_cuda.cu:12,108 -- we take the stream instead).
 *
 * Citations (file:line) are relative to /root/reference/src/lib/models/.
 */
#ifndef H3D_H
#define H3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (the reference raises C++ exceptions via AT_ASSERTM / AT_ERROR,
 *      DCNv2/src/cuda/dcn_v2_cuda.cu:61-85; kernel launch failures are only printf-ed there,
 *      dcn_v2_im2col_cuda.cu:346-350 -- here they are returned) */
#define H3D_OK 0
#define H3D_ERR_SHAPE (-1)       /* "Input shape and kernel shape wont match" class of errors   */
#define H3D_ERR_DTYPE (-2)       /* unsupported element type                                     */
#define H3D_ERR_LAUNCH (-3)      /* hipGetLastError() != hipSuccess after a launch              */
#define H3D_ERR_UNSUPPORTED (-4) /* valid request outside what the kernels cover (message set)  */
#define H3D_ERR_ARG (-5)         /* null pointer / bad enum                                      */

#define H3D_F32 0
#define H3D_BF16 1
#define H3D_F16 2 /* IEEE fp16 activations and weights, fp32 accumulation (BASELINE configs[4]: `--arch resdcn_101` runs in fp16,
                     experiments/ctdet_coco_resdcn101.sh:3); stored values saturate at +-65504 */
#define H3D_F16X3 3 /* the parity arithmetic on the fp16 matrix cores (round 5): fp32 activations in memory exactly as H3D_F32 (same ops,
                       same layouts), every contraction with both fp32 operands split into two fp16 terms x = hi + lo and three products
                       hi.hi + hi.lo + lo.hi accumulated in fp32 (the dropped lo.lo is 2^-22 relative): fp32-level results at ~3x the
                       H3D_F32 plan's rate.  Packed filters hold, per 8 consecutive input channels, 8 fp16 hi terms then 8 fp16 lo terms
                       in the 32 bytes the 8 fp32 values would occupy (engine.PackedWeights / h3d_x3_split).  |activation| <= 65504. */

/* Last error text of the calling thread (thread_local), for the Python shim's RuntimeError. */
const char *h3d_last_error(void);
/* ABI version of this header; the loader checks it. */
int h3d_abi_version(void);
#define H3D_ABI_VERSION 4      /* 2: h3d_op.wexp / wexp2 (120-byte descriptor); 3: fp32 DeformConv packs carry their filter maxima (the sizes
                                  h3d_dcn_v2_packed_weight_bytes / _workspace_bytes return grew by 256 B; bias_out of h3d_dcn_fused_pack_f32_cached
                                  is [rows | 32 | 64] floats); 4: the fp32 operator scales its activations too (h3d_dcn_v2_workspace_bytes and
                                  h3d_dcn_v2_packed_workspace_bytes grew by at most 256 B; h3d_dcn_nchw_to_nhwc_scaled).
                                  Still 4 with dcn_v2_backward: three new entry points, nothing existing changed (additive), so a library built
                                  before them still serves every older caller and tools/ab_lib.py can load it as a baseline */
/* How this library was built: H3D_BUILD_EXTRA = `make EXTRA=1` (the superseded kernel generations kept as A/B references are in:
 * H3D_OP_DCN_V1, H3D_OP_DCN_FUSED_F16, H3D_OP_UPDCN_F16, the H3D_TUNE_DCN_STREAM_F16_DCN5 DeformConv variant, h3d_smpl_verts2 -- without it they return
 * H3D_ERR_UNSUPPORTED); H3D_BUILD_ABLATE = `make ABLATE=1` (profiling switches and in-kernel stamps compiled in). */
#define H3D_BUILD_EXTRA 1
#define H3D_BUILD_ABLATE 2
int h3d_build_flags(void);

/* =====================================================================================
 * 1. Operator boundary: replaces pybind module `_ext` (DCNv2/src/vision.cpp:4-9), function
 *    `dcn_v2_forward` (DCNv2/src/dcn_v2.h:9-39 -> dcn_v2_cuda_forward, dcn_v2_cuda.cu:43-173).
 *    Same operands, same positional meaning; layouts as the reference: contiguous NCHW fp32.
 *      input  [B,C,H,W]   weight [Cout,C,kh,kw]   bias [Cout]
 *      offset [B,2*dg*kh*kw,Ho,Wo]  (channel 2t = dh, 2t+1 = dw of tap t, im2col.cu:170-171)
 *      mask   [B,dg*kh*kw,Ho,Wo]
 *      output [B,Cout,Ho,Wo], Ho=(H+2ph-(dh(kh-1)+1))/sh+1 (dcn_v2_cuda.cu:87-88)
 *    The caller allocates `output` (the reference callee allocates it, dcn_v2_cuda.cu:92).
 *    No scratch: the `columns`/`ones` buffers and pointer tables of the reference
 *    (dcn_v2_cuda.cu:90-103) do not exist -- sampling feeds the contraction through LDS.
 * ===================================================================================== */
int h3d_dcn_v2_forward(const float *input, const float *weight, const float *bias,
                       const float *offset, const float *mask, float *output,
                       int B, int C, int H, int W, int Cout,
                       int kernel_h, int kernel_w, int stride_h, int stride_w,
                       int pad_h, int pad_w, int dilation_h, int dilation_w,
                       int deformable_group, void *stream);

/* =====================================================================================
 * 1b. dcn_v2_backward (DCNv2/src/dcn_v2.h:41-74, cuda/dcn_v2_cuda.cu:175-336): the gradients of the operator above, fp32 contiguous
 *    NCHW.  Operand order of the reference (input, weight, bias, offset, mask, grad_output [B,Cout,Ho,Wo]), then the five outputs,
 *    shaped like input / offset / mask / weight / bias.  ANY of the five output pointers may be NULL: that gradient is not computed and
 *    nothing is written for it.  `bias` is not read (may be NULL).  The callee zeroes what it accumulates into (grad_input, on `stream`);
 *    every other requested output is overwritten.  Asynchronous on `stream`, no allocation, no global state.
 *    Kernels (csrc/dcn_bwd.hip): general fp32 kernels for every configuration; for the model's configuration (3x3, stride 1, pad 1,
 *    dilation 1, deformable_group 1, C % 16 == 0, Cout <= 1024) both contractions run on v_mfma_f32_32x32x2_f32 (exact fmaf chains) with the
 *    sampling in the same kernel.  The _general entry point runs the general kernels on every configuration, the model's included.
 *    Reproducibility: grad_offset, grad_mask, grad_weight and grad_bias are sums in a fixed order -- bit-identical from run to run and
 *    whichever other outputs are requested; grad_input is scattered with float atomic adds (the order of the adds varies: last bits differ).
 *    Workspace (device memory, 256-byte aligned), with NPX = B*Ho*Wo, K = C*kh*kw, a256(x) = x rounded up to 256:
 *      general  = a256(4 * Sg * Cout * K), Sg = splits of the pixels for grad_weight: min(max(ceil(512 / (ceil(K/64) ceil(Cout/64))), 1),
 *                 max(NPX/256, 1), 64), then re-derived from the split length rounded up to 16 pixels
 *      model    = a256(4*B*H*W*C) [input in NHWC] + a256(4 * 9 * ceil(C/32) * ceil(Cout/8) * 256) [filters in MFMA operand order]
 *                 + a256(4 * B*SP * 9*Cout*C) [grad_weight partials], SP = splits per image: min(max(ceil(1024 / (ceil(C/32) ceil(Cout/64) B)), 1),
 *                 max(H*W/512, 1)), then re-derived from the split length rounded up to 8 pixels
 *      bytes    = max(general, model) in the model's configuration, general otherwise -- never a [B, 9C, Ho*Wo] column buffer.
 *    The workspace is needed for grad_weight (and, in the model's configuration, for the data gradients); a NULL or short one is
 *    H3D_ERR_ARG.  The size query returns a status like every other entry and hands the size back through `bytes`. */
int h3d_dcn_v2_backward_workspace_bytes(int B, int C, int H, int W, int Cout, int kernel_h, int kernel_w,
                                        int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w,
                                        int deformable_group, size_t *bytes);
int h3d_dcn_v2_backward(const float *input, const float *weight, const float *bias, const float *offset, const float *mask,
                        const float *grad_output,
                        float *grad_input, float *grad_offset, float *grad_mask, float *grad_weight, float *grad_bias,
                        int B, int C, int H, int W, int Cout, int kernel_h, int kernel_w, int stride_h, int stride_w,
                        int pad_h, int pad_w, int dilation_h, int dilation_w, int deformable_group,
                        void *workspace, size_t workspace_bytes, void *stream);
int h3d_dcn_v2_backward_general(const float *input, const float *weight, const float *bias, const float *offset, const float *mask,
                                const float *grad_output,
                                float *grad_input, float *grad_offset, float *grad_mask, float *grad_weight, float *grad_bias,
                                int B, int C, int H, int W, int Cout, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                int pad_h, int pad_w, int dilation_h, int dilation_w, int deformable_group,
                                void *workspace, size_t workspace_bytes, void *stream);

/* The convolution in front of the operator inside the `DCN` module (dcn_v2.py:107-111, 119-124), for ANY module configuration:
 *   out = Conv2d(C, 3*dg*kh*kw, (kh,kw), stride, padding)(input);  o1, o2, m = chunk(out, 3, dim=1)
 *   offset [B,2*dg*kh*kw,Ho,Wo] = cat(o1, o2)    mask [B,dg*kh*kw,Ho,Wo] = sigmoid(m)
 * off_weight [3*dg*kh*kw, C, kh, kw], off_bias [3*dg*kh*kw]; Ho = (H + 2*pad_h - kh) / stride_h + 1 (the reference passes no dilation to
 * this convolution).  Runs the general operator kernel with zero offsets and a unit mask -- no vendor library on any DCN path. */
int h3d_dcn_offset_mask(const float *input, const float *off_weight, const float *off_bias, float *offset, float *mask,
                        int B, int C, int H, int W, int kernel_h, int kernel_w, int stride_h, int stride_w,
                        int pad_h, int pad_w, int deformable_group, void *stream);

/* The same operator with a caller-provided device workspace of h3d_dcn_v2_workspace_bytes(...) bytes (the reference
 * callee allocates its own scratch: `columns`, `ones`, pointer tables, dcn_v2_cuda.cu:90-103).  For the configuration the
 * model uses (model.py:355: 3x3, stride 1, pad 1, dilation 1, deformable_group 1) and C % 16 == 0 the operands are re-laid
 * into the network kernels' layout inside the workspace and the contraction runs on the LDS-apron + MFMA kernel (csrc/dcn2.hip: since
 * round 5 three fp16 MFMAs on split operands per fp32 product, see H3D_DCN_F32_MFMA below); every other configuration (or a NULL / short workspace) takes h3d_dcn_v2_forward's general kernel. */
size_t h3d_dcn_v2_workspace_bytes(int B, int C, int H, int W, int Cout);
int h3d_dcn_v2_forward_ws(const float *input, const float *weight, const float *bias,
                          const float *offset, const float *mask, float *output,
                          int B, int C, int H, int W, int Cout,
                          int kernel_h, int kernel_w, int stride_h, int stride_w,
                          int pad_h, int pad_w, int dilation_h, int dilation_w,
                          int deformable_group, void *workspace, size_t workspace_bytes, void *stream);

/* The operator's THROUGHPUT form: the same contraction with the per-call work of the reference contract taken out.  The filters
 * are packed once (h3d_dcn_v2_pack_weights into h3d_dcn_v2_packed_weight_bytes(...) bytes; `dtype` H3D_F32 = fp32 tensors (split-operand
 * fp16 MFMAs, or exact fmaf chains on the fp32 matrix instruction with H3D_DCN_F32_MFMA), H3D_BF16 = fp16 filters + fp16 blend + f16 MFMA on a bf16 input); `input` is NCHW fp32 as in the
 * reference or, with H3D_DCN_INPUT_NHWC, channels-last [B,H,W,C] of `dtype` (torch.channels_last: no relayout); the output is
 * NCHW fp32 or, with H3D_DCN_OUTPUT_NHWC, channels-last of `dtype`.  offset [B,18,H,W] and mask [B,9,H,W] stay the reference's
 * NCHW fp32 operands.  3x3, stride 1, pad 1, dilation 1, deformable_group 1 (model.py:355), C % 16 == 0.
 * workspace: h3d_dcn_v2_packed_workspace_bytes(B, C, H, W, flags) bytes. */
#define H3D_DCN_INPUT_NHWC 1
#define H3D_DCN_OUTPUT_NHWC 2
#define H3D_DCN_F32_MFMA 4      /* H3D_F32 packs: contract on the fp32 matrix instruction (exact fmaf chains) instead of the default since round 5,
                                   three fp16 MFMAs on split operands per fp32 product (2^-22 relative per product, fp32 accumulation: ~2x the
                                   rate).  The same choice for every fp32 fast-path entry point: environment H3D_DCN_OP_F32=1 */
size_t h3d_dcn_v2_packed_weight_bytes(int Cout, int C, int dtype);
int h3d_dcn_v2_pack_weights(const float *weight, const float *bias, int Cout, int C, int dtype, void *packed, void *stream);
/* h3d_dcn_v2_pack_weights for a pack that is KEPT across calls: validated on the device, without a host synchronisation.  Every
 * call hashes the bytes of weight and bias on `stream`; the pack kernel runs only when the hash differs from the one `packed` was
 * built from (state[0]), so an in-place parameter edit that no host-side version counter sees (`weight.data.zero_()`,
 * DCNv2/test.py:21; dcn_v2.py:80-81) is picked up by the next call, and an unchanged layer costs three tiny launches.
 * state: 16 bytes of device memory, zeroed by the caller when `packed` is allocated, owned by this function afterwards. */
int h3d_dcn_v2_pack_weights_cached(const float *weight, const float *bias, int Cout, int C, int dtype, void *packed, void *state,
                                   void *stream);
/* The four parameters of the stand-alone `DCN` module (dcn_v2.py:97-116; conv_offset_mask has 27 output channels) in the fp32 layout
 * of H3D_OP_DCN_FUSED: wp [rows = Cout padded to 128][9][C], wo [128][9][C] (rows permuted as the op expects), bias_out
 * [rows | 32 | 64]: the biases, then (round 5) 64 floats of which the first two words are the bit patterns of max |weight| and
 * max |off_weight| -- what an H3D_OP_DCN_FUSED of dtype H3D_F16X3 with H3D_OPF_DCN_FUSED_RAW_PACK derives its power-of-two filter scales
 * from (fp32 packs, split while they are staged; float offsets H3D_DCN_FUSED_BIAS_WMAX / _AMAX below); validated on the device like h3d_dcn_v2_pack_weights_cached (state: 16 zeroed bytes). */
int h3d_dcn_fused_pack_f32_cached(const float *weight, const float *bias, const float *off_weight, const float *off_bias, int Cout, int C,
                                  float *wp, float *wo, float *bias_out, void *state, void *stream);
size_t h3d_dcn_v2_packed_workspace_bytes(int B, int C, int H, int W, int flags);
/* Numerics of the fp32 fast path (h3d_dcn_v2_forward_ws, h3d_dcn_v2_forward_packed with H3D_F32) in its default arithmetic (split
 * operands on the fp16 matrix cores): the filters AND the activations are scaled by powers of two the device derives on the caller's
 * stream -- from max |w|, and from S = max |x| * max(1, max |mask|) over the finite elements of this call -- so every output meets
 * |y - y64| <= 2e-6 (A + |b|), A = sum |w| |column| (the fp64 value on |x|, |w|, |mask|), when its SAMPLES (bilinear blend times mask,
 * |blend| * |mask|) lie within 2^-17 of S; below that window -- small inputs, or small masks such as the sigmoid of a strongly negative
 * logit -- the error stays under 4e-7 S sum |w| of the output row.  Any fp32 mask (values outside [0, 1] included).  Non-finite
 * values follow the reference (dcn_v2_im2col_cuda.cu:37-48, 178): a NaN / inf offset gates its tap out, a NaN / inf mask makes its
 * output NaN even when the tap is gated, a NaN / inf pixel makes every output non-finite whose samples read it.
 * DECIDED HERE: a pixel read with bilinear weight zero counts as read, as in the reference; in addition an output (oy, ox) MAY come out
 * non-finite when a non-finite pixel lies in rows oy-1 .. oy+2, columns ox-1 .. ox+2 (a gated or far sample still reads its undeformed
 * tap's 2x2 corners with weight zero).  No NaN becomes a finite number.  H3D_DCN_F32_MFMA follows the same rules with exact fmaf chains.
 * The stand-alone `DCN` module's launch (H3D_OP_DCN_FUSED; f16x3: h3d_dcn_nchw_to_nhwc_scaled -- max |x|, then x scaled by 2^e in the
 * relayout -- and H3D_OPF_DCN_FUSED_RAW_PACK | H3D_OPF_DCN_FUSED_SCALED_INPUT, under which the kernel stages and splits without a clamp) keeps the same rules, its own offset
 * convolution included: a NaN pixel gives NaN offsets and a sigmoid(NaN) mask, and 0 * NaN is NaN. */
int h3d_dcn_nchw_to_nhwc_scaled(const float *src, float *dst, int B, int C, int H, int W, unsigned *amax, void *stream);
int h3d_dcn_v2_forward_packed(const void *input, const void *packed, const float *offset, const float *mask, void *output,
                              int B, int C, int H, int W, int Cout, int dtype, int flags,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Deformable PS-ROI pooling, forward: `_ext.dcn_v2_psroi_pooling_forward` (DCNv2/src/dcn_v2.h:76-107 ->
 * dcn_v2_psroi_pooling_cuda.cu:58-146, 271-341), positional twin plus outputs, shapes and stream (csrc/psroi.hip).
 *   input  [B,C,H,W] fp32 NCHW contiguous     bbox [num_bbox,5] rows (batch, x1, y1, x2, y2) in input-image px
 *   trans  [>= num_bbox, channels_trans, part_size, part_size]; may be NULL when no_trans (channels_trans is then ignored)
 *   output, output_count [num_bbox, output_dim, P, P], P = pooled_size; output_count = number of valid samples (as float)
 * Arithmetic: the reference's, op for op in fp32 (roundf = half away from zero, fmaxf / fminf clamps, corners floor / ceil).
 * Where this library decides (the reference is undefined or wider):
 *   1. fp32 only (the reference also dispatches double).
 *   2. group_size == 1 only (H3D_ERR_UNSUPPORTED): the reference asserts channels == output_dim yet reads channel
 *      (ctop*gs+gh)*gs+gw, past the input for any group_size > 1.
 *   3. output_dim == C (H3D_ERR_SHAPE, "input channels and output channels must equal").
 *   4. without no_trans: channels_trans even >= 2, num_classes = channels_trans / 2 divides output_dim (H3D_ERR_SHAPE); trans may
 *      have more rows than rois.
 *   5. no read out of bounds on any input: a roi whose batch index is not finite or truncates outside [0,B) gives 0 with count 0
 *      (the reference reads out of bounds); non-finite coordinates / translations follow the reference's arithmetic (infinite
 *      samples fail the gate, NaN ones clamp to 0), so outputs stay finite.
 *   num_bbox == 0: nothing is launched.  pooled_size <= 45.  NULL pointers: H3D_ERR_ARG. */
int h3d_dcn_v2_psroi_pooling_forward(const float *input, const float *bbox, const float *trans, float *output, float *output_count,
                                     int B, int C, int H, int W, int num_bbox, int channels_trans, int no_trans, float spatial_scale,
                                     int output_dim, int group_size, int pooled_size, int part_size, int sample_per_part,
                                     float trans_std, void *stream);
/* The second pooling pass of the `DCNPooling` module (dcn_v2.py:266-292) in one launch: offset_mask is the fully-connected output
 * [num_bbox,3,P,P]; channels 0/1 are the translations (no_trans = 0, one class) and the pooled result is multiplied by
 * sigmoid(channel 2) -- chunk + cat + sigmoid + pool + mul.  part_size == pooled_size; no count output; otherwise as above. */
int h3d_dcn_pooling_modulated(const float *input, const float *bbox, const float *offset_mask, float *output, int B, int C, int H,
                              int W, int num_bbox, float spatial_scale, int output_dim, int group_size, int pooled_size, int part_size,
                              int sample_per_part, float trans_std, void *stream);
/* Deformable PS-ROI pooling, backward: `_ext.dcn_v2_psroi_pooling_backward` (DCNv2/src/dcn_v2.h:109-142 ->
 * dcn_v2_psroi_pooling_cuda.cu:148-269, 343-419), positional twin plus outputs, shapes and stream (csrc/psroi_bwd.hip).
 *   grad_output, output_count [num_bbox, output_dim, P, P]: an element with output_count <= 0 is skipped, the others contribute
 *   grad_output / output_count per valid sample; the sample geometry is the forward's (csrc/psroi_geom.h), exactly
 *   grad_input  [B,C,H,W]: zeroed on `stream`, then a scatter by float atomics (the order of the adds is not fixed)
 *   grad_trans  [num_trans >= num_bbox, channels_trans, part_size, part_size]: zeroed on `stream` (rows beyond num_bbox stay zero);
 *               summed without atomics in an order that depends on the shapes and the geometry only (not on force_direct, nor on
 *               whether grad_input is wanted): bit-identical from run to run
 *   grad_input or grad_trans may be NULL: not computed (grad_trans is ignored when no_trans).  force_direct != 0: every grad_input
 *   contribution is one global atomic (the reference's form) instead of being combined per workgroup in LDS first.
 * Arguments are checked as in the forward, with its texts; a roi with an invalid batch index contributes nothing; num_bbox == 0: the
 * outputs are zeroed and nothing is launched. */
int h3d_dcn_v2_psroi_pooling_backward(const float *grad_output, const float *input, const float *bbox, const float *trans,
                                      const float *output_count, float *grad_input, float *grad_trans, int B, int C, int H, int W,
                                      int num_bbox, int num_trans, int channels_trans, int no_trans, float spatial_scale, int output_dim,
                                      int group_size, int pooled_size, int part_size, int sample_per_part, float trans_std,
                                      int force_direct, void *stream);
/* Backward of h3d_dcn_pooling_modulated: grad_offset_mask [num_bbox,3,P,P] = the translation gradients (channels 0/1) and the
 * gradient of the mask logit m (channel 2), s (1 - s) * sum_c grad_output * pooled with s = sigmoid(m) and pooled the unmasked mean;
 * the upstream of a pooled element is grad_output * s and the count per bin is recomputed.  Same order rules as above. */
int h3d_dcn_pooling_modulated_backward(const float *grad_output, const float *input, const float *bbox, const float *offset_mask,
                                       float *grad_input, float *grad_offset_mask, int B, int C, int H, int W, int num_bbox,
                                       float spatial_scale, int output_dim, int group_size, int pooled_size, int part_size,
                                       int sample_per_part, float trans_std, int force_direct, void *stream);
/* Which grad_input path the backward takes for ONE (roi, class): a function of the geometry alone, computed on the host by the code the
 * kernel runs.  roi = 5 floats, trans_row = that roi's [channels_trans, part_size, part_size] translations (HOST pointers; an
 * [3,P,P] offset_mask row with channels_trans = 2 in modulated mode).  *path = 0: nothing to add (invalid batch index, or no valid
 * sample), 1: combined in LDS, one global atomic per touched pixel, 2: one global atomic per sample corner. */
int h3d_psroi_backward_path(const float *roi, const float *trans_row, int B, int C, int H, int W, int channels_trans, int no_trans,
                            float spatial_scale, int pooled_size, int part_size, int sample_per_part, float trans_std, int class_id,
                            int force_direct, int *path);

/* =====================================================================================
 * 2. Network ops (DLA-34 + DLAUp/IDAUp + heads, model.py:32-61,148-222,286-292,346-415,475-489)
 *    on the internal layout: activations NHWC (channels-last) of element type f32 or bf16,
 *    addressed as (pointer, channel stride) so a tensor can live inside a wider concat buffer
 *    (Root's torch.cat, model.py:160, costs nothing).  Weights are pre-packed by the host:
 *      conv   : [rows = Cout padded to 128][kh*kw][Cin] elements, BatchNorm folded in,
 *               bias fp32[rows]
 *    One descriptor per launch; h3d_run_ops walks an array of them (the forward "plan").
 * ===================================================================================== */
enum {
    H3D_OP_STEM = 1,    /* base_layer 7x7 3->C0 conv+BN+ReLU from NCHW fp32 images (model.py:231-235): stride 1, C0 = 16;
                           bf16 plans also stride 2 with C0 a multiple of 16 (the stems of ResNet-101-DCN / Hourglass-104):
                           w = bf16 [C0][7][32], k = dx*4 + c, zero for dx = 7 and c = 3 */
    H3D_OP_CONV = 2,    /* kxk (k=1|3, stride 1|2, pad k/2) conv + bias [+residual] [+ReLU]            */
    H3D_OP_DCN = 3,     /* modulated deformable 3x3 s1 p1 d1 dg1 conv + bias [+ReLU] (model.py:346-362);
                           weights [rows][9][Cin] are fp16 when dtype = bf16 (csrc/dcn2.hip), fp32 otherwise */
    H3D_OP_MAXPOOL = 4, /* 2x2 stride-2 max pool (Tree.downsample, model.py:200-201)                   */
    H3D_OP_UPADD = 5,   /* depthwise ConvTranspose2d(k=2f,s=f,p=f/2) + skip add (IDAUp, model.py:375-390) */
    H3D_OP_COPY = 6,    /* strided NHWC copy (y[i] = x[i].clone(), model.py:480-482)                   */
    H3D_OP_DCN_FUSED = 9, /* DeformConv with conv_offset_mask fused in (csrc/dcn3.hip): in2 = offset/mask filters
                             [32 permuted rows][9][Cin] (same element type as w), bias = [wrows main | 32 offset] */
    H3D_OP_CONV_STREAM = 10, /* 3x3 p1 conv, stride 1 or 2 (bf16), fed by LDS-DMA (csrc/conv2.hip): w = stage-major filter image
                                [Cin/16][wrows/32][32 rows][19 slots of 8 elements]: slot 2*tap+h = input channels
                                16*stage + 8h..8h+7 of tap `tap`, slot 18 zero; in2 = optional residual    */
    H3D_OP_DCN_FUSED_F16 = 11, /* H3D_OP_DCN_FUSED for a 64-channel fp16 input, Cout <= 64 (csrc/dcn4.hip): w and in2 are
                                  stage-major fp16 filter images [4][wrows/32 | 1][32][19][8] (layout of H3D_OP_CONV_STREAM) */
    H3D_OP_DCN_FUSED_STREAM = 12, /* H3D_OP_DCN_FUSED (bf16 input) with w / in2 as stage-major fp16 filter images of
                                     CK = h3d_dcn_fused_ck(Cin, Cout) channels per stage: [Cin/CK][wrows/32 | 1][32 rows]
                                     [9*CK/8 + 1 slots][8]: slot tap*CK/8 + j = channels CK*stage + 8j.. of tap `tap` */
    H3D_OP_STEM3 = 13,  /* base_layer + level0 + level1 fused (bf16, csrc/stem3.hip): in = NCHW fp32 images, out = level1 map
                           [B,Ho,Wo,32]; w = bf16 [16][7][32] stem (k = dx*4+c) | [5][16][32] level0 (k = (tap&1)*16+c of tap pair)
                           | [32][9][16] level1; bias = fp32 [16 | 16 | 32]; Cin = 3, Cout = 32.
                           in2 != NULL (round 4): ALSO level2's residual branch, project(max_pool2x2(level1)) (Tree.downsample + Tree.project,
                           model.py:200-207): in2 = that OUTPUT map [B,Ho/2,Wo/2,in2_cs] (64 channels, no ReLU); w continues with the 1x1
                           filters [64][32], bias with their 64 values; Ho, Wo even                                            */
    H3D_OP_DCN_V1 = 8,  /* first-generation DCN kernel (global gather, bf16 weights): kept as an A/B reference */
    H3D_OP_UPDCN_F16 = 14, /* IDAUp's node(up(x) + skip) in one launch (model.py:384-390): depthwise ConvTranspose2d (k = 2f,
                           stride f in {2, 4}) + skip add evaluated while the DeformConv's input tile is staged, then
                           DCN_FUSED_F16's kernel.  in = x at the LOW resolution H x W, Ho x Wo = f * (H x W), stride = f,
                           in2 = HOST pointer to h3d_updcn_desc; bf16 plans, 64 channels                               */
    /* ops of the other backbones (BASELINE configs 4, 5: Hourglass-104, ResNet-101-DCN; csrc/extra.hip) */
    H3D_OP_IM2COL = 15,      /* 7x7 stride-2 pad-3 stem conv as im2col: in = NCHW fp32 images [B,Cin,H,W] -> out [B,Ho,Wo,Cout] patches,
                                channel k = c*ks*ks + ky*ks + kx, zero from Cin*ks*ks up to Cout (a multiple of 16): feeds a 1x1 H3D_OP_CONV */
    H3D_OP_MAXPOOL3 = 16,    /* nn.MaxPool2d(3, stride 2, padding 1): Ho = (H-1)/2+1                                        */
    H3D_OP_DEPTH2SPACE = 17, /* [B,H,W,4*Cout] -> [B,2H,2W,Cout]: channel group 2*py+px -> output pixel (2y+py, 2x+px)        */
    H3D_OP_HEADS = 7    /* all output heads fused: Conv3x3(64->head_conv)+ReLU+Conv1x1(->C) per head
                           (model.py:451-460, 485-489); in2 = HOST pointer to h3d_heads_desc          */
};

/* H3D_OP_HEADS: op.in = y (NHWC, 64 ch), op.w = packed 3x3 weights of all heads
 * [nheads*head_conv][9][64], op.bias = fp32 [nheads*head_conv], op.Cout = head_conv,
 * op.in2 = host pointer to this descriptor.  w2: [96 rows][head_conv] elements with K in MFMA
 * accumulator-row order (h3d_amd/engine.py: pack_head_1x1), b2: fp32 [96], out: NCHW fp32. */
#define H3D_HEADS_MAX 16
typedef struct h3d_heads_desc {
    int32_t nheads;
    int32_t wexp;       /* H3D_F16X3: op.w holds 2^wexp times the 3x3 filters AND op.bias 2^wexp times their biases (h3d_op.wexp) */
    struct {
        const void *w2;
        const float *b2;
        float *out;
        int32_t C;
        int32_t wexp2;  /* H3D_F16X3: w2 holds 2^wexp2 times the 1x1 filters (b2 is unscaled) */
    } head[H3D_HEADS_MAX];
} h3d_heads_desc;
/* H3D_OP_UPDCN_F16: the operands that do not fit h3d_op */
typedef struct h3d_updcn_desc {
    const void *skip;    /* bf16 NHWC [B][Ho][Wo][skip_cs]: layers[i-1]                         */
    const float *w_up;   /* fp32 [k*k][64] tap-major transposed-convolution weights (as UPADD)  */
    const void *w_off;   /* offset/mask filter image (as DCN_FUSED_F16's in2)                   */
    int32_t skip_cs;
    int32_t reserved;
} h3d_updcn_desc;
enum { H3D_OUT_NHWC = 0, H3D_OUT_NCHW_F32 = 1, H3D_OUT_NHWC_F32 = 2,
       H3D_OUT_NHWC_F16 = 3 /* H3D_OP_UPADD in a bf16 plan only: fp16 output, the input of H3D_OP_DCN_FUSED_F16 */ };

typedef struct h3d_op {
    int32_t kind;       /* H3D_OP_*                                                        */
    int32_t dtype;      /* H3D_F32 | H3D_BF16: activation + weight element type           */
    const void *in;     /* input activations (STEM: NCHW fp32 images)                      */
    const void *in2;    /* CONV: residual (or NULL); UPADD: skip tensor; DCN: offset/mask  */
    const void *w;      /* packed weights (UPADD: fp32 [C][k*k])                           */
    const float *bias;  /* fp32 [rows] (NULL for POOL/UPADD/COPY)                          */
    void *out;
    int32_t B, H, W;    /* input batch / height / width                                    */
    int32_t Cin, in_cs; /* input channels, input channel stride (elements per pixel)       */
    int32_t in2_cs;     /* channel stride of in2 (DCN: floats per pixel of offset/mask, >=27) */
    int32_t Ho, Wo;     /* output height / width                                           */
    int32_t Cout, out_cs;
    int32_t ksize;      /* CONV: 1|3; STEM: 7; UPADD: 2f                                   */
    int32_t stride;     /* CONV: 1|2; UPADD: f                                             */
    int32_t relu;       /* 1: ReLU epilogue                                                */
    int32_t out_mode;   /* H3D_OUT_*                                                       */
    int32_t wrows;      /* rows of the packed weight buffer (>= Cout, multiple of 128)     */
    int32_t reserved;   /* per-kind flag word: H3D_OPF_* (operand / plan flags, set in production) | H3D_TUNE_* (tuning overrides of
                           tests and tools/, ablation bits of `make ABLATE=1` builds) -- the catalogue below.  0 = the defaults;
                           a bit no name covers for the op's kind and dtype is ignored                     */
    int32_t wexp;       /* H3D_F16X3 plans (ABI 2): the packed filters hold 2^wexp times the layer's filters -- chosen by the packer so
                           that max |w| lands in [2^13, 2^14) and the lo terms of all but vanishing filters are NORMAL fp16 numbers
                           (an unscaled 0.05 has a subnormal lo term: 3e-8 absolute, 2^-20.7 relative, five times the 2^-23 of the
                           split itself) -- and the kernel multiplies its accumulators by 2^-wexp (exact) before the bias.  0 elsewhere */
    int32_t wexp2;      /* ... the same for the offset / mask filters of H3D_OP_DCN_FUSED (in2)                */
} h3d_op;

/* ---- h3d_op.reserved: the flag catalogue ------------------------------------------------------------------------------------------
 * One enum per op kind (and dtype class where the launcher reads the word differently).  Two families:
 *   H3D_OPF_<GROUP>_<NAME>   operand / plan flags: production sets them (engine.py's plans, the operator boundary of csrc/dcn.hip,
 *                            dcn_v2.py).  Several change what the kernel READS: the buffer contract is stated with the flag, and a caller
 *                            who sets one over buffers that do not meet it reads out of bounds.
 *   H3D_TUNE_<GROUP>_<NAME>  tuning overrides: tests/ and tools/ set them to force an instantiation the launcher's rule would not pick
 *                            (same operands, same result up to the summation order).  ..._ABLATE_MASK = the bits a `make ABLATE=1` build
 *                            hands to the kernel's profiling switches (wrong results, timing only); every other build ignores them.
 * One bit value may carry different names in different groups; a group's names only mean anything for that kind and dtype.
 * Function-like macros build / take apart the multi-bit fields.  Kinds not listed read nothing from the word, with one exception:
 * H3D_OP_STEM3 in an ABLATE build takes the whole word as a phase number (1 .. 3: return after that phase). */

/* H3D_DCN_AUX_BYTES: what an fp32 DeformConv filter pack carries behind its [rows] fp32 biases (h3d_dcn_v2_pack_weights with H3D_F32,
 * counted in h3d_dcn_v2_packed_weight_bytes / h3d_dcn_v2_workspace_bytes): word 0 = bit pattern of max |filter|, the rest zero.
 * The packer zeroes and fills it on the caller's stream. */
#define H3D_DCN_AUX_BYTES 256
/* bias_out of h3d_dcn_fused_pack_f32_cached is [rows | 32 | 64] floats; float offsets behind `rows` (= op.wrows) of the 64-float tail: */
#define H3D_DCN_FUSED_BIAS_WMAX 32   /* [+0] bits of max |weight|, [+1] bits of max |off_weight|: written by the packer                       */
#define H3D_DCN_FUSED_BIAS_AMAX 34   /* bits of max |x| over the finite input elements: written by h3d_dcn_nchw_to_nhwc_scaled (its `amax`) */

/* H3D_OP_DCN (csrc/dcn2.hip), every dtype */
enum {
    H3D_OPF_DCN_MASK_FINAL = 0x800,       /* in2 channels 18..26 hold the mask itself, not its logit (the operator boundary: the reference applies
                                             the sigmoid in DCN.forward, dcn_v2.py:124).  No buffer requirement                                */
    H3D_OPF_DCN_RAW_PACK = 0x100000,      /* H3D_F16X3 only (without it an f16x3 H3D_OP_DCN has no kernel): w is the plain fp32 pack [wrows][9][Cin]
                                             of H3D_F32, and bias must extend to [wrows] floats + H3D_DCN_AUX_BYTES: the kernel reads the bit pattern
                                             of max |w| at bias[wrows] and scales / splits the filters while it stages them.  wexp must be 0      */
    H3D_OPF_DCN_ACT_MAXIMA = 0x200000,    /* with RAW_PACK only: in2 must extend 16 bytes past its B*H*W*in2_cs floats; the two words there are
                                             the bit patterns of max |x| and max |mask| over the finite elements (the caller zeroes them, then
                                             fills them on the same stream: csrc/dcn.hip dcn_om_pack); the kernel scales the activations by them */
    H3D_TUNE_DCN_ABLATE_MASK = 0x1f       /* 2 no gather / blend, 4 no MFMA, 8 no slow path, 16 zero offsets                                     */
};

/* H3D_OP_DCN_FUSED (csrc/dcn3.hip), dtype H3D_F16X3 */
enum {
    H3D_OPF_DCN_FUSED_RAW_PACK = 0x100000,     /* w / in2 are the plain fp32 packs of h3d_dcn_fused_pack_f32_cached and bias its bias_out: [wrows | 32 |
                                                  64] floats, of which the kernel reads the two filter maxima at bias[wrows + H3D_DCN_FUSED_BIAS_WMAX]
                                                  and [+ 1].  A [wrows | 32] bias buffer is too short.  wexp and wexp2 must be 0                  */
    H3D_OPF_DCN_FUSED_SCALED_INPUT = 0x200000, /* with RAW_PACK only: `in` was scaled by h3d_dcn_nchw_to_nhwc_scaled, whose amax word is
                                                  bias[wrows + H3D_DCN_FUSED_BIAS_AMAX]; the kernel reads it and divides the scale out again      */
    H3D_TUNE_DCN_FUSED_X3_MARGIN2 = 0x2000,    /* the f32 plan's margin-2 double-buffered tile                                                  */
    H3D_TUNE_DCN_FUSED_X3_MARGIN6 = 0x4000,    /* force the margin-6 apron (default: Cout <= 64 on maps of 64 rows or more)                     */
    H3D_TUNE_DCN_FUSED_X3_MARGIN4 = 0x8000,    /* force the margin-4 apron; wins over MARGIN6, loses to MARGIN2                                  */
    H3D_TUNE_DCN_FUSED_X3_ABLATE_MASK = 0x1f   /* as H3D_TUNE_DCN_STREAM_ABLATE_MASK                                                             */
};

/* H3D_OP_DCN_FUSED_STREAM and H3D_OP_DCN_FUSED (csrc/dcn3.hip), the 2-byte dtypes H3D_BF16 / H3D_F16.  The variant flags select tiles of
 * H3D_OP_DCN_FUSED_STREAM; of an H3D_OP_DCN_FUSED the launcher reads FORCE_NARROW_WG / FORCE_WIDE_WG, and rejects F16_INPUT.  No flag
 * of this group changes what the buffers must hold except F16_INPUT. */
enum {
    H3D_OPF_DCN_STREAM_NO_SLOTS = 0x1000,      /* round 1's tiles without patch slots: every sample outside the apron goes through pass 2 (what a
                                                  layer with Cin % 32 != 0 gets anyway).  Overrides the three variant flags below                */
    H3D_OPF_DCN_STREAM_WIDE_MARGIN = 0x8000,   /* margin-4 tile on the packed apron, 256 patch slots (layers whose offsets reach far:
                                                  DLAEngine.calibrate_dcn_margins).  Wins over SLOTS512                                          */
    H3D_OPF_DCN_STREAM_SLOTS512 = 0x10000,     /* margin 2 on the packed apron, 512 patch slots per tile                                         */
    H3D_OPF_DCN_STREAM_F16_INPUT = 0x40000,    /* H3D_BF16 plans: `in` holds IEEE fp16 values, not bf16 (an H3D_OP_UPADD with H3D_OUT_NHWC_F16 wrote it).
                                                  Exists for the patch-slot tiles with Cin % 32 == 0, Cout > 32, NHWC output with Cout % 8 == 0;
                                                  H3D_ERR_UNSUPPORTED elsewhere                                                                  */
    H3D_OPF_DCN_STREAM_STATS = 0x20000,        /* set by h3d_dcn_far_samples on its private copy of the op, not by callers: a patch-slot tile that
                                                  carries it runs phase A + geometry only and writes per-tile int32 counters to `out`             */
    H3D_OPF_DCN_STREAM_VARIANT_MASK = 0x58600, /* what h3d_dcn_far_samples keeps of the caller's word: WIDE_MARGIN | SLOTS512 | F16_INPUT |
                                                  FORCE_NARROW_WG | FORCE_WIDE_WG -- the bits that select the tile whose apron it measures        */
    H3D_TUNE_DCN_STREAM_FORCE_NARROW_WG = 0x200, /* Cout > 64: 64-channel workgroups whatever the grid (default: below 192 128-channel workgroups)   */
    H3D_TUNE_DCN_STREAM_FORCE_WIDE_WG = 0x400,   /* Cout > 64: 128-channel workgroups whatever the grid; wins over FORCE_NARROW_WG                   */
    H3D_TUNE_DCN_STREAM_F16_DCN5 = 0x4000,     /* H3D_F16 stream ops: the LDS-DMA apron kernel of csrc/dcn5.hip (`make EXTRA=1` builds; H3D_ERR_UNSUPPORTED
                                                  otherwise), unless NO_SLOTS or F16_KEEP_DCN3 is set                                             */
    H3D_TUNE_DCN_STREAM_F16_KEEP_DCN3 = 0x2000, /* with F16_DCN5: stay on csrc/dcn3.hip                                                          */
    H3D_TUNE_DCN_STREAM_ABLATE_MASK = 0x1f     /* dcn3: 1 no phase-A MFMA, 2 no gather / blend, 4 no phase-B MFMA, 8 stage once, 16 no patch fill  */
};
/* ... under F16_DCN5 bits 16..23 are the dcn5 experiment number instead (tools/ab_dcn5.py; <= 64 output channels) */
#define H3D_TUNE_DCN_STREAM_DCN5_XP(xp) ((xp) << 16)
#define H3D_TUNE_DCN_STREAM_DCN5_XP_OF(reserved) (((reserved) >> 16) & 0xff)

/* H3D_OP_DCN_FUSED_STREAM (csrc/dcn3.hip), dtype H3D_F16X3: the apron margin (default 4 for Cin == Cout > 64, else 2) */
enum {
    H3D_TUNE_DCN_STREAM_X3_MARGIN2 = 0x4000,   /* MARGIN2 wins over MARGIN3 and MARGIN4, MARGIN3 over MARGIN4                                    */
    H3D_TUNE_DCN_STREAM_X3_MARGIN3 = 0x8000,
    H3D_TUNE_DCN_STREAM_X3_MARGIN4 = 0x10000,
    H3D_TUNE_DCN_STREAM_X3_ABLATE_MASK = 0x1f
};

/* H3D_OP_DCN_FUSED_F16 and H3D_OP_UPDCN_F16 (csrc/dcn4.hip) */
enum {
    H3D_TUNE_DCN_F16_ONE_WG_PER_CU = 0x100,    /* H3D_OP_DCN_FUSED_F16 only                                                                      */
    H3D_TUNE_DCN_F16_ABLATE_MASK = 0xff        /* a phase number 1 .. 4: return after that phase                                                */
};

/* H3D_OP_CONV_STREAM (csrc/conv2.hip).  The low 16 bits are a tile code, variant << 12 | MT << 8 | WAVES (MT = 32-channel row tiles per
 * workgroup, WAVES = waves per workgroup).  Stride 1 variants: 0 two ring slots, 2 two N-tiles per wave, 3 three ring slots, 5 one ring
 * slot, 6 fragment reads one tap ahead; an unknown code is H3D_ERR_ARG.  Stride 2 knows (4, 4, 4), (4, 4, 8), (4, 2, 4) = one ring slot
 * and (2, 4, 4) = two ring slots, and ignores every other code. */
#define H3D_TUNE_CONV_STREAM_TILE(variant, mt, waves) ((variant) << 12 | (mt) << 8 | (waves))
#define H3D_TUNE_CONV_STREAM_ABLATE(bits) ((bits) << 16)
#define H3D_TUNE_CONV_STREAM_ABLATE_OF(reserved) (((reserved) & H3D_TUNE_CONV_STREAM_ABLATE_MASK) >> 16)
enum {
    H3D_TUNE_CONV_STREAM_TILE_MASK = 0xffff,
    H3D_TUNE_CONV_STREAM_AUTO = 1,             /* tile code "the launcher's own choice": carries ablation bits without an override               */
    H3D_TUNE_CONV_STREAM_ROUND4_RULE = 0x10000000, /* stride 1, Cout > 96 on a small grid: round 4's 128-channel 4-wave tiles instead of narrower blocks */
    H3D_TUNE_CONV_STREAM_ABLATE_MASK = 0x1f0000 /* << 16: 1 no DMA after stage 0, 2 no fragment reads / MFMA, 4 no LDS-transposed epilogue, 8 no
                                                  input DMA, 16 no filter DMA                                                                   */
};

/* H3D_OP_CONV (csrc/conv.hip, csrc/gemm1.hip), the 2-byte dtypes.  A 1x1 conv goes to the GEMM kernel where its shape rule (csrc/gemm1.hip) takes it. */
#define H3D_TUNE_CONV_1X1_TILE(mt, th) (H3D_TUNE_CONV_TILE | (mt) << 4 | (th) >> 3)   /* mt in {2, 4}, th in {8, 16} rows; other pairs: ignored */
#define H3D_TUNE_CONV_1X1_TILE_MT(reserved) (((reserved) >> 4) & 15)
#define H3D_TUNE_CONV_1X1_TILE_TH(reserved) (((reserved) & 15) * 8)
#define H3D_TUNE_CONV_GEMM_TILE(n) ((n) << 8)   /* 1: 256 x 256, 8 waves, two slots; 2: 128 x 128, 8 waves, three slots; 3: 128 x 128, 4 waves, two
                                                   workgroups per CU; others: the launcher's rule                                               */
enum {
    H3D_TUNE_CONV_TILE = 0x1000,               /* 1x1 stride 1, Cin % 64 == 0, Cout > 32: the halo-tile kernel with the tile of H3D_TUNE_CONV_1X1_TILE.
                                                  engine.py sets it on the Root convs of the plans that keep them off the GEMM kernel          */
    H3D_TUNE_CONV_HALO_TILE = 0x2000,          /* 1x1: the halo-tile kernel of csrc/conv.hip (its own tile rule), not the GEMM kernel             */
    H3D_TUNE_CONV_FORCE_GEMM = 0x4000,         /* 1x1: the GEMM kernel whatever the shape (where its layout conditions hold); loses to the two above */
    H3D_TUNE_CONV_GEMM_TILE_MASK = 0xf00
};
/* H3D_OP_CONV, dtype H3D_F16X3 */
#define H3D_TUNE_CONV_X3_TILE(mt, waves, th) (H3D_TUNE_CONV_X3_TILED | (mt) << 8 | (waves) << 4 | (th) >> 3)   /* 3x3; unknown: H3D_ERR_ARG */
enum {
    H3D_TUNE_CONV_X3_TILED = 0x1000,           /* 3x3: the low 12 bits are a tile, see H3D_TUNE_CONV_X3_TILE                                      */
    H3D_TUNE_CONV_X3_TILE_MASK = 0x1fff,
    H3D_TUNE_CONV_X3_CK16 = 0x2000,            /* 1x1 stride 1: 16-channel chunks where 64-channel ones would be used                            */
    H3D_TUNE_CONV_X3_MT2 = 0x4000              /* 1x1 stride 1: 64-channel tiles above 64 output channels too                                    */
};

/* H3D_OP_UPADD (csrc/conv.hip): the word without H3D_OPF_UPADD_FOLDED, compared for equality */
enum {
    H3D_TUNE_UPADD_TAPS_GLOBAL = 1,            /* tap table read from global memory                                                              */
    H3D_TUNE_UPADD_TAPS_LDS = 2,               /* tap table in LDS whenever it fits 64 KiB                                                       */
    H3D_OPF_UPADD_FOLDED = 0x100               /* the plan's claim that nothing but this op reads `in2`.  h3d_run_ops / h3d_run_ops_timed then launch an
                                                  H3D_OP_DCN_FUSED_STREAM op that stands directly in front of this one, and whose `out` is this op's
                                                  `in2`, together with it as ONE kernel where the DeformConv's tile can (2-byte plans, the patch-slot
                                                  tiles of 64-channel workgroups with the LDS-transposed epilogue, f a power of two): that kernel adds
                                                  the up-sampled `in` to every vector it would have stored and writes the sum to this op's `out`; `in2`
                                                  is then NOT written.  The same bits in `out` as the two launches.  Anywhere else the flag is
                                                  ignored, and the timed run reports the pair's time under the DeformConv op and 0 under this one    */
};

/* H3D_OP_MAXPOOL, H3D_OP_CONV and H3D_OP_CONV_STREAM, the 2-byte dtypes: the entry of a DLA Tree (Tree.forward, model.py:209-218) as one launch */
enum {
    H3D_OPF_TREE_ENTRY = 0x20000000,           /* on three ops in a row -- the 2x2 H3D_OP_MAXPOOL of x, the 1x1 H3D_OP_CONV (`project`: no residual, no ReLU)
                                                  that reads exactly the pool's `out`, and the 3x3 stride-2 H3D_OP_CONV_STREAM that reads exactly the pool's
                                                  `in`, H and W even, both convs with the same Cout >= 64, the 3x3 conv on a one-slot tile (its launcher's
                                                  choice from 128 channels on; below that the op also carries H3D_TUNE_CONV_STREAM_TILE(4, 2, 4)) --:
                                                  h3d_run_ops / h3d_run_ops_timed launch them as ONE kernel (csrc/conv2.hip ENTRY: the pool is the maximum of
                                                  four taps the conv holds anyway, `project` one more MFMA chain per stage).  The same bits in all three outputs as the three launches.  Where the
                                                  structure or the tile's conditions do not hold the flag is ignored, on a single op always; the timed run
                                                  reports the launch under the pool op and 0 under the two convs                                      */
    H3D_OPF_TREE_ENTRY_PRIVATE_POOL = 0x40000000 /* on the H3D_OP_MAXPOOL of such a triple: the plan's claim that nothing but the 1x1 conv reads the pooled
                                                  map.  The one launch then does NOT write the pool's `out`                                          */
};

/* H3D_OP_HEADS (csrc/heads.hip) */
enum {
    H3D_TUNE_HEADS_SEPARATE_BIAS = 0x200,      /* separate bias / zeroing pass (launches of equal-width heads only)                              */
    H3D_TUNE_HEADS_SPARSE_LDS_PATCH = 0x400,   /* h3d_heads_sparse*: the neighbourhoods as LDS patches, 64 positions per workgroup, a list's heads in
                                                  series (default: as register fragments, one head per workgroup); the same bits either way        */
    H3D_TUNE_HEADS_SPARSE_WAVES4 = 0x800,      /* h3d_heads_sparse*, register path: 4 waves = 128 positions per workgroup (default: 8 waves = 256)   */
    H3D_TUNE_HEADS_ABLATE_MASK = 0xff          /* 1 no weight loads after the prologue, 2 no stage barrier, 4 / 8 one wave per SIMD, 64 per-wave stamps */
};
/* ---- end of the flag catalogue ---- */

/* channels per filter stage H3D_OP_DCN_FUSED_STREAM expects for a layer (16) */
int h3d_dcn_fused_ck(int Cin, int Cout);

/* How far a fused DeformConv's samples reach, as the kernel itself sees it: per_tile[b * tiles_y * tiles_x + ty * tiles_x + tx]
 * (tiles of 16x16 output pixels, tiles_x = ceil(W/16)) = the number of (pixel, tap) samples of that tile that lie inside the image
 * but have a bilinear corner outside the tile's LDS apron, for the tile variant `op->reserved` selects: of the caller's word
 * H3D_OPF_DCN_STREAM_VARIANT_MASK is kept (margin 2, H3D_OPF_DCN_STREAM_WIDE_MARGIN or _SLOTS512, fp16 input, workgroup width), every
 * other bit is dropped; a word with H3D_OPF_DCN_STREAM_NO_SLOTS is H3D_ERR_UNSUPPORTED.  Phase A + geometry of the production kernel run, nothing else; op->out is not written.  A deterministic function of
 * the layer's input: DLAEngine.calibrate_dcn_margins derives the per-layer variant from these counts (the reference operator,
 * dcn_v2_cuda.cu:43-173, has no data-dependent dispatch at all, so whatever replaces it must not depend on a stopwatch). */
int h3d_dcn_far_samples(const h3d_op *op, int32_t *per_tile, void *stream);

/* Launch ops[0..n) in order on `stream`.  Returns H3D_OK or the first error (index in the
 * message). */
int h3d_run_ops(const h3d_op *ops, int n, void *stream);

/* Same, with a HIP event pair around every op: ms[i] = device time of ops[i] (bench.py's
 * live roofline measurement; events are recorded on `stream`). Synchronises the stream. */
int h3d_run_ops_timed(const h3d_op *ops, int n, void *stream, float *ms);
/* Name of the kernel instantiation `op` dispatches to, as rocprofv3 prints it
 * (e.g. "conv_kernel<unsigned short, 3, 1, 2, 32, 16>"); nothing is launched. */
int h3d_op_kernel_name(const h3d_op *op, char *buf, int buflen);

/* The heads of ONE H3D_OP_HEADS op (H3D_BF16 / H3D_F16; reserved = 0 or H3D_TUNE_HEADS_SPARSE_*) at listed positions only (csrc/heads.hip): inds = [B][K]
 * flat output positions y*W + x (multi_pose_decode's top-K centres).  Every head of the op's descriptor is evaluated at each
 * listed position and written into the head's dense NCHW fp32 map there; no other element is written.  The value is bit for bit
 * what h3d_run_ops writes at that position (same operands, same order of every accumulation).  An entry outside [0, H*W) is
 * skipped; a position may be listed more than once. */
int h3d_heads_sparse(const h3d_op *op, const int64_t *inds, int K, void *stream);

/* The same in ONE launch over several position lists, each with its own heads: list i evaluates the heads whose descriptor slot is
 * set in head_mask at inds [B][K] (h3d_heads_sparse is the one-list, all-heads case).  multi_pose_decode reads `hp_offset` at the
 * 17 x K key-point peaks and every other gathered head at the K centres: two lists, one launch in the serial tail of the step.
 * A workgroup takes its positions from one list and runs ONE head of that list (with H3D_TUNE_HEADS_SPARSE_LDS_PATCH: all of them
 * in series); the lists with the most heads are scheduled first, in a list the widest heads.  A position may appear in several
 * lists and more than once in a list (the same bits are stored again); an entry outside [0, H*W) stores nothing.  A head that no
 * list names is not computed.  A feature map of 2 GiB or more (((B*H*W - 1) * in_cs + 64) elements) takes the
 * H3D_TUNE_HEADS_SPARSE_LDS_PATCH kernel whatever op.reserved says: the default kernel addresses the map by 32-bit buffer offsets.
 * The values are the same on either path.
 *    H3D_ERR_ARG: nlists outside 1..H3D_HEADS_LISTS_MAX, a NULL list, an empty mask, a mask bit at or beyond the descriptor's
 *    nheads, a head named by two lists.  Per list, as h3d_heads_sparse: K <= 0 or B*K > 2^24 is H3D_ERR_SHAPE; a dtype other than
 *    H3D_BF16 / H3D_F16 or a bit of op.reserved other than H3D_TUNE_HEADS_SPARSE_LDS_PATCH / _WAVES4 is H3D_ERR_UNSUPPORTED. */
#define H3D_HEADS_LISTS_MAX 4
typedef struct h3d_heads_list {
    const int64_t *inds;    /* device, [B][K] */
    int32_t K;
    uint32_t head_mask;     /* bit i: head[i] of the op's h3d_heads_desc */
} h3d_heads_list;
int h3d_heads_sparse_lists(const h3d_op *op, int nlists, const h3d_heads_list *lists, void *stream);

/* Layout helpers (host interface keeps the reference's NCHW fp32 tensors at the boundary). */
int h3d_nchw_f32_to_nhwc(const float *src, void *dst, int dtype, int B, int C, int H, int W,
                         int dst_cs, void *stream);
int h3d_nhwc_to_nchw_f32(const void *src, int dtype, float *dst, int B, int C, int H, int W,
                         int src_cs, void *stream);

/* =====================================================================================
 * 2b. Heads backward (csrc/heads_bwd.hip): the gradients of H3D_OP_HEADS' operator, per head
 *         z = W2 relu(conv3x3(y, W1) + b1) + b2          (model.py:451-464, 485-489)
 *    at W1, b1, W2, b2 and at the feature map y (summed over the heads, in head order).  ReLU gradient 0 where the
 *    pre-activation is <= 0 (torch.relu).  fp32 throughout, contractions on v_mfma_f32_32x32x2_f32, no float atomics: every
 *    output is bit-identical from run to run, whichever other outputs are requested, and is overwritten, never accumulated into.
 *    - feat: fp32 NHWC, 64 channels at channel stride in_cs >= 64 (a multiple of 4), 16-byte aligned.  grad_feat: contiguous
 *      [B,H,W,64], 16-byte aligned, may be NULL.
 *    - a head's operands are in the reference's layouts: w1 [head_conv,64,3,3], b1 [head_conv] (16-byte aligned), w2 [C,head_conv]
 *      (b2 is not read), grad_out [B,C,H,W] NCHW fp32; grad_w1 / grad_b1 / grad_w2 / grad_b2 in the layouts of w1 / b1 / w2 / b2, each
 *      may be NULL.  A head whose grad_out is NULL is skipped: nothing of it is written and it adds nothing to grad_feat.  With no
 *      live head grad_feat is zero.
 *    - head_conv % 64 == 0 and <= 256, nheads <= H3D_HEADS_MAX, in_cs >= 64: H3D_ERR_SHAPE otherwise, like non-positive sizes.
 *      1 <= C <= 96: H3D_ERR_UNSUPPORTED.  NULL feat / heads / a live head's operands, a misaligned pointer, a NULL or short workspace
 *      ("workspace" in the message): H3D_ERR_ARG.  Every check runs before the first HIP call.
 *    - workspace (256-byte aligned): with N = B*H*W, S = min(64, ceil(N / 512)) pixel splits, hc = head_conv, in floats
 *      2 * 576 hc (filter images) + 2 * N hc (gh and h of ONE head, NHWC; reused head after head) + S * (576 hc + 96 hc + hc + 96)
 *      (partials), each term rounded up to 256 bytes. */
typedef struct h3d_heads_bwd_head {
    const float *w1, *b1, *w2;
    const float *grad_out;
    float *grad_w1, *grad_b1, *grad_w2, *grad_b2;
    int32_t C;
    int32_t reserved;
} h3d_heads_bwd_head;
int h3d_heads_backward_workspace_bytes(int B, int H, int W, int head_conv, int nheads, const int *C, size_t *bytes);
int h3d_heads_backward(const float *feat, int in_cs, int B, int H, int W, int head_conv, int nheads, const h3d_heads_bwd_head *heads,
                       float *grad_feat, void *workspace, size_t workspace_bytes, void *stream);

/* =====================================================================================
 * 2c. Convolution backward (csrc/conv_bwd.hip): the gradients of H3D_OP_CONV's operator, groups = 1,
 *         y = act(conv2d(x, W, b) + res)                 act = ReLU (H3D_CONV_BWD_RELU) or the identity
 *    at x, res, W and b (BatchNorm stays folded into W, b: fine-tuning with frozen statistics).  With g = dL/dy:
 *         gg = g * [y > 0] under ReLU (gradient 0 where y <= 0, torch.relu), else g;      grad_res = gg;   grad_b[o] = sum_px gg[o,px];
 *         grad_W[o,c,t] = sum_px gg[o,px] x[c, px*s + t*d - p];     grad_x[c,q] = sum_{o,t} W[o,c,t] gg[o,(q + p - t*d)/s].
 *    fp32 throughout, no float atomics: every output is bit-identical from run to run, whichever other outputs are requested, and is
 *    overwritten, never accumulated into.
 *    - x [B,H,W,C at x_cs], y and grad_y [B,Ho,Wo,Cout at y_cs / gy_cs]: fp32 NHWC with a channel stride >= the channels, a multiple
 *      of 4, 16-byte aligned.  y is the SAVED output and is read only with H3D_CONV_BWD_RELU (may be NULL without).  grad_x [B,H,W,C]
 *      and grad_res [B,Ho,Wo,Cout]: contiguous NHWC, 16-byte aligned.  weight / grad_weight: the reference's [Cout,C,kh,kw];
 *      grad_bias [Cout].  Every output pointer may be NULL (all NULL: nothing is launched).
 *    - h3d_conv2d_backward runs the matrix-core kernels (v_mfma_f32_32x32x2_f32) on 3x3 stride 1 pad 1, 3x3 stride 2 pad 1 and
 *      1x1 stride 1 pad 0 with dilation 1, C % 16 == 0, Cout % 16 == 0 and C, Cout <= H3D_CONV_BWD_MFMA_CMAX, and the general fp32 FMA
 *      kernels on everything else; h3d_conv2d_backward_general runs the general kernels on every configuration.
 *    - non-positive or inconsistent sizes (kernel larger than the padded input, kernel side > 64, a channel stride below the channels or
 *      no multiple of 4, more than 2^31 / 256 pixels or filter elements): H3D_ERR_SHAPE.  NULL x / weight / grad_y (y with
 *      H3D_CONV_BWD_RELU), unknown flag bits, a misaligned pointer, a NULL, misaligned or short workspace ("workspace" in the message):
 *      H3D_ERR_ARG.  Every check runs before the first HIP call.
 *    - workspace (256-byte aligned): with N = B*Ho*Wo, S = min(256, ceil(N / 512)) pixel splits (split length ceil(N / S) rounded up to 8),
 *      V = 4 if Cout % 4 == 0 else 1, P = 256 / min(Cout / V, 256) and Sb = ceil(N / (128 P)) chunks of the bias sums, in floats
 *      N Cout (gg; with H3D_CONV_BWD_RELU only) + kh kw Cout ceil64(C) (the grad_x filter image; matrix-core configurations only)
 *      + S kh kw Cout C (grad_W partials) + Sb Cout (grad_b partials), each term rounded up to 256 bytes. */
enum {
    H3D_CONV_BWD_RELU = 1           /* flags: act = ReLU; y is required */
};
#define H3D_CONV_BWD_MFMA_CMAX 2048 /* widest C / Cout of the matrix-core kernels (DLA-34's widest conv input is level5's Root: 1280) */
int h3d_conv2d_backward_workspace_bytes(int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                        int flags, size_t *bytes);
int h3d_conv2d_backward(const float *x, int x_cs, const float *weight, const float *y, int y_cs, const float *grad_y, int gy_cs,
                        float *grad_x, float *grad_res, float *grad_weight, float *grad_bias, int B, int C, int H, int W, int Cout,
                        int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int flags, void *workspace, size_t workspace_bytes,
                        void *stream);
int h3d_conv2d_backward_general(const float *x, int x_cs, const float *weight, const float *y, int y_cs, const float *grad_y, int gy_cs,
                                float *grad_x, float *grad_res, float *grad_weight, float *grad_bias, int B, int C, int H, int W, int Cout,
                                int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int flags, void *workspace,
                                size_t workspace_bytes, void *stream);

/* =====================================================================================
 * 2d. Max-pool and up-sample + add backward (csrc/pool_up_bwd.hip): the gradients of H3D_OP_MAXPOOL (2x2, stride 2, floor) and of
 *     H3D_OP_UPADD, y = skip + ConvTranspose2d(x; w, k = 2f, stride f, padding p = f/2, groups = C).
 *    Common: fp32 NHWC with a channel stride (*_cs >= C, a multiple of 4), 16-byte aligned; C % 4 == 0; every output pointer may be NULL
 *    (all NULL: nothing is launched); no float atomics: every output element is written exactly once, as a sum in a fixed order, so the
 *    results are bit-identical from run to run whichever other outputs are requested; outputs are overwritten, never accumulated into.
 *    Non-positive or inconsistent sizes (C % 4, a channel stride below C or no multiple of 4, f outside {2, 4, 8}, more than 2^31 / 4
 *    pixels): H3D_ERR_SHAPE.  NULL operands, a misaligned pointer, a NULL / misaligned / short workspace ("workspace" in the message):
 *    H3D_ERR_ARG.  Every check runs before the first HIP call.
 *    - h3d_maxpool2_backward: x [B,H,W,C], grad_y [B,H/2,W/2,C] (floor; not read when H < 2 or W < 2), grad_x [B,H,W,C at gx_cs].  The
 *      gradient of an output pixel goes to the FIRST element of its window, in the order (0,0), (0,1), (1,0), (1,1), that equals the
 *      window's maximum (the scan of torch's CPU max_pool2d: from -inf, move on `v > max || isnan(v)`); the other three elements and the
 *      last row / column of an odd H / W get 0.  The argmax is recomputed from x.
 *    - h3d_upsample_backward: x [B,H,W,C], w = H3D_OP_UPADD's tap-major [k*k][C] image (k = 2f), grad_y [B,H f,W f,C];
 *          grad_x[c,iy,ix] = sum_{ki,kj} w[ki,kj,c] gy[c, iy f - p + ki, ix f - p + kj]              (grad_x [B,H,W,C at gx_cs])
 *          grad_w[ki,kj,c] = sum_{b,iy,ix} x[b,c,iy,ix] gy[b,c, iy f - p + ki, ix f - p + kj]         (grad_w [k*k][C], contiguous)
 *      over the in-range positions (an out-of-range position enters as an exact zero).  The skip's gradient is grad_y itself.
 *      Order: grad_x is the sum of R = 1, 2, 16 (f = 2, 4, 8) fmaf chains over 2f / R kernel rows each, taps in (ki, kj) order, the
 *      chains added in order.  grad_w: one fmaf chain per tile of 8x8, 4x4, 2x2 input pixels (row-major), then with S = B * tiles,
 *      G = ceil(S / 64): chain g adds the tiles g, g + G, ... in order (at most 64 terms), and the G chain sums are added in order.
 *      workspace (256-byte aligned; read only with grad_w): ceil(S / G) G k k C floats + (G > 1 ? G k k C : 0), each rounded up to 256 bytes. */
int h3d_maxpool2_backward(const float *x, int x_cs, const float *grad_y, int gy_cs, float *grad_x, int gx_cs, int B, int C, int H, int W,
                          void *stream);
int h3d_upsample_backward_workspace_bytes(int B, int C, int H, int W, int f, size_t *bytes);
int h3d_upsample_backward(const float *x, int x_cs, const float *w, const float *grad_y, int gy_cs, float *grad_x, int gx_cs, float *grad_w,
                          int B, int C, int H, int W, int f, void *workspace, size_t workspace_bytes, void *stream);

/* =====================================================================================
 * 2e. BatchNorm2d with batch statistics (csrc/bn.hip): nn.BatchNorm2d (+ residual) (+ ReLU) in training and evaluation mode, and its
 *     gradients.  2d's common contract: fp32 NHWC with a channel stride (*_cs >= C, a multiple of 4), every operand 16-byte aligned,
 *     C % 4 == 0, every output pointer may be NULL, no float atomics, every output element written once as a sum in a fixed order that
 *     depends on the shape alone, outputs overwritten.  Errors as in 2d; N = B H W = 1 in training: H3D_ERR_SHAPE (torch refuses it too);
 *     eps < 0 or momentum outside [0, 1]: H3D_ERR_ARG.  Every check runs before the first HIP call.
 *       mean = sum x / N, var = sum (x - mean)^2 / N (biased, two passes), invstd = 1 / sqrt(var + eps)
 *       y = act((x - mean) (gamma invstd) + beta + res)          res optional; act = ReLU (relu != 0) or the identity
 *    - h3d_batch_norm_forward, training != 0: the statistics are the batch's.  Writes y, mean (= save_mean), var (biased), save_invstd and,
 *      in place, running_mean <- (1 - momentum) running_mean + momentum mean, running_var <- (1 - momentum) running_var + momentum var N / (N - 1).
 *      training == 0: `mean` / `var` are inputs (the running statistics); writes y and save_invstd.
 *      Launches: 1 in evaluation; in training 1 when the plan has one slot, else 3.
 *    - h3d_batch_norm_backward: gg = grad_y [y > 0] under ReLU (the mask from the saved output y; y is not read otherwise), else grad_y.
 *          grad_res = gg     grad_beta = sum gg     grad_gamma = sum gg xhat,  xhat = (x - save_mean) save_invstd
 *          training:   grad_x = gamma invstd (gg - grad_beta / N - xhat grad_gamma / N)
 *          evaluation: grad_x = gg gamma invstd
 *      gamma is read only with grad_x.  At most 2 launches.
 *    - Order of the sums (h3d_batch_norm_plan): a workgroup is V x PPP threads (V = 1, 2, 4, 8 = the smallest with 4 V >= min(C, 32),
 *      PPP = 256 / V) and owns `chunk` consecutive pixels of 4 V channels: thread p adds the pixels p, p + PPP, ... of the chunk in order (at
 *      most 64 terms), the PPP sums meet in a halving tree (h = PPP / 2 ... 1: p += p + h).  The `slots` = ceil(N / chunk) workgroup sums are
 *      added as h3d_upsample_backward adds its tiles: G = ceil(slots / 64) chains over the slots g, g + G, ..., then the chain sums in order.
 *      The per-channel scalars (the divisions by N, invstd, the running update) are formed in double and rounded once.
 *    - workspace (256-byte aligned): 2 slots C floats + 2 C floats, each rounded up to 256 bytes; needed by backward, and by the training
 *      forward when slots > 1. */
int h3d_batch_norm_workspace_bytes(int B, int C, int H, int W, size_t *bytes);
int h3d_batch_norm_plan(int B, int C, int H, int W, int *chunk, int *slots);
int h3d_batch_norm_forward(const float *x, int x_cs, const float *gamma, const float *beta, const float *res, int res_cs, float *y, int y_cs,
                           float *mean, float *var, float *save_invstd, float *running_mean, float *running_var, int B, int C, int H, int W,
                           int training, int relu, float momentum, float eps, void *workspace, size_t workspace_bytes, void *stream);
int h3d_batch_norm_backward(const float *x, int x_cs, const float *y, int y_cs, const float *grad_y, int gy_cs, const float *gamma,
                            const float *save_mean, const float *save_invstd, float *grad_x, int gx_cs, float *grad_res, int gr_cs,
                            float *grad_gamma, float *grad_beta, int B, int C, int H, int W, int training, int relu, void *workspace,
                            size_t workspace_bytes, void *stream);

/* =====================================================================================
 * 3. Heat-map decode (decode.py, utils.py).  All tensors contiguous NCHW fp32 as the
 *    reference's heads (model.py:485-489).  Index outputs are int64 like torch.topk's.
 *    Tie rule: equal scores -> lowest flat index first (torch leaves it unspecified).
 * ===================================================================================== */

/* _sigmoid (utils.py:8-10) optionally, then _nms (decode.py:6-13) and the per-channel top-K of
 * _topk_channel / stage 1 of _topk (decode.py:15-24, 26-33) in one pass per (b, c) map.
 *   heat [B,C,H,W]; with H3D_NMS_SIGMOID heat holds logits and scores are
 *   clamp(sigmoid(x), 1e-4, 1-1e-4).  Requires K <= min(H*W, 1024), H*W <= 36864 (larger maps: h3d_nms_topk_large).
 *   out: scores [B,C,K] f32 (descending), inds [B,C,K] i64 (flat y*W+x), ys/xs [B,C,K] f32. */
#define H3D_NMS_SIGMOID 1 /* heat holds logits: apply _sigmoid first            */
#define H3D_NMS_SKIP 2    /* heat is already NMS-ed (plain _topk/_topk_channel) */
int h3d_nms_topk(const float *heat, int B, int C, int H, int W, int K, int flags,
                 float *scores, int64_t *inds, float *ys, float *xs, void *stream);
/* The same for TWO heat-map tensors [B,Ca,H,W] and [B,Cb,H,W] in one launch (the detector's `hm` and `hm_hp`,
 * decode.py:85 and :118: the 1-class map alone occupies B workgroups).  Outputs as h3d_nms_topk, per tensor. */
int h3d_nms_topk2(const float *heat_a, int Ca, float *scores_a, int64_t *inds_a, float *ys_a, float *xs_a,
                  const float *heat_b, int Cb, float *scores_b, int64_t *inds_b, float *ys_b, float *xs_b,
                  int B, int H, int W, int K, int flags, void *stream);

/* h3d_nms_topk for maps of any size (H * W > 36864: e.g. the 320 x 184 output of a --keep_res 1280 x 736 frame,
 * datasets/coco.py:160-163): the map is cut into bands of rows (each with one halo row on either side for the 3x3 max), the bands'
 * top K are merged; same results and the same tie rule as h3d_nms_topk.  workspace: h3d_nms_topk_large_workspace_bytes(...) bytes
 * (0 = the shape is not supported: a band of rows + two halo rows must fit 36864 pixels, bands x K <= 8192). */
size_t h3d_nms_topk_large_workspace_bytes(int B, int C, int H, int W, int K);
int h3d_nms_topk_large(const float *heat, int B, int C, int H, int W, int K, int flags,
                       float *scores, int64_t *inds, float *ys, float *xs,
                       void *workspace, size_t workspace_bytes, void *stream);

/* stand-alone _nms (decode.py:6-13): out = heat * (maxpool3x3(heat) == heat), [B,C,H,W] */
int h3d_nms(const float *heat, int B, int C, int H, int W, float *out, void *stream);
/* stand-alone _sigmoid (utils.py:8-10): out = clamp(sigmoid(in), 1e-4, 1-1e-4); in == out allowed */
int h3d_sigmoid_clamp(const float *in, float *out, size_t n, void *stream);

/* Stage 2 of _topk (decode.py:34-39): top-K over the C*K stage-1 candidates of each image.
 *   in : scores/inds/ys/xs [B,C,K];  out: score [B,K], ind [B,K] i64, cls [B,K] i32, y/x [B,K].
 *   Requires C*K <= 8192. */
int h3d_topk_merge(const float *scores, const int64_t *inds, const float *ys, const float *xs,
                   int B, int C, int K, float *o_score, int64_t *o_ind, int32_t *o_cls,
                   float *o_y, float *o_x, void *stream);

/* _transpose_and_gather_feat (utils.py:23-27): feat [B,C,H,W] (channels_last=0), ind [B,N]
 * -> out [B,N,C], without the NHWC transpose; _gather_feat (utils.py:12-21) itself is the
 * channels_last=1 case: feat [B,HW,C]. */
int h3d_gather_feat(const float *feat, const int64_t *ind, int B, int C, int HW, int N,
                    int channels_last, float *out, void *stream);

/* multi_pose_decode after the two top-k's (decode.py:86-161): gathers, boxes, keypoint
 * matching, assembly of dets [B,K,5+2J+1].  reg / hp_* may be NULL exactly as in the
 * reference signature (reg=None, hm_hp=None, hp_offset=None).
 *   centre top-k  : c_score/c_ind/c_cls/c_y/c_x [B,K]
 *   joint  top-k  : hp_score/hp_ind/hp_y/hp_x [B,J,K] (NULL when hm_hp is None)
 *   wh [B,2,H,W], hps [B,2J,H,W], reg [B,2,H,W]|NULL, hp_offset [B,2,H,W]|NULL */
int h3d_multi_pose_assemble(const float *c_score, const int64_t *c_ind, const int32_t *c_cls,
                            const float *c_y, const float *c_x,
                            const float *hp_score, const int64_t *hp_ind, const float *hp_y,
                            const float *hp_x,
                            const float *wh, const float *hps, const float *reg,
                            const float *hp_offset,
                            int B, int J, int H, int W, int K, float *dets, void *stream);

/* ctdet_decode after _topk (decode.py:52-75): dets [B,K,6]. wh [B,2 or 2C,H,W]. */
int h3d_ctdet_assemble(const float *c_score, const int64_t *c_ind, const int32_t *c_cls,
                       const float *c_y, const float *c_x, const float *wh, const float *reg,
                       int B, int C, int H, int W, int K, int cat_spec_wh, float *dets,
                       void *stream);

/* Pre-process, val branch of datasets/coco_hp.py:151-212: images [B,h,w,3] uint8 (BGR, rows of
 * row_bytes) -> out [B,3,res_h,res_w] fp32 = ((warpAffine(img, M, INTER_LINEAR, border 0) / 255) - mean) / std.
 * minv [B,6] double = the INVERSE (dst -> src) 2x3 affine of get_affine_transform(c, s, 0, [res,res])
 * (utils/image.py:27-62); OpenCV's fixed-point bilinear scheme, see csrc/preprocess.hip. */
int h3d_preprocess(const uint8_t *images, int B, int h, int w, int row_bytes, const double *minv,
                   const float *mean, const float *stdv, int res_h, int res_w, float *out, void *stream);

/* ---- 3b. Training input: the train branch of the same loaders (csrc/augment.hip; h3d_amd/train_input.py) -------------------------
 * coco_hp.py:151-212 / coco.py:156-198 with split == 'train' and color_aug (utils/image.py:200-232): random crop, rotation, mirror,
 * colour augmentation, standardise, for B frames that may differ in size.  The random draws are the host's; per image the kernels get: */
struct h3d_train_image {
    double minv[6];            /* the INVERSE (dst -> src) 2x3 map of get_affine_transform(c, s, rot, [res_w, res_h]), as h3d_preprocess takes it;
                                  for a mirrored image c[0] is already w - c[0] - 1, as in the reference                                       */
    double light[3];           /* lighting_: np.dot(eig_vec, eig_val * alpha) in float64, added per channel (B, G, R) in double             */
    int64_t offset;            /* byte offset of the frame's first pixel in `images`                                                          */
    int32_t h, w, row_bytes;   /* 1 <= h, w <= 32767; row_bytes >= 3 w                                                                         */
    int32_t flipped;           /* 0 | 1: read source column w-1-x (the reference's img[:, ::-1, :])                                          */
    int32_t order[3];          /* the colour operations in their drawn order: a permutation of H3D_TRAIN_BRIGHTNESS / _CONTRAST / _SATURATION */
    float alpha[3];            /* per step of `order`: (float32)(1 + uniform(-0.4, 0.4)) ...                                                  */
    float one_minus_alpha[3];  /* ... and (float32)(1 - alpha), the subtraction in double                                                     */
    int32_t reserved;          /* 0                                                                                                           */
};                             /* 136 bytes, no padding                                                                                       */
#define H3D_TRAIN_BRIGHTNESS 0
#define H3D_TRAIN_CONTRAST 1
#define H3D_TRAIN_SATURATION 2
#define H3D_TRAIN_INPUT_NO_COLOR_AUG 1       /* options: opt.no_color_aug -- one launch, no workspace, order / alpha / light unread */
/*    images: one buffer of images_bytes bytes that holds every frame (BGR uint8 rows).  `desc` is the descriptor array in HOST memory --
 *    every per-image check below reads it, before the first HIP call -- and `desc_dev` the same B descriptors in device memory, which the
 *    kernels read.  mean / stdv [3] and out [B,3,res_h,res_w] fp32 on the device; gs_mean_out [B] fp32 or NULL: the grey mean contrast_
 *    blends with (written only with colour augmentation).  workspace: h3d_train_input_workspace_bytes (0 with NO_COLOR_AUG), 256-byte
 *    aligned.  Two launches (warp + fp64 grey sum; colour + standardise), one with NO_COLOR_AUG; the output is bit-identical from run to run.
 *    B, res_h, res_w, an image's h or w <= 0 or > 32767, row_bytes < 3 w, a frame that leaves the buffer: H3D_ERR_SHAPE.  NULL or
 *    misaligned pointers, unknown option bits, flipped outside 0 | 1, an order that is no permutation, a NULL or short workspace
 *    ("workspace" in the message): H3D_ERR_ARG. */
int h3d_train_input_workspace_bytes(int B, int res_h, int res_w, int options, size_t *bytes);
int h3d_train_input(const uint8_t *images, size_t images_bytes, const struct h3d_train_image *desc,
                    const struct h3d_train_image *desc_dev, int B, const float *mean, const float *stdv, int res_h, int res_w,
                    int options, void *workspace, size_t workspace_bytes, float *out, float *gs_mean_out, void *stream);

/* multi_pose_post_process (utils/post_process.py:41-52 + utils/image.py:19-68, inv affine with
 * rot = 0): dets [B,K,40] (output-res px) + c [B,2], s [B] -> out [B,K,39] image px.
 * J = 0 is the transform of ctdet_post_process (utils/post_process.py:24-38): dets [B,K,6] -> out [B,K,5] (box, score). */
int h3d_multi_pose_post_process(const float *dets, const float *c, const float *s, int B, int K,
                                int J, int out_h, int out_w, float *out, void *stream);

/* =====================================================================================
 * 4. SMPL pose/shape -> LBS mesh (north_star; no reference code: published formulation).
 *    Model tensors are packed by the host (h3d_amd/smpl.py: SMPLModel.device_pack):
 *      v_template [3][Vpad], shapedirsT [10][3][Vpad], posedirsT [207][3][Vpad], j_template [24*3],
 *      j_shapedirs [24*3][10], parents i32[24], lbs_idx i32[V][nnz], lbs_w f32[V][nnz]
 * ===================================================================================== */
/* per person: Rodrigues (24), pose feature (207), joints, kinematic chain.
 *   betas [P,10], thetas [P,72] -> pose_feat [P,207], A [P,24,12] (3x4 skinning transforms),
 *   joints [P,24,3] (posed joint positions); if coefT != NULL also the k-major coefficient matrix
 *   coefT [217][Ppad] = [beta | pose_feat]^T consumed by h3d_smpl_verts2 (Ppad multiple of 128). */
int h3d_smpl_pose(const float *betas, const float *thetas, const float *j_template,
                  const float *j_shapedirs, const int32_t *parents, int P,
                  float *pose_feat, float *A, float *joints, float *coefT, int Ppad, void *stream);
/* h3d_smpl_pose + the two gathers in front of it + h3d_smpl_coef_pack behind it in ONE launch (the detector's tail: at a per-GPU shard
 * of 8 images every launch of the tail is a sub-wave-count grid on the critical path): person p = detection p % n of image p / n reads
 * its thetas / betas from the `pose` [B,72,HW] / `shape` [B,10,HW] head maps at pixel inds[(p / n) * K + p % n] -- what
 * _transpose_and_gather_feat (utils.py:23-27) would copy out -- and coefK3 [Ppad][14][3][16] is written by the lanes that hold the
 * values (zero rows for p >= B*n; Ppad multiple of 128).  betas_out [B*n,10] may be NULL.  Bit-identical to the separate launches. */
int h3d_smpl_pose_heads(const float *pose_map, const float *shape_map, const int64_t *inds, int B, int K, int n, int HW,
                        const float *j_template, const float *j_shapedirs, const int32_t *parents, float *betas_out,
                        float *pose_feat, float *A, float *joints, void *coefK3, int Ppad, void *stream);
/* generation 3: blend shapes on the bf16 matrix cores with every fp32 operand split into three bf16 terms
 * (fp32-level accuracy, csrc/smpl.hip).  coefK3 [Ppad][14][3][16] bf16 = per person and K step of 16 the h/m/l terms
 * of [beta | pose_feat | 0] (h3d_smpl_coef_pack; Ppad multiple of 128), dirsK3 [3][Vpad][14][3][16] bf16 = the same
 * split of the K-contiguous direction rows (10 shape + 207 pose, zero padded to 224; Vpad multiple of 64;
 * h3d_amd/smpl.py: _dirs_k3), A from h3d_smpl_pose, <= 4 skinning weights per vertex. */
int h3d_smpl_coef_pack(const float *betas, const float *pose_feat, int P, int Ppad, void *coefK3, void *stream);
int h3d_smpl_verts3(const void *coefK3, const float *A, const float *v_template, const void *dirsK3,
                    const int32_t *lbs_idx, const float *lbs_w, int nnz, int P, int Ppad, int V, int Vpad,
                    float *verts, void *stream);
/* The same with all six products of the three-term split (h3d_smpl_verts3 keeps hh + hm + mh: 2^-16 relative per dropped
 * product, 2e-6 abs on the blend-shape displacement): agrees with the fp32 vector kernels to 2e-6 -- what the f32
 * (parity-mode) detectors run; 1.16x the time. */
int h3d_smpl_verts3_exact(const void *coefK3, const float *A, const float *v_template, const void *dirsK3,
                          const int32_t *lbs_idx, const float *lbs_w, int nnz, int P, int Ppad, int V, int Vpad,
                          float *verts, void *stream);
/* blend shapes + LBS: verts [P,V,3].  Model tensors struct-of-arrays with row stride Vpad:
 * v_template [3][Vpad], shapedirsT [10][3][Vpad], posedirsT [207][3][Vpad]. */
int h3d_smpl_verts(const float *betas, const float *pose_feat, const float *A,
                   const float *v_template, const float *shapedirsT, const float *posedirsT,
                   const int32_t *lbs_idx, const float *lbs_w, int nnz, int P, int V, int Vpad,
                   float *verts, void *stream);
/* same result, LDS-streamed generation 2 (needs nnz <= 4, Vpad % 64 == 0, Ppad % 128 == 0). */
int h3d_smpl_verts2(const float *coefT, const float *A, const float *v_template,
                    const float *shapedirsT, const float *posedirsT, const int32_t *lbs_idx,
                    const float *lbs_w, int nnz, int P, int Ppad, int V, int Vpad, float *verts,
                    void *stream);

/* =====================================================================================
 * 4b. SMPL backward (csrc/smpl_bwd.hip): the gradients of the stage above with respect to betas / thetas (h3d_smpl_backward) or to the
 *    `shape` / `pose` head maps (h3d_smpl_heads_backward), from upstream gradients at the vertices and / or the posed joints.
 *    betas [P,10], thetas [P,72] as the forward read them; grad_verts [P,V,3] or NULL; grad_joints [P,24,3] or NULL; the model pack of the
 *    forward (j_template, j_shapedirs, parents, v_template, dirsK3, lbs_idx, lbs_w) and dirsV3 [3 terms][224][3][Vpad] bf16, the same
 *    three-term split of the directions (round-to-nearest-even) stored V-contiguous for the transposed contraction (h3d_amd/smpl.py:
 *    _dirs_v3); grad_betas [P,10], grad_thetas [P,72], either may be NULL.
 *    - Asynchronous on `stream`, no allocation, no global state.  Everything is recomputed from betas / thetas and the model pack:
 *      nothing saved by the forward is needed.
 *    - The gradient is that of the exact formulation (oracle/smpl.py, including angle = ||theta + 1e-8||, axis = theta / angle): the
 *      same whichever forward generation produced the values.  v_posed is recomputed with all six products of the three-term split.
 *    - grad_verts == NULL: no vertex kernel is launched, only joints -> chain -> Rodrigues (one small launch), and the model pointers
 *      from v_template on and the workspace are not read.  Both upstream pointers NULL: the requested outputs are zero-filled.
 *      P == 0: nothing is launched, H3D_OK.
 *    - Reproducibility: grad_betas and grad_thetas are sums in a fixed order, bit-identical from run to run; no float atomics in
 *      h3d_smpl_backward.  The sum over the vertices into the 24 x 12 transform gradients is taken in vertex order inside a tile group
 *      (one plain-stored partial per group and person) and over the groups in order, in fp64; the sum over 3 Vpad into the 217 coefficient
 *      gradients is one fp32 MFMA chain per split and fp64 over the splits in order.
 *    - nnz > 4: H3D_ERR_UNSUPPORTED.  NULL required operands, or (with grad_verts) a NULL or short workspace: H3D_ERR_ARG, the latter
 *      with "workspace" in the message.  Negative sizes, V <= 0, nnz <= 0, Vpad % 64 != 0, Vpad < V, an operand of 2 GiB: H3D_ERR_SHAPE.
 *    - Out of scope: gradients with respect to the model tensors (shapedirs, posedirs, skinning weights, joint regressor), and second
 *      derivatives (the Python binding is once_differentiable).
 *    Workspace (device memory, 256-byte aligned; a256(x) = x rounded up to 256), with Ppad = P rounded up to 128,
 *    NG = ceil(Vpad / 64 / 4) vertex-tile groups and NS = ceil(3 Vpad / 1536) splits of the coefficient contraction:
 *      bytes = a256(4 P 207) [pose_feat] + a256(4 P 288) [A] + a256(4 P 72) [joints] + a256(1344 Ppad) [coefK3]
 *            + a256(4 P 3 Vpad) [g_vp] + a256(4 NG P 288) [transform-gradient partials] + a256(4 NS P 224) [coefficient partials]
 *    (6890 vertices: 83 kB + 31 kB + 12 kB per person beside the 3 kB of forward intermediates; `verts` itself is 83 kB), and 0 when
 *    want_verts == 0 or P == 0.  The size query returns a status and hands the size back through `bytes`. */
int h3d_smpl_backward_workspace_bytes(int P, int V, int Vpad, int nnz, int want_verts, size_t *bytes);
int h3d_smpl_backward(const float *betas, const float *thetas, const float *grad_verts, const float *grad_joints,
                      const float *j_template, const float *j_shapedirs, const int32_t *parents, const float *v_template,
                      const void *dirsK3, const void *dirsV3, const int32_t *lbs_idx, const float *lbs_w, int nnz, int P, int V, int Vpad,
                      float *grad_betas, float *grad_thetas, void *workspace, size_t workspace_bytes, void *stream);
/* The same with the parameters read where h3d_smpl_pose_heads reads them (person p = detection p % n of image p / n, pixel
 * inds[(p / n) * K + p % n] of pose_map [B,72,HW] / shape_map [B,10,HW]); P = B * n in the workspace formula.  grad_pose_map [B,72,HW] and
 * grad_shape_map [B,10,HW] (either may be NULL) are zero-filled by the callee on `stream`, then every person's 72 + 10 values are added at
 * its pixel with float atomic adds, because two detections of an image may share a pixel: the order of those adds varies (last bits of a
 * shared pixel), everything else is bit-identical from run to run -- as h3d_loss_backward scatters. */
int h3d_smpl_heads_backward(const float *pose_map, const float *shape_map, const int64_t *inds, int B, int K, int n, int HW,
                            const float *grad_verts, const float *grad_joints, const float *j_template, const float *j_shapedirs,
                            const int32_t *parents, const float *v_template, const void *dirsK3, const void *dirsV3,
                            const int32_t *lbs_idx, const float *lbs_w, int nnz, int V, int Vpad, float *grad_pose_map,
                            float *grad_shape_map, void *workspace, size_t workspace_bytes, void *stream);

/* =====================================================================================
 * 4c. SMPL keypoint reprojection loss (csrc/smpl_loss.hip; no reference code: the project's own definition).
 *    Per person slot p = b n + m (image b < B, the first n <= max_objs slots of its label rows), keypoint k < K, c in {x, y}:
 *      kp3d[p,k]   = sum_j JW[k,j] joints[p,j] + sum_{i<NV} VW[k,i] verts[p, VI[k,i]]     (j ascending, then i ascending; fp32, every
 *                                                                                          product and sum rounded on its own)
 *      (s, tx, ty) = cam_map[b, 0..2, ind[b,m]]                                            (NCHW [B,3,HW] read in place, raw values)
 *      pred[p,k,c] = s kp3d[p,k,c] + t_c
 *      l = sum m |pred - hps[b,m,2k+c]|,  num = sum m,  m = hps_mask[b,m,2k+c],  loss = l / (num + 1e-4)    (RegWeightedL1Loss's convention)
 *    joints [P,24,3], verts [P,V,3] (NULL with NV == 0), ind [B,max_objs] int64, hps [B,max_objs,2K], hps_mask [B,max_objs,2K] of
 *    mask_type H3D_LOSS_MASK_U8 | H3D_LOSS_MASK_F32; the regressor: joint_w [K,24], vert_idx i32 [K,NV], vert_w [K,NV].
 *    Outputs of the forward: kp3d [P,K,3], pred [P,K,2], stats [3] = {loss, l, num}.
 *    DECIDED HERE (as in section 5): a slot whose ind lies outside [0,HW) adds nothing to l, num or any gradient; its pred is stored as 0,
 *    its kp3d as for any slot.  A vert_idx entry outside [0,V) is skipped by the kernels (the Python constructor refuses it).
 *    - Forward: two launches, asynchronous on `stream`, no allocation.  One wave per slot; fp32 per lane -> wave shuffles -> LDS -> one
 *      plain-stored partial per workgroup, summed in a fixed order in fp64 by the finish launch: no float atomics, bit-identical from run
 *      to run.  num == 0 gives loss 0.
 *    - Backward: g = coef sign(pred - hps) m with coef = grad_out[0] / (num + 1e-4) formed in fp64 and rounded once (grad_out and stats in
 *      device memory; sign(0) = 0, torch's L1 subgradient), g_s = sum_{k,c} g kp3d_c, g_t_c = sum_k g, g_kp3d[p,k] = (s g_x, s g_y, 0);
 *      grad_joints [P,24,3] = sum_k JW[k,j] g_kp3d[p,k] (k ascending; every element stored), grad_verts [P,V,3] = sum over the inverted
 *      table (below) and 0 elsewhere, grad_cam_map [B,3,HW] = g_s, g_t added at the slot's pixel and 0 elsewhere.  Any of the three may be
 *      NULL (skipped).  Two launches: a zero fill of grad_cam_map and grad_verts, then the scatter; the camera values are added with float
 *      atomic adds because two slots may share a pixel -- the order of those adds varies (last bits of a shared pixel), everything else is
 *      bit-identical from run to run.  kp3d and pred are what the forward wrote.
 *    - The inverted table (built by the host, h3d_amd/smpl_loss.py): inv_vertex i32 [n_touched] = the vertices with a non-zero weight,
 *      ascending; inv_start i32 [n_touched + 1]; inv_k i32 / inv_w f32 [inv_start[n_touched]] = per touched vertex its (k, VW[k,i]) in
 *      (k, i) order.  n_touched <= K * H3D_SMPL_KP_MAX_NV.
 *    - Limits the kernels are built for: K <= H3D_SMPL_KP_MAX_K (one lane per (k, c) of a wave in the backward), NV <= H3D_SMPL_KP_MAX_NV.
 *      Beyond them: H3D_ERR_UNSUPPORTED.  B, max_objs, n, HW, K <= 0, n > max_objs, NV < 0, V <= 0 where vertices are used, more than
 *      2^31 / 96 person slots: H3D_ERR_SHAPE.  NULL operands, a bad mask_type, a NULL, short or not 8-byte aligned workspace
 *      ("workspace" in the message): H3D_ERR_ARG.  Every check runs before the first HIP call.
 *    Workspace: a256(8 ceil(B n / 4)) bytes, one {l, num} partial per workgroup of four slots.
 * ===================================================================================== */
#define H3D_SMPL_KP_MAX_K 32
#define H3D_SMPL_KP_MAX_NV 16
int h3d_smpl_kp_loss_workspace_bytes(int B, int n, size_t *bytes);
int h3d_smpl_kp_loss_forward(const float *joints, const float *verts, const float *cam_map, const int64_t *ind, const float *hps,
                             const void *hps_mask, int mask_type, const float *joint_w, const int32_t *vert_idx, const float *vert_w,
                             int B, int max_objs, int n, int HW, int K, int NV, int V, float *kp3d, float *pred, float *stats,
                             void *workspace, size_t workspace_bytes, void *stream);
int h3d_smpl_kp_loss_backward(const float *kp3d, const float *pred, const float *cam_map, const int64_t *ind, const float *hps,
                              const void *hps_mask, int mask_type, const float *stats, const float *grad_out, const float *joint_w,
                              const int32_t *inv_vertex, const int32_t *inv_start, const int32_t *inv_k, const float *inv_w, int n_touched,
                              int B, int max_objs, int n, int HW, int K, int V, float *grad_joints, float *grad_verts, float *grad_cam_map,
                              void *stream);

/* =====================================================================================
 * 4d. Mesh rendering: a z-buffered visibility-buffer rasteriser for batches of posed meshes under section 4c's weak-perspective camera
 *    (csrc/render.hip; h3d_amd/render.py; no reference code: the project's own definition).
 *    Inputs: verts [P,V,3] f32 with P = B n (slot p = b n + m belongs to image b), faces [F,3] i32 shared by all slots, cam_map
 *    [B,3,H,W] f32 and ind [B,max_objs] i64 read in place exactly as section 4c reads them, valid [P] u8 or NULL, dz [P] f32 or NULL
 *    (NULL = 0), the integer up-sampling factor up >= 1: the target is Hr x Wr = up H x up W pixels.
 *    Every float step below is ONE IEEE-754 binary32 operation, round to nearest even, no contraction, / and sqrt correctly rounded,
 *    denormals kept; (float)(integer) rounds to nearest even.
 *    PROJECTION of vertex (X, Y, Z) of slot p, with (s, tx, ty) = cam_map[b, 0..2, ind[b,m]] and cx = ind % W, cy = ind / W:
 *        xs = (float)up * (((s * X) + tx) + (float)cx)        ys = (float)up * (((s * Y) + ty) + (float)cy)
 *        fx = rintf(16 * xs), fy = rintf(16 * ys)              the 1/16-pixel lattice; xi = (int)fx, yi = (int)fy
 *        d  = Z + dz[p]            with H3D_RENDER_NEGATE_Z:  d = (-Z) + dz[p]            (a smaller d is nearer)
 *      A vertex is BAD when |fx| <= 2^19, |fy| <= 2^19 or |d| < inf fails (so with any NaN).  Pixel (i, j) of the target is sampled at
 *      lattice point (16 i, 16 j): no half-pixel shift (CenterNet's map-to-input scaling), so a vertex and the pred of section 4c of the
 *      same body point coincide.
 *    SKIPPED SLOTS (write nothing): ind outside [0,HW); valid[p] == 0; s NaN, infinite or <= 0.
 *    SKIPPED FACES: an index outside [0,V) (never dereferenced); a BAD vertex; o == 0, or H3D_RENDER_CULL_BACK and S < 0, where
 *        o = (int64)(x1 - x0) * (y2 - y0) - (int64)(y1 - y0) * (x2 - x0)                   (exact: every product is below 2^42)
 *        S = -o, with H3D_RENDER_NEGATE_Z S = o: the doubled signed area, POSITIVE when the side from which the face's vertices run
 *        counter-clockwise in the right-handed body frame -- the outside of an outward-oriented mesh -- is turned to the viewer.
 *    COVERAGE (exact integers): with o < 0 vertices 1 and 2 (and their d) change places, so that A = |o| > 0.  At lattice point (px, py)
 *        w0 = (x2 - x1) (py - y1) - (y2 - y1) (px - x1)       edge 0 = v1 -> v2
 *        w1 = (x0 - x2) (py - y2) - (y0 - y2) (px - x2)       edge 1 = v2 -> v0
 *        w2 = (x1 - x0) (py - y0) - (y1 - y0) (px - x0)       edge 2 = v0 -> v1               (w0 + w1 + w2 = A)
 *      The pixel is covered when for every edge w > 0, or w == 0 and the edge a -> b is a TOP edge (by == ay and bx > ax) or a LEFT edge
 *      (by < ay): the top-left rule -- a pixel centre on an edge shared by two faces belongs to exactly one of them, one on the right or
 *      bottom border of a mesh to none.  Only the pixels of the bounding box [ceil(min x / 16), floor(max x / 16)] x (the same in y),
 *      clipped to the target, are visited.
 *    DEPTH at a covered pixel:  depth = d0 + (((float)w1 * (d1 - d0)) + ((float)w2 * (d2 - d0))) / (float)A   (two differences, two
 *      products, one sum, one division, one sum, in this order; d1 and d2 after the exchange above).  A face of one depth has exactly that
 *      depth everywhere, and the rounding errors scale with the depth range of the face, not with its distance.  A face whose depth is NaN
 *      at the pixel does not take it.
 *    VISIBILITY: one 64-bit key per target pixel, key = hi << 32 | (m F + f) with u = the bits of depth and hi = ~u if u has its sign
 *      bit set, else u | 0x80000000 (unsigned order = float order, -0 below +0; invertible).  The key buffer starts as all ones (one
 *      memset) and every covering face takes an unsigned 64-bit atomic minimum: the result is the nearest face, among equal depths the
 *      smallest id, whatever the arrival order -- bit-identical from run to run.  No float atomics.  n F must be below 2^31.
 *    OUTPUTS (every byte is written; hand in uninitialised memory): face_id [B,Hr,Wr] i32 = m F + f or -1 (background);
 *      depth [B,Hr,Wr] f32 = the float recovered from the key, +inf for background; rgb [B,Hr,Wr,3] u8 (the shade entry point) over
 *      image [B,Hr,Wr,3] u8 or, with image NULL, the colour `background` (0xRRGGBB).
 *    SHADING of the winning face (f, m) of a pixel, headlight Lambert, from the body coordinates (v0, v1, v2 in the face's own order):
 *        e1 = v1 - v0, e2 = v2 - v0;  nx = e1y e2z - e1z e2y, ny = e1z e2x - e1x e2z, nz = e1x e2y - e1y e2x      (two products, one difference)
 *        len = sqrtf((nx nx + ny ny) + nz nz);   I = 0 if len == 0, else ambient + (1 - ambient) * (|nz| / len)
 *        out_c = sat8(rintf(alpha * (I * (float)colour_c) + (1 - alpha) * (float)image_c))     sat8: NaN and negatives 0, above 255 -> 255
 *      colour [P,3] u8 or NULL (then default_colour, 0xRRGGBB); a background pixel copies image_c (or the background colour).  A key whose
 *      id is not below n F, or whose face holds an index outside [0,V), is shaded as background (a key buffer of another mesh cannot
 *      make the kernel read out of bounds).  The keys are only read: one key buffer serves any number of shade calls.
 *    Launches: rasterize = one memset, render_raster_kernel (one workgroup per slot: the slot's projected vertices in LDS, 12 bytes each),
 *      render_resolve_kernel; shade = one render_resolve_kernel launch.  Asynchronous on `stream`, no allocation.
 *    Workspace: the key buffer, a256(8 B Hr Wr) bytes, 8-byte aligned; rasterize leaves the keys in it for the shade entry point.
 *    Checked before the first HIP call: NULL verts / faces / cam_map / ind / outputs / keys, a NULL, short or not 8-byte aligned
 *      workspace ("workspace" in the message), unknown flag bits, alpha or ambient outside [0,1] (or NaN): H3D_ERR_ARG; B, max_objs, n,
 *      V, F, H, W <= 0, n > max_objs, up < 1, Hr or Wr > H3D_RENDER_MAX_SIDE, B Hr Wr >= 2^31: H3D_ERR_SHAPE; V > H3D_RENDER_MAX_V (the
 *      largest V, a multiple of 64, whose 12 V bytes of staging fit the 160 KiB of LDS beside the 6 KiB face queue), n F >= 2^31:
 *      H3D_ERR_UNSUPPORTED.  There is no second path.
 * ===================================================================================== */
#define H3D_RENDER_NEGATE_Z 1
#define H3D_RENDER_CULL_BACK 2
#define H3D_RENDER_MAX_V 13120
#define H3D_RENDER_MAX_SIDE 16384
int h3d_render_workspace_bytes(int B, int Hr, int Wr, size_t *bytes);
int h3d_render_rasterize(const float *verts, const int32_t *faces, const float *cam_map, const int64_t *ind, const uint8_t *valid,
                         const float *dz, int B, int max_objs, int n, int V, int F, int H, int W, int up, int flags, int32_t *face_id,
                         float *depth, void *workspace, size_t workspace_bytes, void *stream);
int h3d_render_shade(const void *keys, const float *verts, const int32_t *faces, const uint8_t *colour, const uint8_t *image, int B, int n,
                     int V, int F, int Hr, int Wr, float alpha, float ambient, int default_colour, int background, uint8_t *rgb,
                     void *stream);

/* =====================================================================================
 * 4e. SMPL 3D supervision: the label transform and the rotation / shape / 3D-joint loss (csrc/smpl_sup.hip; h3d_amd/smpl_sup.py; no
 *    reference code: the project's own definition).  Model x / y are the output map's x / y (y down), as in 4c.
 *    pi = the mirror's joint permutation, the pairs (1,2) (4,5) (7,8) (10,11) (13,14) (16,17) (18,19) (20,21) (22,23); S = diag(-1, 1, 1).
 *    LABEL TRANSFORM (h3d_smpl_sup_labels), image b, output row m < max_objs = annotation m of pose_lab [B,M,72], shape_lab [B,M,10],
 *    joints_lab [B,M,24,3] or NULL, valid [B,M] f32, pose_w / joints_w [B,M,24] f32 or NULL, num [B] i32, reg_mask [B,max_objs] u8 (what
 *    h3d_multi_pose_targets wrote), flipped [B] i32 or NULL, rot2 [B,2,2] f64 or NULL (= identity):
 *      gate        = m < min(num[b], max_objs, M)  and  reg_mask[b,m] != 0  and  valid[b,m] != 0
 *      R_lab[j]    = Rodrigues(pose_lab[b,m,j])        smpl_pose.h's convention (angle = ||theta + 1e-8||), in fp64
 *      flipped:      R'[pi(j)] = S R_lab[j] S          J'[pi(j)] = S J_lab[j]         w'[pi(j)] = w[j]          (exact: sign changes only)
 *      then rot2:    R''[0]    = Rz R'[0]              J''[j]    = Rz J'[j]           Rz = [[A2, 0], [0, 1]], A2 = rot2[b]; the other 23
 *                                                                                     rotations are parent-relative: unchanged
 *      weights:      smpl_pose_w = gate ? (pose_w or valid) : 0;  smpl_shape_w = gate ? valid : 0;  smpl_joints_w = gate and joints_lab ?
 *                    (joints_w or valid) : 0
 *    Outputs, fp32, every element written: smpl_rotmat [B,max_objs,24,9] (row-major as SmplRot::R), smpl_pose_w [B,max_objs,24], smpl_shape
 *    [B,max_objs,10] (copied: a mirror does not change betas), smpl_shape_w [B,max_objs], smpl_joints [B,max_objs,24,3], smpl_joints_w
 *    [B,max_objs,24].  Rows and entries whose weight is 0 hold zeros and their labels are never read into a result (NaN labels behind
 *    valid == 0 are harmless).  The arithmetic is fp64, each product and sum rounded on its own, rounded once to fp32.  One launch.
 *    LOSS (h3d_smpl_sup_loss_forward), slot p = b n + m (the first n <= max_objs rows), theta = pose_map[b, :, ind[b,m]] and beta =
 *    shape_map[b, :, ind[b,m]] read in place from the NCHW fp32 head maps [B,72,HW] / [B,10,HW]:
 *      R[j]    = smpl_rodrigues<float>(theta_j)                                                 the SMPL forward's own bits
 *      l_pose  = sum_p sum_j wp[b,m,j] sum_{a<9} (R[j][a] - smpl_rotmat[b,m,j][a])^2            num_pose  = 9 sum wp
 *      l_shape = sum_p ws[b,m] sum_{k<10} (beta_k - smpl_shape[b,m,k])^2                        num_shape = 10 sum ws
 *      root(X) = 0.5 (X[1] + X[2])                                                              (section 8b's root = (1, 2))
 *      d_j     = (joints[p,j] - root(joints[p])) - (smpl_joints[b,m,j] - root(smpl_joints[b,m]))
 *      l_j3d   = sum_p sum_j wj[b,m,j] ||d_j||^2                                                num_j3d   = 3 sum wj
 *      stats[9] = {loss_t, l_t, num_t} for t = pose, shape, j3d;  loss_t = l_t / (num_t + 1e-4)
 *    joints [P,24,3] (P = B n) is what h3d_smpl_pose_heads wrote; NULL = the third term is absent (stats[6..8] = 0).
 *    DECIDED HERE: a slot whose ind lies outside [0,HW) adds nothing to any l, num or gradient (as in sections 4c and 5); an entry whose
 *    weight is 0 adds exactly 0 even when its label is NaN (a select, not a product); rows m >= n are never read; num_t == 0 gives loss 0
 *    and zero gradients.
 *    - Forward: two launches, asynchronous on `stream`, no allocation.  One wave per slot, four per workgroup; fp32 per lane -> wave
 *      shuffles -> LDS -> six plain-stored partials per workgroup, summed in a fixed order in fp64 by the finish launch: no float atomics,
 *      bit-identical from run to run.
 *    - Backward (h3d_smpl_sup_loss_backward): coef_t = grad_out[t] / (num_t + 1e-4) formed in fp64 and rounded once (grad_out [3] and stats
 *      in device memory).  grad_pose_map [B,72,HW] += 2 coef wp sum_a (R - R_lab)_a dR_a / dtheta_c at the slot's pixel -- Rodrigues, the
 *      residual and the derivative recomputed in fp64 from the fp32 inputs and rounded once (an untrained head emits theta ~ 0, where the
 *      fp32 derivative of sin a / a and (1 - cos a) / a^2 is lost to cancellation); grad_shape_map [B,10,HW] += 2 coef ws (beta - beta_lab);
 *      grad_joints [P,24,3] = 2 coef wj[j] d_j, joints 1 and 2 each in addition -0.5 sum_j 2 coef wj[j] d_j (the sum by the wave's shuffle
 *      tree: a fixed order); every element of grad_joints is stored.  Any of the three may be NULL (skipped; grad_joints needs joints).  Two
 *      launches: a zero fill of the two maps, then the scatter; the map gradients are added with float atomic adds because two slots may
 *      share a pixel -- the order of those adds varies (last bits of a shared pixel), everything else is bit-identical from run to run.
 *    B, M, max_objs, n, HW <= 0, n > max_objs, more than 2^31 / 216 label rows: H3D_ERR_SHAPE.  NULL operands, joints_w without joints_lab,
 *    joints without smpl_joints / smpl_joints_w, grad_joints without joints, a pointer that is not aligned to its element, a NULL, short or
 *    not 8-byte aligned workspace ("workspace" in the message): H3D_ERR_ARG.  Every check runs before the first HIP call.
 *    Workspace: a256(24 ceil(B n / 4)) bytes, six partials per workgroup of four slots.
 * ===================================================================================== */
int h3d_smpl_sup_labels(const float *pose_lab, const float *shape_lab, const float *joints_lab, const float *valid, const float *pose_w,
                        const float *joints_w, const int32_t *num, const uint8_t *reg_mask, const int32_t *flipped, const double *rot2, int B,
                        int M, int max_objs, float *smpl_rotmat, float *smpl_pose_w, float *smpl_shape, float *smpl_shape_w, float *smpl_joints,
                        float *smpl_joints_w, void *stream);
int h3d_smpl_sup_loss_workspace_bytes(int B, int n, size_t *bytes);
int h3d_smpl_sup_loss_forward(const float *pose_map, const float *shape_map, const int64_t *ind, const float *joints, const float *smpl_rotmat,
                              const float *smpl_pose_w, const float *smpl_shape, const float *smpl_shape_w, const float *smpl_joints,
                              const float *smpl_joints_w, int B, int max_objs, int n, int HW, float *stats, void *workspace,
                              size_t workspace_bytes, void *stream);
int h3d_smpl_sup_loss_backward(const float *pose_map, const float *shape_map, const int64_t *ind, const float *joints, const float *smpl_rotmat,
                               const float *smpl_pose_w, const float *smpl_shape, const float *smpl_shape_w, const float *smpl_joints,
                               const float *smpl_joints_w, int B, int max_objs, int n, int HW, const float *stats, const float *grad_out,
                               float *grad_pose_map, float *grad_shape_map, float *grad_joints, void *stream);

/* =====================================================================================
 * 5. Losses (losses.py, trains/trainer.py:29-137): the focal term of `_neg_loss` (losses.py:42-67) and the four gathered regression
 *    terms, forward and backward, in descriptor form: one h3d_loss_term per term, ALL terms of a call in one partial-sum launch plus
 *    one finish launch (csrc/loss.hip).  No host synchronisation: where the reference branches on the host (`if num_pos == 0`) the
 *    finish kernel selects on the device.  Every sum is taken in a fixed order (fp32 per thread, wave shuffles, LDS, one plain-stored
 *    partial per workgroup, fp64 over the partials): the statistics are bit-identical from run to run.
 *    kinds:
 *      H3D_LOSS_FOCAL        x, gt [n] fp32.  p = x, or clamp(sigmoid(x), 1e-4, 1-1e-4) with H3D_LOSS_FROM_LOGITS (then `pred`, when not NULL,
 *                            receives p: bit-identical to h3d_sigmoid_clamp).  gt == 1: pos += log(p) (1-p)^2, num_pos += 1; gt < 1:
 *                            neg += log(1-p) p^2 (1-gt)^4; gt > 1 (or NaN): nothing.  loss = -neg if num_pos == 0, else -(pos+neg)/num_pos.
 *                            aux = {pos, neg, num_pos}.  Any 4-byte aligned pointers, any n.
 *      H3D_LOSS_REG_L1       RegL1Loss (losses.py:139-149): x = feat [B,C,HW] (NCHW, read in place at b C HW + c HW + ind), ind [B,M] int64,
 *                            mask [B,M], gt = target [B,M,C]; per (b,m,c) with k = mask[b,m]: num += |p k - t k|, den += k (the sum of the
 *                            EXPANDED mask).  loss = num / (den + 1e-4).  aux = {num, den, 0}
 *      H3D_LOSS_REG_WEIGHTED_L1  RegWeightedL1Loss (losses.py:165-175): the same with mask [B,M,C]
 *      H3D_LOSS_NORM_REG_L1  NormRegL1Loss (losses.py:151-163): mask [B,M]; num += |p / (t + 1e-4) k - k|
 *      H3D_LOSS_REG_SL1      RegLoss (losses.py:97-112, 123-137): mask [B,M]; num += smooth_l1(p k - t k), den += k once per (b,m) (the
 *                            UNEXPANDED mask)
 *    mask_type: H3D_LOSS_MASK_U8 (uint8) or H3D_LOSS_MASK_F32.  DECIDED HERE: a slot whose ind lies outside [0,HW) reads nothing and adds
 *    nothing to num or den (the reference gathers out of bounds).
 *    Backward: grad (shaped like x; NULL = this term is skipped, nothing is written for it) = coef[t] * d loss_t / d x, the 1/num_pos or
 *    1/(den + 1e-4) read from the forward's stats on the device.  FROM_LOGITS chains through the clamp (gradient passes for
 *    1e-4 <= sigmoid(x) <= 1-1e-4, torch's rule) and p (1-p), p recomputed from x.  A regression term's grad is zero-filled in one
 *    launch and scattered in the next (slots with mask 0 skipped; slots sharing an ind accumulate with float atomic adds: the order
 *    of those adds varies, everything else is bit-identical from run to run).
 *    A term with no elements (n == 0, or B C M HW == 0) launches nothing, reads no pointer and has loss 0; n_terms == 0 launches nothing and
 *    sets the total to 0.  Negative sizes: H3D_ERR_SHAPE; NULL terms / stats / operands: H3D_ERR_ARG; more than H3D_LOSS_MAX_TERMS
 *    terms: H3D_ERR_UNSUPPORTED; a NULL or short workspace: H3D_ERR_ARG ("workspace" in the message).
 * ===================================================================================== */
enum { H3D_LOSS_FOCAL = 1, H3D_LOSS_REG_L1 = 2, H3D_LOSS_REG_WEIGHTED_L1 = 3, H3D_LOSS_NORM_REG_L1 = 4, H3D_LOSS_REG_SL1 = 5 };
enum { H3D_LOSS_MASK_U8 = 0, H3D_LOSS_MASK_F32 = 1 };
#define H3D_LOSS_FROM_LOGITS 1       /* focal: x holds logits                                                                          */
#define H3D_LOSS_TUNE_GRID8 0x100    /* tests: at most 8 workgroups for this term, so that the grid-stride loop wraps at small sizes   */
#define H3D_LOSS_MAX_TERMS 16
typedef struct h3d_loss_term {
    int32_t kind;        /* H3D_LOSS_*                                                             */
    int32_t flags;       /* H3D_LOSS_FROM_LOGITS | H3D_LOSS_TUNE_GRID8                              */
    const float *x;      /* focal: logits or probabilities [n]; regression: feat [B,C,HW]          */
    const float *gt;     /* focal: gt [n]; regression: target [B,M,C]                              */
    float *pred;         /* focal + FROM_LOGITS: receives p [n], or NULL                           */
    const int64_t *ind;  /* regression: [B,M]                                                      */
    const void *mask;    /* regression: [B,M] ([B,M,C] for REG_WEIGHTED_L1) of mask_type           */
    float *grad;         /* backward: d/dx, shaped like x; NULL = skip this term                   */
    int64_t n;           /* focal: elements                                                        */
    int32_t B, C, HW, M; /* regression                                                             */
    int32_t mask_type;   /* H3D_LOSS_MASK_*                                                        */
    float weight;        /* the term's weight in the total                                         */
} h3d_loss_term;
/* stats: 4 * n_terms + 1 floats of device memory: per term {loss, aux0, aux1, aux2}, then total = sum of weight_t * loss_t (in term
 * order, fp64).  workspace: h3d_loss_workspace_bytes bytes (16 per workgroup of the partial launch), 16-byte aligned. */
int h3d_loss_workspace_bytes(const h3d_loss_term *terms, int n_terms, size_t *bytes);
int h3d_loss_forward(const h3d_loss_term *terms, int n_terms, float *stats, void *workspace, size_t workspace_bytes, void *stream);
/* stats: what h3d_loss_forward wrote for the same terms; coef [n_terms]: device memory, the upstream coefficient of each term's loss. */
int h3d_loss_backward(const h3d_loss_term *terms, int n_terms, const float *stats, const float *coef, void *stream);

/* =====================================================================================
 * 6. Training targets (csrc/targets.hip): the label half of the reference's dataset items, COCOHP._get_label (datasets/coco_hp.py:215-309)
 *    and the ctdet block of COCO.__getitem__ (datasets/coco.py:203-248), for a whole batch in two launches: an objects kernel (one wave
 *    per (image, object): box path, radius, rows, the compact gt_det) and a render kernel (one workgroup per 1024 pixels of one map: the
 *    maximum over the splats that cover a pixel).  Asynchronous on `stream`, no allocation, no memset, no atomics: every element of every
 *    requested output is stored exactly once, zeros included (hand in uninitialised memory), bit-identical from run to run.
 *    Inputs (device memory):
 *      boxes      [B,M,4] f32    COCO xywh of the annotations, M = the row stride of the inputs
 *      keypoints  [B,M,J,3] f32  (x, y, visibility)                                  (multi_pose)
 *      cls        [B,M] i32      class index in [0, num_classes); outside it the object is skipped          (ctdet)
 *      num        [B] i32        annotations of the image; min(num, M, max_objs) are used, negative = 0
 *      trans      [B,2,6] f64    row-major 2x3 matrices: [b,0] = trans_output, [b,1] = trans_output_rot (ctdet reads [b,0] only)
 *      rot_flag   [B] i32        non-zero = the image's `rot != 0` (multi_pose); NULL = no image is rotated
 *      flipped    [B] i32, width [B] i32   non-zero = mirrored, and the image width the mirror uses; flipped == NULL = none (then width may
 *                                be NULL)
 *      flip_pairs [n_flip_pairs,2] i32     the joint pairs a mirror swaps (flip_idx), applied in order; NULL with n_flip_pairs == 0
 *    Arithmetic: float32 wherever numpy holds float32 (xywh -> xyxy, the mirror, the clip, h, w, ct, reg), float64 for the 2x3 matrix
 *    times [x, y, 1] (rounded to float32 once) and for gaussian_radius (utils/image.py:97-117, its operation order); the splat value
 *    exp(-(dx^2 + dy^2) / (2 sigma^2)), sigma = (2r + 1) / 6, in float64, rounded to float32, combined by maximum.  Not built because they
 *    never change a value: the eps * max threshold of gaussian2D and the 0.9999 written for a person without keypoints.
 *    Outputs (device memory; ANY may be NULL = not wanted, nothing is written for it), N = max_objs, dtypes of the reference:
 *      multi_pose: hm [B,1,H,W] f32, hm_hp [B,J,H,W] f32, wh [B,N,2] f32, reg [B,N,2] f32, ind [B,N] i64, reg_mask [B,N] u8,
 *                  kps [B,N,2J] f32, kps_mask [B,N,2J] u8, hp_offset [B,N*J,2] f32, hp_ind [B,N*J] i64, hp_mask [B,N*J] i64,
 *                  gt_det [B,N,5+2J+1] f32 = [bbox(4), 1, pts(2J), 0] per LIVE object, compact in object order, zero rows behind them,
 *                  gt_count [B] i32 = the live objects.  An image with rot_flag: hm = 0.9999 everywhere, reg_mask = kps_mask = 0.
 *      ctdet:      hm [B,num_classes,H,W], wh, reg, ind, reg_mask as above, cat_spec_wh [B,N,2 num_classes] f32, cat_spec_mask (same
 *                  shape) u8, gt_det [B,N,6] = [ct -+ w/2, ct -+ h/2, 1, cls], gt_count [B].
 *    Pointers need the alignment of their element type only (maps are stored with 16-byte stores wherever 4 pixels share an aligned
 *    16 bytes, whatever the base and the width).
 *    Workspace: (1 + num_joints) * B * max_objs splat slots of 16 bytes {x, y, r, cls}, r < 0 = none (ctdet: num_joints = 0); 16-byte
 *    aligned; needed only when a map is requested.  The size query returns a status and hands the size back through `bytes`.
 *    options: H3D_TARGETS_MSE_LOSS (draw_msra_gaussian), H3D_TARGETS_DENSE_HP, H3D_TARGETS_DENSE_WH (draw_dense_reg depends on the object
 *    order) are out of scope: H3D_ERR_UNSUPPORTED, as are J > 64 and max_objs > 512.  Negative sizes, Hout / Wout / max_objs <= 0 or
 *    Hout, Wout > 16384, more than 65535 images or channels: H3D_ERR_SHAPE.  NULL required inputs, a misaligned pointer, a NULL or short
 *    workspace ("workspace" in the message): H3D_ERR_ARG.  B == 0: nothing is launched, H3D_OK.
 * ===================================================================================== */
#define H3D_TARGETS_MSE_LOSS 1
#define H3D_TARGETS_DENSE_HP 2
#define H3D_TARGETS_DENSE_WH 4
#define H3D_TARGETS_MAX_JOINTS 64
#define H3D_TARGETS_MAX_OBJS 512
int h3d_targets_workspace_bytes(int B, int max_objs, int num_joints, size_t *bytes);
int h3d_multi_pose_targets(const float *boxes, const float *keypoints, const int32_t *num, const double *trans, const int32_t *rot_flag,
                           const int32_t *flipped, const int32_t *width, const int32_t *flip_pairs, int n_flip_pairs, int B, int M, int J,
                           int Hout, int Wout, int max_objs, float *hm, float *hm_hp, float *wh, float *reg, int64_t *ind,
                           uint8_t *reg_mask, float *kps, uint8_t *kps_mask, float *hp_offset, int64_t *hp_ind, int64_t *hp_mask,
                           float *gt_det, int32_t *gt_count, int options, void *workspace, size_t workspace_bytes, void *stream);
int h3d_ctdet_targets(const float *boxes, const int32_t *cls, const int32_t *num, const double *trans, const int32_t *flipped,
                      const int32_t *width, int B, int M, int Hout, int Wout, int num_classes, int max_objs, float *hm, float *wh,
                      float *reg, int64_t *ind, uint8_t *reg_mask, float *cat_spec_wh, uint8_t *cat_spec_mask, float *gt_det,
                      int32_t *gt_count, int options, void *workspace, size_t workspace_bytes, void *stream);

/* =====================================================================================
 * 7. Optimiser (csrc/optim.hip): multi-tensor Adam, the step of torch.optim.Adam(model.parameters(), opt.lr) (trains/trainer.py:166,
 *    264-267) for a whole parameter list in one launch.  fp32 storage and arithmetic; asynchronous on `stream`, no allocation, no
 *    workspace, no table upload: the descriptors travel as the kernel argument, H3D_ADAM_CAPACITY tensors per launch (a longer list
 *    takes ceil(T / H3D_ADAM_CAPACITY) launches; tensors with n == 0 take no slot).  Per element, every step ONE IEEE-754 binary32
 *    operation, round to nearest, no contraction, sqrt and / correctly rounded, denormals kept:
 *        g   = grad                      (weight_decay != 0:  g = grad + weight_decay * p)
 *        m   = m + one_minus_b1 * (g - m)
 *        v   = v * b2;   v = v + (one_minus_b2 * g) * g
 *        den = sqrt(v) / bc2_sqrt + eps
 *        p   = p + neg_step_size * (m / den)
 *    with the scalars torch's single-tensor path forms on the host in double and rounds to float once: bc2_sqrt = sqrt(1 - b2^t),
 *    neg_step_size = -(lr / (1 - b1^t)), t = the tensor's own step count.  `tensors` is HOST memory (read before the call returns); its
 *    pointers are device memory, 4-byte aligned: 16-byte accesses are used where the four bases of a tensor share their offset inside
 *    16 bytes, and the result of an element does not depend on the access it takes.  A workgroup steps H3D_ADAM_CHUNK elements.
 *    Checked before the first HIP call: n_tensors < 0 or n < 0: H3D_ERR_SHAPE; NULL `tensors`, a NULL pointer in a tensor with n > 0,
 *    a base off a 4-byte boundary, a non-finite scalar, b2 outside [0,1), eps < 0, bc2_sqrt <= 0: H3D_ERR_ARG.  n_tensors == 0 and
 *    tensors with n == 0 launch nothing.  The buffers of one call must not overlap.
 * ===================================================================================== */
#define H3D_ADAM_CAPACITY 48
#define H3D_ADAM_CHUNK 2048
typedef struct h3d_adam_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t n;
    float one_minus_b1, b2, one_minus_b2, bc2_sqrt, eps, neg_step_size, weight_decay;
} h3d_adam_tensor;
int h3d_adam_step(const h3d_adam_tensor *tensors /* host memory */, int n_tensors, void *stream);

/* =====================================================================================
 * 8. Evaluation (csrc/eval.hip; h3d_amd/coco_eval.py): COCO keypoint (OKS) and box AP on the device tensors the
 *    detectors produce -- what the reference's val() gets from pycocotools' COCOeval (datasets/coco_hp.py:92-138, datasets/coco.py:
 *    126-135).  Detections are fp32 and widened exactly; ground truth, thresholds and every result are fp64.  Every step is ONE IEEE-754
 *    binary64 operation, round to nearest, no contraction, in the order written here (tests/coco_eval_ref.py restates it with loops);
 *    exp is the only operation that is not correctly rounded.  Asynchronous on `stream`, no allocation.
 *
 *    h3d_coco_match, one workgroup per image n.  dets [N,D,det_stride] f32: a row is x1, y1, x2, y2, score and, for keypoints, 17 (x, y)
 *    pairs; det_cls [N,D] i32 or NULL (all class 0); det_num [N] i32 or NULL (all D; clamped to [0,D]); ground truth padded to G per
 *    image: gt_boxes [N,G,4] (x, y, w, h), gt_keypoints [N,G,17,3] (x, y, v; keypoints only), gt_area, gt_iscrowd (u8), gt_cls [N,G],
 *    gt_num [N] (clamped to [0,G]).  area_rng [A,2], iou_thrs [T], kp_vars [17] = (2 sigma)^2: device memory, written by the host, so
 *    that device and host compare against the same doubles.
 *      records  w = x2 - x1, h = y2 - y1 in fp64; with H3D_COCO_ROUND2 every box value, the score and every keypoint coordinate v becomes
 *               rint(v * 100) / 100 = float("{:.2f}".format(v)), the reference's export rounding (DOMAIN: finite values, |v| < 2^20;
 *               rint is half-to-even like the decimal formatting on an exact tie).  area = w * h of the rounded box, for both types.
 *               Written to dt_box [N,D,4] (x, y, w, h), dt_score, dt_area [N,D], dt_keypoints [N,D,34]; rows d >= det_num are 0.
 *      ranks    dt_rank [N,D]: the detection's place among those of its image AND class by score descending, stable (ties in index
 *               order); -1 for d >= det_num.  Detections with rank >= max_det (the largest maxDet) are not matched.
 *      ignore   gt_ignore [N,A,G] = iscrowd (keypoints: or no joint with v > 0) or area < lo or area > hi; 0 in the padding.
 *      matrix   row d, column g, 0 in the padding.  Boxes: iw = min(dx + dw, gx + gw) - max(dx, gx), ih likewise; 0 if either is <= 0,
 *               else I = iw ih, U = dw dh (crowd) or dw dh + gw gh - I, I / U.  Keypoints: k1 = joints with vg > 0; per joint
 *               dx = xd - xg (k1 > 0) or max(0, x0 - xd) + max(0, xd - x1) with x0 = x - w, x1 = x + w 2 of the ground-truth box
 *               (k1 = 0), dy likewise; e = (dx dx + dy dy) / vars / (area + 2^-52) / 2; oks = (sum of exp(-e) in joint order over the
 *               joints with vg > 0, or over all 17 when k1 = 0) / (k1 or 17).  Classes are not looked at here.
 *      walk     per (area range, threshold t), detections in score order, each against the ground truths of its class, not-ignored
 *               ones first (stable): best = min(t, 1 - 1e-10), m = none; skip g if matched at this t and not crowd; stop if m is a
 *               not-ignored one and g is ignored; skip if matrix[d,g] < best; else best = matrix[d,g], m = g (the last of equals
 *               wins).  dt_match [N,A,T,D] = m (index into the image's ground truths, -1 = none), dt_ignore = gt_ignore of m, or,
 *               unmatched, area of d outside the range.  Unranked and padding detections: -1 and 0.
 *    ious [N,D,G] may be NULL; the matrix then lives in LDS when D G 8 <= 96 KiB and in the workspace otherwise (bytes from
 *    h3d_coco_match_workspace_bytes; with ious given no workspace is used).  LIMITS: D <= H3D_COCO_MAX_D, G <= H3D_COCO_MAX_G,
 *    A <= H3D_COCO_MAX_A, A T <= H3D_COCO_MAX_LANES: H3D_ERR_UNSUPPORTED beyond them, checked before the first HIP call, nothing is
 *    written.  Negative sizes, det_stride < 5 (39 for keypoints), max_det < 1, N A T D or N A G >= 2^31: H3D_ERR_SHAPE.  NULL required
 *    operands, an unknown iou_type or flag, an fp64 pointer off an 8-byte boundary, a NULL or short workspace ("workspace" in the
 *    message): H3D_ERR_ARG.  N == 0: nothing is launched.
 *
 *    h3d_coco_accumulate, one workgroup per (class k, area range a, maxDet m, threshold t).  order [N D] i64: flat indices n D + d of ALL
 *    detection slots sorted by class, and inside a class by dt_score descending, stable with respect to n D + d (two stable sorts);
 *    seg_start [K+1] i32: the first position of every class in it (slots that belong to no class of 0 .. K-1 lie outside
 *    [seg_start[0], seg_start[K])).  Of its class' detections the row keeps those with 0 <= dt_rank < max_dets[m]:
 *        npig = ground truths of class k with gt_ignore == 0;  npig == 0: precision and recall of the cell are -1
 *        tp = running count of (matched and not dt_ignore), fp = of (unmatched and not dt_ignore)
 *        rc = tp / npig;  pr = tp / (fp + tp + 2^-52);  recall = the last rc, 0 without detections
 *        precision[r] = max { pr[i] : rc[i] >= rec_thrs[r] }, 0 for the empty set
 *    which is COCOeval's right-to-left envelope followed by searchsorted(rc, recThrs, 'left').  precision [T,R,K,A,M], recall
 *    [T,K,A,M] fp64.  max_dets [M] is HOST memory (read before the call returns), M <= H3D_COCO_MAX_M; rec_thrs [R] device memory,
 *    ascending, R <= H3D_COCO_MAX_R.  The workspace (h3d_coco_accumulate_workspace_bytes) holds npig [K,A] i32 at its start.
 *    A workgroup scans H3D_COCO_SCAN_CHUNK positions per step.  Errors as above.
 * ===================================================================================== */
#define H3D_COCO_BBOX 0
#define H3D_COCO_KEYPOINTS 1
#define H3D_COCO_ROUND2 1
#define H3D_COCO_MAX_D 128
#define H3D_COCO_MAX_G 1024
#define H3D_COCO_MAX_A 4
#define H3D_COCO_MAX_LANES 64
#define H3D_COCO_MAX_M 4
#define H3D_COCO_MAX_R 128
#define H3D_COCO_SCAN_CHUNK 1024
int h3d_coco_match_workspace_bytes(int N, int D, int G, size_t *bytes);
int h3d_coco_match(const float *dets, int det_stride, const int32_t *det_cls, const int32_t *det_num, const double *gt_boxes,
                   const double *gt_keypoints, const double *gt_area, const uint8_t *gt_iscrowd, const int32_t *gt_cls,
                   const int32_t *gt_num, int N, int D, int G, int iou_type, int flags, int max_det, const double *area_rng, int A,
                   const double *iou_thrs, int T, const double *kp_vars, double *ious, int32_t *dt_match, uint8_t *dt_ignore,
                   uint8_t *gt_ignore, double *dt_score, int32_t *dt_rank, double *dt_box, double *dt_area, double *dt_keypoints,
                   void *workspace, size_t workspace_bytes, void *stream);
int h3d_coco_accumulate_workspace_bytes(int K, int A, size_t *bytes);
int h3d_coco_accumulate(const int64_t *order, const int32_t *seg_start, const int32_t *dt_rank, const int32_t *dt_match,
                        const uint8_t *dt_ignore, const uint8_t *gt_ignore, const int32_t *gt_cls, const int32_t *gt_num, int N, int D,
                        int G, int K, int A, int T, const int32_t *max_dets /* host memory */, int M, const double *rec_thrs, int R,
                        double *precision, double *recall, void *workspace, size_t workspace_bytes, void *stream);

/* =====================================================================================
 * 8b. 3D evaluation (csrc/mesh_eval.hip; h3d_amd/mesh_eval.py; no reference code: the project's own definition):
 *    MPJPE / PVE (the plain error) and PA-MPJPE / PA-PVE (the error after a similarity Procrustes alignment) of P pairs of point sets.
 *    Points are fp32 and widened exactly; everything after the loads is fp64, every step ONE IEEE-754 binary64 operation, round to
 *    nearest, no contraction, in the order written here, parentheses included (tests/mesh_eval_ref.py restates it with loops,
 *    mesh_eval.evaluate_numpy is the numpy mirror; + - * / and sqrt are correctly rounded, so the kernels are bit-equal to both).
 *    Asynchronous on `stream`, no allocation, no workspace, no atomics: two calls give the same bits.
 *
 *    h3d_pointset_errors, one workgroup per pair k.  pred [Np,n,3], gt [Ng,n,3] f32; pred_idx, gt_idx [P] i32: pair k compares
 *    pred[pred_idx[k]] with gt[gt_idx[k]] (an index may repeat).  An index < 0 or >= Np (Ng) makes the pair INVALID: nothing of it is
 *    dereferenced, err, count and transform of the pair are 0.  weight [Ng,n] u8 or NULL (all ones): point i of the pair is valid when
 *    weight[gt_idx[k], i] != 0; count [P] = the valid points; count == 0: everything of the pair is 0.  Root sources pred_root
 *    [Np,nr,3], gt_root [Ng,nr,3] f32 (both or neither) and 0 <= root_a, root_b < nr: the origins are o_p = (src[a] + src[b]) * 0.5 per
 *    coordinate of pred_root[pred_idx[k]], o_g likewise of gt_root[gt_idx[k]] (a == b: that point itself; the weight is not looked at);
 *    without root sources both are 0.
 *      SUM      "sum over i of f(i)" below is, for every n: thread t of 256 starts at 0.0 and adds f(i) for the VALID i = t, t + 256, ...
 *               in ascending order; inside each of the four waves (threads 64 w .. 64 w + 63) v[l] = v[l] + v[l + off] for off = 32, 16,
 *               8, 4, 2, 1 (lanes l < off; lane 0 holds the wave's sum); the result is ((w0 + w1) + w2) + w3.  A function of n and the
 *               weights only: never of P, the grid or the batch.
 *      plain    err[k,0] = SUM |(p - o_p) - (g - o_g)| / count, with |d| = sqrt((d0 d0 + d1 d1) + d2 d2) and count as a double.
 *      centre   mu_p = SUM p / count, mu_g = SUM g / count (per coordinate); x = p - mu_p, y = g - mu_g.
 *      moments  in a second pass M[r][c] = SUM y_r x_c, var = SUM ((x0 x0 + x1 x1) + x2 x2).
 *      special  var == 0 (no extent in the source; count == 1): R = I, s = 1.
 *      SVD      of M = [c0 c1 c2] V^T by cyclic one-sided Jacobi on the columns of A = M and V = I.  A sweep visits the column pairs
 *               (p,q) = (0,1), (0,2), (1,2); with dot(u,v) = (u0 v0 + u1 v1) + u2 v2: a = dot(A_p,A_p), b = dot(A_q,A_q), g = dot(A_p,A_q).
 *               The pair is SKIPPED when |g| <= 2^-50 max(a, b): the rotation left undone is by less than 2^-50.  (The relative test
 *               |g| <= eps sqrt(a b) never fires against a column that is rounding noise of a larger one -- a coplanar or collinear set
 *               -- since every rotation renews the noise; this one does, a zero column (a b == 0, so g == 0) included, and forms no
 *               product a b that could underflow or overflow.  The small columns are left orthogonal to the large ones only to 2^-50 of
 *               the LARGE norm: U1 is re-orthogonalised below, and of c2 only the norm and one sign are used.)  Otherwise h = b - a,
 *               g2 = 2 g and
 *                   |g2| <= |h|:  r = g2 / h,  t = r / (1 + sqrt(1 + r r))
 *                   else:         z = h / g2,  u = 1 / (|z| + sqrt(1 + z z)),  t = -u if z < 0 else u
 *               (the smaller root of t^2 + 2 zeta t - 1 = 0 with zeta = h / g2, formed from whichever of zeta and 1 / zeta is at most 1
 *               in magnitude, so nothing overflows), cs = 1 / sqrt(1 + t t), sn = cs t, and for A and for V, per row:
 *               new_p = cs old_p - sn old_q, new_q = sn old_p + cs old_q.  The loop ends after the first sweep that skipped all three
 *               pairs, at the latest after H3D_MESH_EVAL_MAX_SWEEPS sweeps.
 *      order    nn_j = dot(A_j,A_j); the columns by nn descending through the compare-exchanges (0,1), (1,2), (0,1), each swapping only
 *               when the later one is strictly larger (a tie keeps the lower original column first); dv = -1 for an odd number of
 *               swaps else 1: det V (the rotations have determinant 1).  S_j = sqrt(nn_j), c_j and V_j in that order.
 *      rank 0   S0 == 0 (every target point at its centroid): R = I, s = 0.
 *      U        U0 = c0 / S0.  U1: if S1 > 0, u = c1 / S1, hh = dot(u,U0), w = u - hh U0, nw = |w|, and U1 = w / nw when nw >= 0.5;
 *               else (rank 1, a collinear set) k = the coordinate where |U0| is least (the first of equals), w = e_k - U0[k] U0,
 *               U1 = w / |w|.  U2 = U0 x U1 (U2[0] = U0[1] U1[2] - U0[2] U1[1], cyclic).
 *      R, s, t  R[r][c] = (U0[r] V0[c] + U1[r] V1[c]) + dv (U2[r] V2[c]): a rotation for every rank, without a direction from a vanishing
 *               third column.  d = -dv if dot(c2,U2) < 0 else dv;  s = ((S0 + S1) + d S2) / var;
 *               t[r] = mu_g[r] - s ((R[r][0] mu_p[0] + R[r][1] mu_p[1]) + R[r][2] mu_p[2]).
 *      aligned  err[k,1] = SUM |q - g| / count with q[r] = s ((R[r][0] p0 + R[r][1] p1) + R[r][2] p2) + t[r], in a third pass.
 *    err [P,2] f64, count [P] i32, transform [P,13] f64 or NULL: s, R row-major, t.  No NaN or Inf for finite inputs.
 *    n <= 0, P < 0, Np < 0, Ng < 0, 3 n or 3 nr >= 2^31, one root source without the other, a root index outside [0,nr), a NULL required
 *    operand, an fp64 pointer off an 8-byte boundary: H3D_ERR_ARG, checked before the first HIP call.  P == 0: nothing is launched.
 *
 *    h3d_metric_means, one wave.  err [P,2] f64, count [P] i32 -> means [2] f64 = the means of err[:,0] and err[:,1] over the pairs with
 *    count > 0, n_pairs [1] i32 = their number (0: both means are 0).  Lane l starts at 0.0 and adds its pairs l, l + 64, ... in
 *    ascending order, then the wave tree of SUM; the sum is divided by n_pairs as a double.  P == 0 writes zeros.  Errors as above.
 * ===================================================================================== */
#define H3D_MESH_EVAL_MAX_SWEEPS 30
int h3d_pointset_errors(const float *pred, int Np, const float *gt, int Ng, int n, const int32_t *pred_idx, const int32_t *gt_idx, int P,
                        const uint8_t *weight, const float *pred_root, const float *gt_root, int nr, int root_a, int root_b, double *err,
                        int32_t *count, double *transform, void *stream);
int h3d_metric_means(const double *err, const int32_t *count, int P, double *means, int32_t *n_pairs, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* H3D_H */
