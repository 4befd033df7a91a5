/*
 * detops.h — C ABI of libdetops_gfx950.so, the MI355X (gfx950 / CDNA4) detection-head
 * operator library.
 *
 * This is the drop-in boundary for the hot path of facebookresearch/maskrcnn-benchmark:
 * every entry point below replaces one function of the reference's pybind module
 * `maskrcnn_benchmark._C` (reference: maskrcnn_benchmark/csrc/vision.cpp:9-25), which the
 * reference's `maskrcnn_benchmark.layers` package binds.  The host side that re-exports the
 * exact 14-name `_C` surface on top of this ABI is
 * `maskrcnn-benchmark_amd/maskrcnn_benchmark/_C.py` (ctypes).
 *
 * Conventions
 *   - All pointers are DEVICE pointers (HBM) unless the name ends in `_host`.
 *   - Tensors are dense, contiguous, NCHW, fp32 unless the function name says otherwise.
 *   - `stream` is a `hipStream_t` passed as `void*` (0 = the null stream).  Every launch goes
 *     to that stream; no entry point synchronises the host, allocates or frees device memory
 *     (scratch comes from caller-provided workspaces sized by the *_workspace_bytes queries),
 *     so every call is hipGraph-capturable and re-entrant per stream.
 *   - Return value: 0 on success, a positive hipError_t if a HIP call failed, or one of the
 *     negative DETOPS_E* codes for argument errors.  Nothing is written on error.
 *   - ROI rows are (batch_index, x1, y1, x2, y2) in image coordinates, batch index stored as
 *     float (reference: maskrcnn_benchmark/modeling/poolers.py:78-89).
 */
#ifndef DETOPS_H_
#define DETOPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DETOPS_ABI_VERSION 1

#define DETOPS_EINVAL   (-1) /* bad shape / null pointer / negative size            */
#define DETOPS_EWORKSPACE (-2) /* workspace too small (see *_workspace_bytes)       */
#define DETOPS_EUNSUPPORTED (-3) /* configuration outside what the kernels implement */
#define DETOPS_EGTCAP   (-4) /* detops_eval_match only: some problem has more than DETOPS_EVAL_MAX_GT ground truths */

typedef void* detops_stream_t; /* hipStream_t */

/* Library identification: returns DETOPS_ABI_VERSION; `arch` (may be NULL) receives a static
 * string naming the ISA the device code was built for ("gfx950"). */
int detops_version(const char** arch);

/* Tuning / test switches (all default 0 = automatic).  Read once at library load from the environment variable
 * DETOPS_TUNING="key=value,key=value"; this call changes one at run time (tests, A/B measurements — process-wide,
 * not thread-safe against concurrent launches).  The launch paths never read the environment.  Keys:
 *   roi_bwd_impl      1 ring (needs a workspace) | 2 scan | 3 atomic scatter
 *   roi_bwd_seg       ring: hits per hit-list segment (default 32, >= 8)
 *   roi_bwd_groups    scan: ROI-list split        roi_bwd_scan_ct   scan: channels per workgroup (4 | 16)
 *   roi_bwd_debug     ablation bits (1 = skip the walk)
 *   roi_fwd_impl      1 generic gather kernel    roi_fwd_order     1 never rank | 2 rank even tiny maps
 *   roi_fwd_order_mink  smallest K that gets the ranking pre-pass
 *   dcn_col2im        1 gather | 2 scatter | 3 ell    dcn_fused  1 force | 2 off    dcn_gather_xcd  1 plain block order
 *   dcn_nhwc          2 = never use the channels-last pipeline (the layers then run the reference-layout kernels)
 * Returns 0, or DETOPS_EINVAL for an unknown key. */
int detops_tuning_set(const char* key, int value);
int detops_tuning_get(const char* key, int* value);

/* ------------------------------------------------------------------------------------------
 * ROIAlign  — replaces _C.roi_align_forward / _C.roi_align_backward
 *   reference: csrc/ROIAlign.h:11-25 (forward), :27-45 (backward);
 *              csrc/cpu/ROIAlign_cpu.cpp:113-257, csrc/cuda/ROIAlign_cuda.cu:64-122,177-346.
 *   input  [N,C,H,W]   rois [K,5]   output / grad_out [K,C,PH,PW]   grad_in [N,C,H,W]
 *   sampling_ratio <= 0 selects the adaptive grid ceil(roi_h/PH) x ceil(roi_w/PW).
 *   backward: `zero_grad_in` != 0 makes the call zero-fill grad_in first (the reference
 *   allocates it with at::zeros, ROIAlign_cuda.cu:316); 0 accumulates into the caller's buffer
 *   (used by the multi-level pooler to fuse several ROI sets into one gradient map).
 * ---------------------------------------------------------------------------------------- */
int detops_roi_align_forward_f32(const float* input, const float* rois, float* output,
                                 int N, int C, int H, int W, int K, int PH, int PW,
                                 float spatial_scale, int sampling_ratio,
                                 detops_stream_t stream);

int detops_roi_align_backward_f32(const float* grad_out, const float* rois, float* grad_in,
                                  int N, int C, int H, int W, int K, int PH, int PW,
                                  float spatial_scale, int sampling_ratio, int zero_grad_in,
                                  detops_stream_t stream);

/* Forward with a caller-provided workspace (`detops_roi_align_forward_workspace_bytes(K, PH, PW, sampling_ratio)`
 * bytes; 0 = not used for this shape): ONE pre-pass launch (a) builds per-ROI sample records — footprint bounds and,
 * per output bin, the patch offsets and bilinear weights of its samples by the reference arithmetic — which every
 * channel-chunk workgroup of the main launch loads instead of re-deriving, and (b) for K >= 384 ranks the ROIs by
 * (level, image, position) so that the main launch visits overlapping footprints while they are still in the XCD's
 * L2.  The output is identical, bit for bit, to the workspace-free call (what detops_roi_align_forward_f32 /
 * detops_roi_align_fpn_forward_f32 do); workspace == NULL or too small selects that path. */
size_t detops_roi_align_forward_workspace_bytes(int K, int PH, int PW, int sampling_ratio);

int detops_roi_align_forward_ws_f32(const float* input, const float* rois, float* output,
                                    int N, int C, int H, int W, int K, int PH, int PW,
                                    float spatial_scale, int sampling_ratio, void* workspace,
                                    size_t workspace_bytes, detops_stream_t stream);

/* Backward with a caller-provided workspace: selects the binned pixel-owner kernel (a pre-pass launch
 * builds per-ROI adjoint rows and per-tile hit lists in the workspace, the main launch only gathers).
 * `detops_roi_align_backward_workspace_bytes` returns the size for a set of maps (H_host/W_host:
 * num_levels entries; 1 for the single-map call), or 0 when the shape is served by the
 * workspace-free kernels.  workspace == NULL or too small: same result through the workspace-free
 * path (what detops_roi_align_backward_f32 / detops_roi_align_fpn_backward_f32 do). */
size_t detops_roi_align_backward_workspace_bytes(const int* H_host, const int* W_host,
                                                 int num_levels, int N, int C, int K, int PH, int PW);

int detops_roi_align_backward_ws_f32(const float* grad_out, const float* rois, float* grad_in,
                                     int N, int C, int H, int W, int K, int PH, int PW,
                                     float spatial_scale, int sampling_ratio, int zero_grad_in,
                                     void* workspace, size_t workspace_bytes,
                                     detops_stream_t stream);

/* Multi-level (FPN) ROIAlign in ONE launch — the sync-free form of
 * modeling/poolers.py:91-121 (LevelMapper :11-42 + per-level ROIAlign :116-119).
 *   inputs[l] : device pointer to level l's feature map [N,C,H[l],W[l]], scale[l] its stride^-1
 *   rois [K,5]; the FPN level of each ROI is computed on device with the reference's formula
 *   lvl = clamp(floor(canonical_level + log2(sqrt(area)/canonical_scale + eps)), k_min, k_max)
 *   with area = (x2-x1+1)*(y2-y1+1)  (structures/bounding_box.py:212-216, TO_REMOVE = 1).
 *   `levels_out` (may be NULL) receives the 0-based level index per ROI as int32.
 *   num_levels <= DETOPS_MAX_LEVELS.  The pointer/shape arrays are HOST arrays (copied into
 *   the kernel argument block).
 */
#define DETOPS_MAX_LEVELS 8
int detops_roi_align_fpn_forward_f32(const float* const* inputs_host, const int* H_host,
                                     const int* W_host, const float* scale_host,
                                     int num_levels, const float* rois, float* output,
                                     int32_t* levels_out, int N, int C, int K, int PH, int PW,
                                     int sampling_ratio, int k_min, int k_max,
                                     float canonical_scale, float canonical_level, float eps,
                                     detops_stream_t stream);

int detops_roi_align_fpn_forward_ws_f32(const float* const* inputs_host, const int* H_host,
                                        const int* W_host, const float* scale_host,
                                        int num_levels, const float* rois, float* output,
                                        int32_t* levels_out, int N, int C, int K, int PH, int PW,
                                        int sampling_ratio, int k_min, int k_max,
                                        float canonical_scale, float canonical_level, float eps,
                                        void* workspace, size_t workspace_bytes,
                                        detops_stream_t stream);

int detops_roi_align_fpn_backward_ws_f32(const float* grad_out, const float* rois,
                                         const int32_t* levels, float* const* grad_inputs_host,
                                         const int* H_host, const int* W_host,
                                         const float* scale_host, int num_levels, int N, int C,
                                         int K, int PH, int PW, int sampling_ratio,
                                         int zero_grad_in, void* workspace, size_t workspace_bytes,
                                         detops_stream_t stream);

/* The binned backward in two calls.  Its pre-pass (per-ROI adjoint rows + per-tile hit lists) depends on the ROIs and the
 * map shapes only: `..._prepare_f32` may be issued at FORWARD time, on any stream, into a workspace of
 * detops_roi_align_backward_workspace_bytes(...) bytes that the caller keeps until the backward pass; `..._prepared_f32`
 * (same shapes, same workspace, stream-ordered after the prepare call) then launches the main kernel alone.  `prepare`
 * returns DETOPS_EUNSUPPORTED when the shape is served by the other kernels: use detops_roi_align_fpn_backward_ws_f32. */
int detops_roi_align_fpn_backward_prepare_f32(const float* rois, const int32_t* levels, const int* H_host,
                                              const int* W_host, const float* scale_host, int num_levels, int N,
                                              int C, int K, int PH, int PW, int sampling_ratio, void* workspace,
                                              size_t workspace_bytes, detops_stream_t stream);

int detops_roi_align_fpn_backward_prepared_f32(const float* grad_out, float* const* grad_inputs_host,
                                               const int* H_host, const int* W_host, const float* scale_host,
                                               int num_levels, int N, int C, int K, int PH, int PW,
                                               int zero_grad_in, void* workspace, size_t workspace_bytes,
                                               detops_stream_t stream);

int detops_roi_align_fpn_backward_f32(const float* grad_out, const float* rois,
                                      const int32_t* levels, float* const* grad_inputs_host,
                                      const int* H_host, const int* W_host,
                                      const float* scale_host, int num_levels, int N, int C,
                                      int K, int PH, int PW, int sampling_ratio,
                                      int zero_grad_in, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ROIAlign over a CHANNELS-LAST pyramid (csrc/roi_align_nhwc.hip) — the same operator as above (reference
 * csrc/cuda/ROIAlign_cuda.cu:64-122 forward, :125-254 backward, modeling/poolers.py:91-121) for feature maps stored
 * [N, H[l], W[l], C] (what MIOpen's implicit-GEMM convolutions read and write natively: a detector whose backbone runs
 * channels-last needs no layout transposes around its pooler).  num_levels == 1 is the single-map operator.
 *   forward : inputs[l] NHWC; output [K, C, PH, PW] (output_nhwc = 0) or [K, PH, PW, C] (output_nhwc = 1).  Reference
 *             operation order with FP contraction off: bit-identical to the reference CPU kernel (and to the NCHW
 *             kernels above) for finite inputs.  workspace (detops_roi_align_fpn_forward_nhwc_workspace_bytes(K) bytes,
 *             may be NULL): the ROI visiting order (L2 locality only; the output does not depend on it).
 *   backward: grad_out [K, C, PH, PW] (grad_out_nhwc = 0) or [K, PH, PW, C] (1); grad_inputs[l] NHWC, every element
 *             written exactly once (zero_grad_in = 1) or added to (0); atomic-free, bit-reproducible run to run;
 *             `levels` = the forward's levels_out (required when num_levels > 1); workspace REQUIRED
 *             (detops_roi_align_fpn_backward_nhwc_workspace_bytes: per-ROI adjoint rows + per-tile hit lists).
 * ---------------------------------------------------------------------------------------- */
size_t detops_roi_align_fpn_forward_nhwc_workspace_bytes(int K);
int detops_roi_align_fpn_forward_nhwc_f32(const float* const* inputs_host, const int* H_host, const int* W_host,
                                          const float* scale_host, int num_levels, const float* rois, float* output,
                                          int output_nhwc, int32_t* levels_out, int N, int C, int K, int PH, int PW,
                                          int sampling_ratio, int k_min, int k_max, float canonical_scale,
                                          float canonical_level, float eps, void* workspace, size_t workspace_bytes,
                                          detops_stream_t stream);
/* The pixel-owner ring backward (csrc/roi_align_bwd.hip) with channels-last gradient maps: same kernels, the store epilogue
 * writes a thread's channel sums as consecutive floats.  grad_out [K, C, PH, PW]; workspace of
 * detops_roi_align_backward_workspace_bytes(...) bytes.  DETOPS_EUNSUPPORTED when the ring plan does not serve the shape
 * (small / under-filled maps, other bin counts): use detops_roi_align_fpn_backward_nhwc_f32 then. */
int detops_roi_align_fpn_backward_ring_nhwc_f32(const float* grad_out, const float* rois, const int32_t* levels,
                                                float* const* grad_inputs_host, const int* H_host, const int* W_host,
                                                const float* scale_host, int num_levels, int N, int C, int K, int PH,
                                                int PW, int sampling_ratio, int zero_grad_in, void* workspace,
                                                size_t workspace_bytes, detops_stream_t stream);
size_t detops_roi_align_fpn_backward_nhwc_workspace_bytes(const int* H_host, const int* W_host, int num_levels, int N,
                                                          int C, int K, int PH, int PW);
int detops_roi_align_fpn_backward_nhwc_f32(const float* grad_out, int grad_out_nhwc, const float* rois,
                                           const int32_t* levels, float* const* grad_inputs_host, const int* H_host,
                                           const int* W_host, const float* scale_host, int num_levels, int N, int C,
                                           int K, int PH, int PW, int sampling_ratio, int zero_grad_in, void* workspace,
                                           size_t workspace_bytes, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ROIPool — replaces _C.roi_pool_forward / _C.roi_pool_backward
 *   reference: csrc/ROIPool.h:11-45, csrc/cuda/ROIPool_cuda.cu:16-108 (CUDA-only there).
 *   argmax [K,C,PH,PW] int32: index h*W+w inside the channel plane, -1 for an empty bin.
 * ---------------------------------------------------------------------------------------- */
int detops_roi_pool_forward_f32(const float* input, const float* rois, float* output,
                                int32_t* argmax, int N, int C, int H, int W, int K, int PH,
                                int PW, float spatial_scale, detops_stream_t stream);

int detops_roi_pool_backward_f32(const float* grad_out, const float* rois,
                                 const int32_t* argmax, float* grad_in, int N, int C, int H,
                                 int W, int K, int PH, int PW, int zero_grad_in,
                                 detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * NMS — replaces _C.nms
 *   reference: csrc/nms.h:10-28, csrc/cpu/nms_cpu.cpp:5-75 (the CPU semantics are the
 *   contract: suppress j iff IoU(i,j) >= threshold, +1 pixel convention, result = kept
 *   ORIGINAL indices in ascending order, int64).
 *   boxes [n,4] xyxy fp32, scores [n] fp32.  Sort order: score descending, ties broken by
 *   ascending original index (stable).
 *   keep      [n]  int64, first *num_keep entries valid (ascending original indices)
 *   num_keep  [1]  int32 on device (the caller decides when/if to read it back); -1 = FAILED: a workgroup of the
 *                  single-launch kernel waited for another one of the same launch beyond its polling budget (seconds:
 *                  the compute units were held by other work).  The repair pass described at
 *                  detops_nms_batched_status_f32 redoes such a segment before the call's work ends, so a caller only ever
 *                  SEES -1 (and an all-zero keep mask) with the repair switched off (tuning "nms_no_repair" = 1: tests)
 *   Entirely device-side: no host round trip (the reference's CUDA path copies the n x n/64
 *   bitmask to the host and scans it there, csrc/cuda/nms.cu:100-123).
 * ---------------------------------------------------------------------------------------- */
size_t detops_nms_workspace_bytes(int n);

int detops_nms_f32(const float* boxes, const float* scores, int n, float threshold,
                   int64_t* keep, int32_t* num_keep, void* workspace, size_t workspace_bytes,
                   detops_stream_t stream);

/* Batched / segmented NMS: S independent problems in one launch sequence (the RPN's
 * per-(image, level) loop, modeling/rpn/inference.py:111-121, and the per-class loop of
 * modeling/roi_heads/box_head/inference.py:122-135).
 *   seg_offsets [S+1] int32 on device: segment s owns rows seg_offsets[s] .. seg_offsets[s+1]-1
 *   of boxes/scores; max_n >= the longest segment (host-known upper bound).
 *   keep [total] int64: segment s writes its kept indices (LOCAL to the segment, ascending)
 *   at keep[seg_offsets[s] ...]; num_keep [S] int32.
 */
size_t detops_nms_batched_workspace_bytes(int num_segments, int max_n);

int detops_nms_batched_f32(const float* boxes, const float* scores,
                           const int32_t* seg_offsets, int num_segments, int max_n,
                           float threshold, int64_t* keep, int32_t* num_keep, void* workspace,
                           size_t workspace_bytes, detops_stream_t stream);

/* Same computation, dense result: keep_mask [total] uint8, keep_mask[seg_offsets[s] + i] = 1 iff
 * box i of segment s survives.  Fixed-shape output for callers that never read a count back
 * (the padded RPN proposal path; replaces the `keep` index list + nonzero of
 * modeling/rpn/inference.py:111-121). */
int detops_nms_batched_mask_f32(const float* boxes, const float* scores,
                                const int32_t* seg_offsets, int num_segments, int max_n,
                                float threshold, uint8_t* keep_mask, int32_t* num_keep,
                                void* workspace, size_t workspace_bytes, detops_stream_t stream);

/* Both result forms optional (keep and / or keep_mask, at least one) + a sticky STATUS word.  Every entry point of this
 * section launches, right behind the single-launch kernel and on the same stream, a repair pass: a segment the single
 * launch marked as failed (num_keep = -1, see above) is redone by ONE workgroup that waits for nobody, so that — like the
 * reference (csrc/cuda/nms.cu:70-131) — no segment is ever dropped; num_keep[s] then holds the real count.  *status
 * (int32 on device, may be NULL; never cleared by the library) is incremented once per redone segment: a trainer reads it
 * with its next loss read-back and reports how often the fast path gave up — no synchronisation of its own. */
int detops_nms_batched_status_f32(const float* boxes, const float* scores, const int32_t* seg_offsets,
                                  int num_segments, int max_n, float threshold, int64_t* keep, uint8_t* keep_mask,
                                  int32_t* num_keep, int32_t* status, void* workspace, size_t workspace_bytes,
                                  detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SigmoidFocalLoss — replaces _C.sigmoid_focalloss_forward / _backward
 *   reference: csrc/SigmoidFocalLoss.h:10-41, csrc/cuda/SigmoidFocalLoss_cuda.cu:20-101.
 *   logits [R,C] fp32, targets [R] int32 in {-1 ignore, 0 background, 1..C}, losses [R,C].
 *   `_sum` additionally (or only, if losses == NULL) accumulates sum(losses) into *loss_sum
 *   (fp32, device; must be zeroed by the caller) — what layers/sigmoid_focal_loss.py:66-67
 *   does with a separate .sum().
 * ---------------------------------------------------------------------------------------- */
int detops_sigmoid_focal_loss_forward_f32(const float* logits, const int32_t* targets,
                                          float* losses, int R, int C, float gamma,
                                          float alpha, detops_stream_t stream);

int detops_sigmoid_focal_loss_backward_f32(const float* logits, const int32_t* targets,
                                           const float* d_losses, float* d_logits, int R,
                                           int C, float gamma, float alpha,
                                           detops_stream_t stream);

/* backward of the summed loss: every element shares ONE upstream gradient, read from the device
 * scalar *d_loss_scalar (no [R,C] broadcast buffer). */
int detops_sigmoid_focal_loss_backward_scalar_f32(const float* logits, const int32_t* targets,
                                                  const float* d_loss_scalar, float* d_logits,
                                                  int R, int C, float gamma, float alpha,
                                                  detops_stream_t stream);

int detops_sigmoid_focal_loss_forward_sum_f32(const float* logits, const int32_t* targets,
                                              float* losses /* nullable */, float* loss_sum,
                                              int R, int C, float gamma, float alpha,
                                              detops_stream_t stream);

/* As _forward_sum, but workgroup partial sums are spread over `num_slots` words
 * (partial_sums[num_slots], zeroed by the caller; sum(losses) = sum of the slots): thousands of
 * workgroups retiring together on one word serialise in L2. */
int detops_sigmoid_focal_loss_forward_partial_sums_f32(const float* logits, const int32_t* targets,
                                                       float* losses /* nullable */,
                                                       float* partial_sums, int num_slots, int R,
                                                       int C, float gamma, float alpha,
                                                       detops_stream_t stream);

/* Two-stage, atomic-free form of _forward_sum: stage 1 leaves one sum per workgroup in `workspace`
 * (`detops_sigmoid_focal_loss_sum_workspace_bytes()` bytes, need not be initialised), stage 2 adds them in a fixed
 * order and OVERWRITES loss_sum[0] — no zero-fill launch, no host-side reduction, bit-reproducible run to run. */
size_t detops_sigmoid_focal_loss_sum_workspace_bytes(void);
int detops_sigmoid_focal_loss_forward_sum_ws_f32(const float* logits, const int32_t* targets,
                                                 float* losses, float* loss_sum, int R, int C,
                                                 float gamma, float alpha, void* workspace,
                                                 size_t workspace_bytes, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Deformable convolution building blocks — the kernels behind _C.deform_conv_forward,
 * _backward_input, _backward_parameters, _C.modulated_deform_conv_forward/_backward
 *   reference: csrc/deform_conv.h:11-191, csrc/cuda/deform_conv_kernel_cuda.cu:197-874,
 *              host orchestration csrc/cuda/deform_conv_cuda.cu:158-691.
 *   dtype: 0 = fp32, 1 = fp16, 2 = bf16 (all buffers share it; interpolation runs in fp32).
 *   im       [B, C, H, W]
 *   offset   [B, dg*2*kh*kw, Ho, Wo]   channel 2*(i*kw+j) = dh, +1 = dw
 *   mask     [B, dg*kh*kw,   Ho, Wo]   NULL selects the v1 (un-modulated) operator
 *   col      [C*kh*kw, B*Ho*Wo]        row (c*kh+i)*kw+j, column (b*Ho+ho)*Wo+wo
 *   col2im accumulates into grad_im (caller zero-fills, as deform_conv_func.py:88 does);
 *   col2im_coord overwrites grad_offset (and grad_mask when mask != NULL).
 * ---------------------------------------------------------------------------------------- */
#define DETOPS_F32 0
#define DETOPS_F16 1
#define DETOPS_BF16 2

int detops_deformable_im2col(const void* im, const void* offset, const void* mask, void* col,
                             int dtype, int B, int C, int H, int W, int kh, int kw, int pad_h,
                             int pad_w, int stride_h, int stride_w, int dil_h, int dil_w,
                             int deformable_group, detops_stream_t stream);

int detops_deformable_col2im(const void* col, const void* offset, const void* mask,
                             void* grad_im, int dtype, int B, int C, int H, int W, int kh,
                             int kw, int pad_h, int pad_w, int stride_h, int stride_w,
                             int dil_h, int dil_w, int deformable_group,
                             detops_stream_t stream);

/* col2im without atomics on the data: the scatter pattern (shared by all channels of a deformable
 * group) is inverted once per call into per-pixel gather lists held in a caller workspace
 * (>= detops_deformable_col2im_workspace_bytes(...) bytes, device memory, any contents); each
 * gradient pixel is then summed in registers in a fixed order (deterministic).  A NULL / too
 * small workspace, or a shape beyond the 32-bit index plan (workspace_bytes() == 0), runs the
 * atomic scatter kernels of detops_deformable_col2im instead. */
size_t detops_deformable_col2im_workspace_bytes(int B, int C, int H, int W, int kh, int kw,
                                                int pad_h, int pad_w, int stride_h, int stride_w,
                                                int dil_h, int dil_w, int deformable_group);

int detops_deformable_col2im_ws(const void* col, const void* offset, const void* mask,
                                void* grad_im, int dtype, int B, int C, int H, int W, int kh,
                                int kw, int pad_h, int pad_w, int stride_h, int stride_w,
                                int dil_h, int dil_w, int deformable_group, void* workspace,
                                size_t workspace_bytes, detops_stream_t stream);

int detops_deformable_col2im_coord(const void* col, const void* im, const void* offset,
                                   const void* mask, void* grad_offset, void* grad_mask,
                                   int dtype, int B, int C, int H, int W, int kh, int kw,
                                   int pad_h, int pad_w, int stride_h, int stride_w, int dil_h,
                                   int dil_w, int deformable_group, detops_stream_t stream);

/* Fused deformable-convolution FORWARD: one implicit GEMM on the matrix cores
 * (v_mfma_f32_32x32x16_{f16,bf16}); the deformed operand tile is built in LDS, `columns` is never written.
 * Replaces the im2col + GEMM sequence of csrc/cuda/deform_conv_cuda.cu:228-245 / :520-560 for 16-bit storage,
 * convolution groups == 1 and (C / deformable_group) % 32 == 0; other shapes return DETOPS_EUNSUPPORTED
 * (workspace_bytes() == 0) and the caller runs detops_deformable_im2col + its GEMM.
 *   im [B,C,H,W], weight [Cout,C,kh,kw], offset / mask as above (mask NULL = v1), bias [Cout] or NULL,
 *   out [B,Cout,Ho,Wo]; all of `dtype`.  workspace: NHWC copy of im + tap-major copy of weight. */
size_t detops_deform_conv_forward_fused_workspace_bytes(int dtype, int B, int C, int H, int W, int Cout,
                                                        int kh, int kw, int pad_h, int pad_w, int stride_h,
                                                        int stride_w, int dil_h, int dil_w,
                                                        int deformable_group);

int detops_deform_conv_forward_fused(const void* im, const void* weight, const void* offset,
                                     const void* mask, const void* bias, void* out, int dtype, int B, int C,
                                     int H, int W, int Cout, int kh, int kw, int pad_h, int pad_w,
                                     int stride_h, int stride_w, int dil_h, int dil_w, int deformable_group,
                                     void* workspace, size_t workspace_bytes, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Deformable position-sensitive ROI pooling — replaces _C.deform_psroi_pooling_forward /
 * _C.deform_psroi_pooling_backward
 *   reference: csrc/deform_pool.h:11-70, csrc/cuda/deform_pool_cuda.cu:38-87,
 *              csrc/cuda/deform_pool_kernel_cuda.cu:31-364 (CUDA-only there).
 *   data [N,C,H,W] with C >= output_dim * group_size^2, rois [K,5],
 *   trans [K, channels_trans, part_size, part_size] (NULL when no_trans; channels_trans = 2 *
 *   num_classes, output_dim must be a multiple of num_classes),
 *   out / top_count / out_grad [K, output_dim, pooled_size, pooled_size] (top_count holds the
 *   number of in-bounds samples of each bin as float, like the reference).
 *   backward: `zero_grads` != 0 zero-fills data_grad and trans_grad first (the reference's caller
 *   passes torch.zeros_like buffers, layers/dcn/deform_pool_func.py:72-73); the kernel accumulates.
 * ---------------------------------------------------------------------------------------- */
int detops_deform_psroi_pool_forward_f32(const float* data, const float* rois, const float* trans,
                                         float* out, float* top_count, int N, int C, int H, int W,
                                         int K, int channels_trans, int no_trans,
                                         float spatial_scale, int output_dim, int group_size,
                                         int pooled_size, int part_size, int sample_per_part,
                                         float trans_std, detops_stream_t stream);

int detops_deform_psroi_pool_backward_f32(const float* out_grad, const float* data,
                                          const float* rois, const float* trans,
                                          const float* top_count, float* data_grad,
                                          float* trans_grad, int N, int C, int H, int W, int K,
                                          int channels_trans, int no_trans, float spatial_scale,
                                          int output_dim, int group_size, int pooled_size,
                                          int part_size, int sample_per_part, float trans_std,
                                          int zero_grads, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-target assignment on the device (extensions; the reference does these with ATen compositions
 * and host round trips: SURVEY.md section 8 rows f2 / f3).
 *
 * detops_match_boxes_f32 — IoU + Matcher fused (structures/boxlist_ops.py:53-89, modeling/matcher.py:42-112):
 *   gt_boxes [N, M, 4] xyxy fp32 (padded rows flagged 0 in gt_valid [N, M] uint8), boxes [K, 4] shared by
 *   the N images (boxes_batched = 0) or [N, K, 4]; matched_idxs [N, K] int64 = arg-max ground truth (first
 *   index among ties), -1 below low_threshold, -2 between the thresholds; with allow_low_quality_matches every
 *   box attaining some valid ground truth's maximum IoU keeps its arg-max.  The [M, K] matrix is never stored.
 *   workspace (only with the low-quality rule): >= detops_match_boxes_workspace_bytes(N, M).
 *
 * detops_sample_labels — BalancedPositiveNegativeSampler (modeling/balanced_positive_negative_sampler.py:19-68):
 *   labels [N, n] (label_dtype: fp32 or int64; >= 1 positive, 0 negative, < 0 ignored); per row a uniformly
 *   random subset of min(#pos, max_positives) positives and min(#neg, B - that) negatives, as 0/1 masks
 *   [N, n] and (optional, both or neither) a fixed-length list sampled_idx / sampled_valid [N, B], positives
 *   first.  Deterministic in (labels, seed); B <= 512.
 *
 * detops_mask_targets — mask-head targets (roi_heads/mask_head/loss.py:11-42 via
 *   structures/segmentation_mask.py:118-158): for ROI p crop instance mask_index[p] of masks [G, H, W] to the
 *   rounded, clamped box and resize bilinearly (align_corners = False) to M x M; integer masks truncate the
 *   interpolated value, bool masks map non-zero to 1.  out [P, M, M] fp32.
 * ---------------------------------------------------------------------------------------- */
#define DETOPS_LABEL_F32 0
#define DETOPS_LABEL_I64 1
#define DETOPS_MASK_U8 0
#define DETOPS_MASK_F32 1
#define DETOPS_MASK_BOOL 2

size_t detops_match_boxes_workspace_bytes(int N, int M);

int detops_match_boxes_f32(const float* gt_boxes, const uint8_t* gt_valid, const float* boxes,
                           int boxes_batched, int N, int M, int K, float high_threshold,
                           float low_threshold, int allow_low_quality_matches, int64_t* matched_idxs,
                           void* workspace, size_t workspace_bytes, detops_stream_t stream);

size_t detops_sample_labels_workspace_bytes(int N, int batch_size_per_image);

int detops_sample_labels(const void* labels, int label_dtype, int N, int n, int batch_size_per_image,
                         int max_positives, uint64_t seed, uint8_t* pos_mask, uint8_t* neg_mask,
                         int64_t* sampled_idx, uint8_t* sampled_valid, void* workspace,
                         size_t workspace_bytes, detops_stream_t stream);

/* the same with a device word mixed into the seed when the kernels run (NULL: exactly detops_sample_labels): for launches captured
 * into a HIP graph, whose arguments are frozen at capture */
int detops_sample_labels_dseed(const void* labels, int label_dtype, int N, int n, int batch_size_per_image,
                               int max_positives, uint64_t seed, const uint64_t* seed_dev, uint8_t* pos_mask,
                               uint8_t* neg_mask, int64_t* sampled_idx, uint8_t* sampled_valid, void* workspace,
                               size_t workspace_bytes, detops_stream_t stream);

int detops_mask_targets(const void* masks, int mask_dtype, const int64_t* mask_index, const float* boxes,
                        int G, int H, int W, int P, int M, float* out, detops_stream_t stream);

/* detops_rpn_decode_f32 — the box path of RPN proposal selection for one feature level
 *   (modeling/rpn/inference.py:75-110: gather of the pre-NMS top-k anchors' deltas, BoxCoder.decode —
 *   modeling/box_coder.py:61-95 —, clip_to_image(remove_empty=False) — structures/bounding_box.py:202-213 —,
 *   remove_small_boxes — structures/boxlist_ops.py:34-50 — as a mask): ~35 ATen launches per level in the reference.
 *   box_regression [N, 4A, H, W] fp32 (the head's own layout), topk_idx / topk_scores [N, k] (positions in the
 *   (y, x, a) order of permute_and_flatten, modeling/rpn/utils.py:9-13), anchors [A*H*W, 4] in that order,
 *   image_hw [N, 2] = (height, width) fp32.  Writes boxes [N][.][4] and scores [N][.] at the caller's column offset
 *   (row strides in elements), and this level's slice of the NMS input: nms_boxes [N*k, 4], nms_scores [N*k]
 *   (boxes smaller than min_size are moved far away with score -1), ok [N*k] uint8. */
int detops_rpn_decode_f32(const float* box_regression, const int64_t* topk_idx, const float* topk_scores,
                          const float* anchors, const float* image_hw, int N, int A, int H, int W, int k,
                          float wx, float wy, float ww, float wh, float bbox_xform_clip, float min_size,
                          float* boxes, int64_t boxes_row_stride, float* scores, int64_t scores_row_stride,
                          float* nms_boxes, float* nms_scores, uint8_t* ok, detops_stream_t stream);

/* detops_match_labels — Matcher output -> training labels (modeling/rpn/loss.py:70-88 and
 *   roi_heads/box_head/loss.py:56-72 of the reference: the clamp / gather / three masked assignments per image):
 *   matched [N, K] int64; gt_labels [N, M] int64 or NULL (NULL: every match labels 1, the RPN rule);
 *   valid [N, K] uint8 or NULL (anchor visibility / proposal validity: false -> -1).
 *   out [N, K]: float32 (out_dtype 0) or int64 (out_dtype 1);  >= 0 -> class, -1 -> 0, -2 -> -1. */
int detops_match_labels(const int64_t* matched, const int64_t* gt_labels, const uint8_t* valid, int N, int K, int M,
                        int out_dtype, void* out, detops_stream_t stream);

/* detops_roi_head_targets_f32 — the box head's sampled slots (roi_heads/box_head/loss.py:56-110: labels, BoxCoder.encode of
 *   the matched ground truth — modeling/box_coder.py:27-51 —, the per-image indexing by the sampled positions):
 *   boxes [N, K, 4], matched [N, K], gt_boxes [N, M, 4], gt_labels [N, M], valid [N, K] or NULL, idx / slot_valid [N, B]
 *   (detops_sample_labels' slot list), objectness [N, K] or NULL -> per slot: box [N, B, 4], label [N, B] int64 (-1 for an
 *   unfilled slot), regression target [N, B, 4], matched index [N, B], objectness [N, B] (out_objectness may be NULL). */
int detops_roi_head_targets_f32(const float* boxes, const int64_t* matched, const float* gt_boxes, const int64_t* gt_labels,
                                const uint8_t* valid, const int64_t* idx, const uint8_t* slot_valid, const float* objectness,
                                int N, int K, int M, int B, float wx, float wy, float ww, float wh, float* out_boxes,
                                int64_t* out_labels, float* out_regression_targets, int64_t* out_matched,
                                float* out_objectness, detops_stream_t stream);

/* ---- ROI-head losses: value and gradient in one pass (csrc/head_loss.hip) ------------------------------------------------
 * detops_fastrcnn_loss_f32 — FastRCNNLossComputation.__call__ (roi_heads/box_head/loss.py:140-193 of the reference):
 *   class_logits [R, C], box_regression [R, D] (D = 4C, or >= 8 with cls_agnostic: columns 4..7), labels [R] int64
 *   (-1 = not sampled), regression_targets [R, 4].  losses2 = {cross_entropy(sum over labels >= 0), smooth_l1(beta) summed
 *   over labels > 0 on the class's four columns} / max(#(labels >= 0), 1).  grad_logits [R, C] and grad_box [R, D] receive
 *   d losses2[0] / d class_logits and d losses2[1] / d box_regression (every element written).
 * detops_mask_loss_f32 — MaskRCNNLossComputation.__call__ (roi_heads/mask_head/loss.py:113-143): mask_logits [P, C, M, M],
 *   labels [P] int64 (> 0 = positive), mask_targets [P, M, M] -> loss1 = mean BCE-with-logits between each positive ROI's
 *   class plane and its target (0 without positives); grad_logits [P, C, M, M] fully written.
 * detops_head_loss_backward_f32 — grad_a *= upstream_a[0], grad_b *= upstream_b[0] (device scalars), in place, one launch. */
size_t detops_fastrcnn_loss_workspace_bytes(int R);
int detops_fastrcnn_loss_f32(const float* class_logits, const float* box_regression, const int64_t* labels,
                             const float* regression_targets, int R, int C, int D, int cls_agnostic, float beta,
                             float* grad_logits, float* grad_box, float* losses2, void* workspace, size_t workspace_bytes,
                             detops_stream_t stream);
size_t detops_mask_loss_workspace_bytes(int P);
int detops_mask_loss_f32(const float* mask_logits, const int64_t* labels, const float* mask_targets, int P, int C, int M,
                         float* grad_logits, float* loss1, void* workspace, size_t workspace_bytes, detops_stream_t stream);
int detops_head_loss_backward_f32(float* grad_a, int64_t count_a, const float* upstream_a, float* grad_b, int64_t count_b,
                                  const float* upstream_b, detops_stream_t stream);

/* ---- keypoint head (csrc/keypoint.hip) ---------------------------------------------------------------------------------
 * detops_keypoint_targets — KeypointRCNNLossComputation.prepare_targets + keypoints_to_heat_map (reference
 *   roi_heads/keypoint_head/loss.py:79-100, 145-157; structures/keypoint.py:154-188) for the whole batch in one launch:
 *   boxes [P, 4] xyxy (the slots), matched [P] int64 (row of gt_boxes / gt_keypoints, global across the images; < 0 = none),
 *   labels [P] int64 (> 0 = positive slot), gt_boxes [G, 4] xyxy, gt_keypoints [G, K, 3] (x, y, v).  Per (p, k):
 *   x -> floor((x - x1) * ((1 / (x2 - x1)) * M)) in fp32 without contraction (torch's `M / t` is reciprocal() * M),
 *   x == x2 -> M - 1, the same for y;
 *   valid[p, k] = 0 <= x, y < M  and  v > 0  and  labels[p] > 0  and  gt matched[p] has a keypoint with v > 0 inside its own
 *   box (inclusive edges, loss.py:40-53, 93-98); heatmaps[p, k] = valid ? y * M + x : 0.  heatmaps [P, K] int64,
 *   valid [P, K] uint8.  Bit-equal to the torch formulation.
 * detops_keypoint_loss_f32 — KeypointRCNNLossComputation.__call__ (loss.py:145-169): logits [P, K, H, W] read through the
 *   HOST array logit_strides[4] (elements; NCHW and channels-last alike), heatmaps [P, K] int64 (target pixel y * W + x of
 *   each row), valid [P, K] uint8.  loss1 = sum over the valid rows of the softmax cross-entropy of the row's H * W logits
 *   / max(#valid, 1) — the count formed on the device; 0 without valid rows.  grad_logits (strides grad_strides[4]) fully
 *   written: d loss1 / d logits, 0 on invalid rows.  Accumulation in fp32, sums in a fixed order.  Three launches: the
 *   count, one workgroup per (ROI, keypoint) row (per ROI when the keypoint stride is 1, channels-last), the final
 *   sum; workspace (P * K + 1) floats.
 * detops_heatmaps_to_keypoints_f32 — heatmaps_to_keypoints (roi_heads/keypoint_head/inference.py:40-94) for every
 *   detection of the batch: heatmaps [N, K, H, W] (H * W <= 4096) read through the HOST array strides[4], boxes [N, 4]
 *   xyxy.  Per (n, k): the map resized to ceil(max(w, 1)) x ceil(max(h, 1)) with OpenCV's INTER_CUBIC (A = -0.75,
 *   source (d + 0.5) * in / out - 0.5, border taps clamped, horizontal then vertical pass, fp32), its argmax (row-major,
 *   first maximum) and the value there.  keypoints [N, K, 3] = ((x_int + 0.5) * (w / ceil(w)) + x1, likewise y, 1),
 *   evaluated in fp64 and rounded once to fp32 (numpy's promotion); scores [N, K] = the maximum.  The resized map is
 *   never stored. */
int detops_keypoint_targets(const float* boxes, const int64_t* matched, const int64_t* labels, const float* gt_boxes,
                            const float* gt_keypoints, int P, int G, int K, int M, int64_t* heatmaps, unsigned char* valid,
                            detops_stream_t stream);
size_t detops_keypoint_loss_workspace_bytes(int P, int K);
int detops_keypoint_loss_f32(const float* logits, const int64_t* logit_strides, const int64_t* heatmaps,
                             const unsigned char* valid, int P, int K, int H, int W, float* grad_logits,
                             const int64_t* grad_strides, float* loss1, void* workspace, size_t workspace_bytes,
                             detops_stream_t stream);
int detops_heatmaps_to_keypoints_f32(const float* heatmaps, const int64_t* strides, const float* boxes, int N, int K, int H,
                                     int W, float* keypoints, float* scores, detops_stream_t stream);

/* ---- masks at inference (csrc/masker.hip) ------------------------------------------------------------------------------
 * detops_paste_masks — Masker / paste_mask_in_image (reference roi_heads/mask_head/inference.py:91-199) for every detection
 *   of every image of the batch in one launch.  masks [N, M, M] contiguous (each detection's class channel), dtype code
 *   DETOPS_F32 / F16 / BF16 with fp32 arithmetic (the reference casts to float); boxes [N, 4] fp32 xyxy; det_hw [N, 2]
 *   int32 = (H, W) of the detection's image (the images of a batch differ); out_offset [N] int64 = where detection n's
 *   H x W uint8 plane starts in `out` (bytes, any alignment; 64-bit address arithmetic).  Per detection:
 *     - the map is zero-padded by `padding`; scale = (M + 2 * padding) / M as a Python float, rounded to fp32 by the multiply;
 *     - expand_boxes in fp32 (half sizes and centre, half sizes * scale, centre -+ half size: one rounding each), then the
 *       conversion to int32 by TRUNCATION TOWARD ZERO, not floor: a left edge of -0.4 becomes 0;
 *     - w = max(x2 - x1 + 1, 1), h likewise; the padded map is resized to h x w as ATen's CPU bilinear kernel does with
 *       align_corners = False: source max((d + 0.5) * (float(in) / out) - 0.5, 0), upper index clamped to in - 1, value
 *       hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * c + wx1 * d), every operation one fp32 rounding (no contraction);
 *     - pixel = value > threshold for threshold >= 0, value * 255 != 0 for threshold < 0 (the reference's debugging mode);
 *     - the window [max(x1, 0), min(x2 + 1, W)) x [max(y1, 0), min(y2 + 1, H)) of it lands in an H x W plane of zeros.
 *   The reference has no defined answer for a box whose expanded integer window misses the image (its slice bounds go
 *   negative); THIS LIBRARY'S CHOICE is an all-zero plane.  NaN and coordinates beyond +-5e8 saturate and give that plane.
 *   Every byte of every plane is written exactly once (0 or 1), nothing outside the planes.  DETOPS_EINVAL for
 *   padding < 1 (the reference's expand_masks is not defined there) and for M + 2 * padding > 64; N == 0 is a no-op.
 * detops_paste_masks_rle_count / _write — the same masks (the same per-pixel device function) as UNCOMPRESSED COCO RLE
 *   without the planes: per detection the run lengths over the H x W plane in column-major order, alternating 0-runs and
 *   1-runs and starting with a 0-run.  Canonical: only a detection's first count may be 0 (pixel (0, 0) set), the counts
 *   sum to H * W, an all-zero plane is the single count H * W.  The work is proportional to the clipped windows.
 *     _count: run_offset [N + 1] int64 (device) = exclusive sum of the detections' count numbers;
 *     the caller reads run_offset[N] (the one host read of the path) and allocates counts [run_offset[N]] int32;
 *     _write: fills counts; detection n's are counts[run_offset[n] .. run_offset[n + 1]).
 *   Both calls take the same arguments and the same workspace of detops_paste_masks_rle_workspace_bytes(N, max_w) bytes,
 *   untouched in between; H * W of a detection must stay below 2^31.  max_w must be at least every W of det_hw: the
 *   widths live on the device, so a smaller max_w cannot be refused — such a detection's window is silently CLIPPED to
 *   the columns below max_w (its counts then still sum to H * W; nothing is written out of bounds).
 *   Returns: DETOPS_EINVAL as detops_paste_masks, and for max_w < 1, max_w > 65535 * 32 (one workgroup row per 32
 *   columns) or a null pointer; DETOPS_EWORKSPACE for a workspace smaller than the query's answer.  N == 0: _count
 *   writes run_offset[0] = 0, _write is a no-op. */
int detops_paste_masks(const void* masks, int dtype, const float* boxes, const int32_t* det_hw, const int64_t* out_offset,
                       int N, int M, int padding, float threshold, unsigned char* out, detops_stream_t stream);
size_t detops_paste_masks_rle_workspace_bytes(int N, int max_w);
int detops_paste_masks_rle_count(const void* masks, int dtype, const float* boxes, const int32_t* det_hw, int N, int M,
                                 int padding, float threshold, int max_w, int64_t* run_offset, void* workspace,
                                 size_t workspace_bytes, detops_stream_t stream);
int detops_paste_masks_rle_write(const void* masks, int dtype, const float* boxes, const int32_t* det_hw, int N, int M,
                                 int padding, float threshold, int max_w, const int64_t* run_offset, int32_t* counts,
                                 void* workspace, size_t workspace_bytes, detops_stream_t stream);

/* ---- Compressed RLE strings (csrc/rle_string.hip) ------------------------------------------------------------------------
 * The `counts` string of a COCO results file: a restatement of pycocotools' rleToString, written from knowledge of that
 * code (pycocotools is not installed where this library is built and tested: nobody has run this against it).
 * For the runs c[0 .. m) of one mask (int32, column-major, starting with a 0-run, as detops_paste_masks_rle_write and
 * rle_encode make them):
 *   - for i in order: x = c[i], and x -= c[i - 2] when i > 2.  GREATER THAN 2: runs 0, 1, 2 are coded as they are;
 *   - x is a signed 64-bit value;
 *   - repeat:
 *       1. ch = x & 0x1f
 *       2. x >>= 5 (arithmetic shift)
 *       3. more = (x != -1) if ch & 0x10, else (x != 0)
 *       4. if more, ch |= 0x20
 *       5. emit the byte ch + 48
 *       6. stop when more is false.
 * The number of bytes of one value is the smallest k >= 1 with -2^(5k-1) <= x < 2^(5k-1); the difference of two int32
 * values takes at most 7.  (pycocotools itself reserves 6 per run; every int32 input is coded by the rule above, nothing
 * is refused.)  [16] -> "`0", [0, 5, 3] -> "053", [15, 16, 17, 1] -> "?`0a0A", [1066400] -> "P]aP1".
 *
 * detops_rle_string_count / _write — the strings of N masks from their flat run array: counts [total] int32, run_offset
 *   [N + 1] int64 (run_offset[0] = 0, non-decreasing, run_offset[N] = total; a mask may have no runs: the empty string).
 *     _count: byte_offset [N + 1] int64 (device) = exclusive sum of the strings' lengths;
 *     the caller reads byte_offset[N] (the one host read of the path) and allocates out [byte_offset[N]] uint8;
 *     _write: fills out; mask n's string is out[byte_offset[n] .. byte_offset[n + 1]), no terminator.
 *   Both calls take the same workspace of detops_rle_string_workspace_bytes(total) bytes, untouched in between: the
 *   write call places every chunk from what the count call left there and reads nothing else of the count's results;
 *   byte_offset is in its signature so that the pair reads as count / write of one result, and is only checked for null.
 *   The work is cut by chunks of the flat run array, not by mask; offsets are prefix sums in a fixed order (no atomics): every
 *   byte of out is written exactly once, nothing outside it, and two runs give identical bytes.
 *   Returns: DETOPS_EINVAL for N < 0, total < 0 or a null pointer; DETOPS_EWORKSPACE for a workspace smaller than the
 *   query's answer.  N == 0 or total == 0 returns 0 with nothing launched and nothing written (the caller's byte_offset
 *   is then all zeros by its own doing). */
size_t detops_rle_string_workspace_bytes(int64_t total);
int detops_rle_string_count(const int32_t* counts, const int64_t* run_offset, int64_t total, int N, int64_t* byte_offset,
                            void* workspace, size_t workspace_bytes, detops_stream_t stream);
int detops_rle_string_write(const int32_t* counts, const int64_t* run_offset, int64_t total, int N,
                            const int64_t* byte_offset, uint8_t* out, const void* workspace, size_t workspace_bytes,
                            detops_stream_t stream);

/* ---- Reading compressed RLE strings (csrc/rle_decode.hip) -----------------------------------------------------------------
 * The inverse of the coding above: a restatement of pycocotools' rleFrString, written from knowledge of that code and,
 * like the coder, never run against it.  For the bytes of one mask's string:
 *   - a value is a maximal group of bytes that ends at the first byte b with ((b - 48) & 0x20) == 0;
 *   - its 5-bit groups are assembled from the low end: x |= ((b - 48) & 0x1f) << 5k for the group's k-th byte;
 *   - if the last group has bit 0x10 set, the value is sign-extended: x |= -1 << 5k (k = the number of bytes); x is a
 *     signed 64-bit value;
 *   - c[i] = x[i] for i <= 2, c[i] = x[i] + c[i - 2] for i > 2: two interleaved running sums that start at runs 1 and 2;
 *     c[0] stands alone.  The runs are stored as int32.
 * Malformed input is data.  A string's last byte ends a value whatever its continuation bit says; a value of more than
 * 7 bytes is read from its last 7; (b - 48) is taken modulo 256; sums wrap in 64 bits.  status [N] int32 reports per mask:
 *   DETOPS_RLE_BAD_BYTE    a byte outside 48..111
 *   DETOPS_RLE_TRUNCATED   the last byte has the continuation bit set
 *   DETOPS_RLE_LONG_VALUE  a value of more than 7 bytes
 *   DETOPS_RLE_BAD_RUN     a run below 0 or at or above 2^31 after the sums
 *   DETOPS_RLE_BAD_SUM     the runs do not sum to h * w (only when hw [N, 2] int32 is passed)
 * The runs of a flagged mask are unspecified (here: what the rules above give, truncated to int32) but in bounds.
 *
 * detops_rle_decode_count / _write — bytes [B] uint8 and byte_offset [N + 1] int64 (byte_offset[0] = 0, non-decreasing,
 *   byte_offset[N] = B) as detops_rle_string_write leaves them, or as the strings of a result file concatenated.
 *     _count: run_offset [N + 1] int64 (device) = exclusive sum of the masks' numbers of values;
 *     the caller reads run_offset[N] = total (the one host read of the path) and allocates counts [total] int32;
 *     _write: fills counts and status (hw may be null).
 *   Both calls take the same workspace of detops_rle_decode_workspace_bytes(B, N) bytes, untouched in between.  The work
 *   is cut by chunks of the flat byte array, not by mask; a value is decoded by the thread that holds its last byte,
 *   which walks back over at most 6 bytes; the running sums and the status bits are differences of plain prefix sums
 *   taken in a fixed order (no atomics): every element of counts, run_offset and status is written exactly once, nothing
 *   outside them, nothing is read outside bytes [0, B) whatever the bytes hold, and two runs give identical output.
 *   Returns: DETOPS_EINVAL for N < 0, B < 0, total < 0 or a null pointer; DETOPS_EWORKSPACE for a workspace smaller than
 *   the query's answer.  N == 0 or B == 0 (only empty strings) returns 0 with nothing launched and nothing written. */
#define DETOPS_RLE_BAD_BYTE 1
#define DETOPS_RLE_TRUNCATED 2
#define DETOPS_RLE_LONG_VALUE 4
#define DETOPS_RLE_BAD_RUN 8
#define DETOPS_RLE_BAD_SUM 16
size_t detops_rle_decode_workspace_bytes(int64_t B, int N);
int detops_rle_decode_count(const uint8_t* bytes, const int64_t* byte_offset, int64_t B, int N, int64_t* run_offset,
                            void* workspace, size_t workspace_bytes, detops_stream_t stream);
int detops_rle_decode_write(const uint8_t* bytes, const int64_t* byte_offset, int64_t B, int N, const int64_t* run_offset,
                            int64_t total, const int32_t* hw, int32_t* counts, int32_t* status, void* workspace,
                            size_t workspace_bytes, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Polygon instance masks (extensions; the reference rasterises polygons one ROI at a time on the CPU through pycocotools:
 * structures/segmentation_mask.py:273-335, roi_heads/mask_head/loss.py:11-42, "FIXME: CPU computation bottleneck").
 *
 * Packed polygons: verts [V, 2] fp32 (x, y); poly_offset [P + 1] int32: polygon p owns vertices
 * [poly_offset[p], poly_offset[p + 1]); inst_offset [G + 1] int32: instance g owns polygons [inst_offset[g], inst_offset[g + 1]).
 * Offsets are clamped to [0, V] and [0, P]: wrong ones give wrong pixels, never an access outside the arrays.
 *
 * THE DEFINITION of the fill of one polygon xy = [x0, y0, x1, y1, ...] (k >= 3 vertices) on an h x w grid is this
 * restatement of pycocotools' polygon-to-RLE routine (rleFrPoly).  It has NOT been checked against pycocotools, which
 * is not available where this library is built and tested.  All arithmetic fp64, every operation one rounding (no
 * contraction), int() truncates toward zero:
 *     x[j] = int(5 * xy[2j] + .5), y[j] = int(5 * xy[2j + 1] + .5), closed by x[k] = x[0], y[k] = y[0];
 *     every edge (xs, ys) -> (xe, ye) is walked in unit steps of its major axis (x when |dx| >= |dy|), from the end with
 *     the smaller major coordinate (a, b) towards the other, d = 0 .. |major difference|: the major coordinate is a + d
 *     and the minor one int(b + ((b' - b) / |major difference|) * d + .5); an edge of zero length is its single point;
 *     the points are emitted in the polygon's direction, (u, v) = (x, y) of the walk;
 *     two consecutive points with different u give a crossing: xd = (min(u, u') + .5) / 5 - .5; it counts if xd is an
 *     integer in [0, w - 1]; yd = (min(v, v') + .5) / 5 - .5 clamped to [0, h]; position = xd * h + ceil(yd);
 *     pixel (row, col) is set iff the number of crossings at column-major positions <= col * h + row is odd.
 * A position at row h is row 0 of the next column (for the last column it fills nothing).  An instance is the union
 * (OR) of its polygons' fills; polygons of fewer than 3 vertices fill nothing.  Coordinates with |5 * v| > 5e8 and NaN
 * saturate to +-5e8 (the literal routine has no defined answer there).
 *
 * detops_polygon_mask_targets — the mask head's targets for S slots of a batch in one launch.  Slot s: instance
 *   slot_inst[s] (int64, global index into the packed batch; outside [0, G): an all-zero target), box boxes[s] fp32
 *   xyxy, slot_wh[s] = (W, H) int32 of the slot's image.  PolygonInstance.crop + resize((M, M)), without rounding:
 *     xmin = min(max(b0, 0), W - 1), xmax = max(min(max(b2, 0), W), xmin + 1) (fp64), likewise y;
 *     every vertex becomes fp32(fp32(x - fp32(xmin)) * fp32(M / (xmax - xmin))), quotient in fp64; vertices are not clamped;
 *   then the fill on the M x M grid.  out [S, M, M] fp32 of 0 / 1, row-major, every element written once.
 *   DETOPS_EINVAL: M < 1, M > 256, a negative count, a null pointer with S > 0 (verts may be null when V == 0).
 *   S == 0 is a no-op.  The work of a slot is (edges of its instance) x M, whatever the ratio of instance to box size.
 * detops_polygons_to_masks — the dense planes of the G instances of one H x W image: out [G, H, W] uint8 of 0 / 1,
 *   every byte written once, zeros included.  DETOPS_EINVAL: a negative count, H > 3584 (a strip of columns of the
 *   plane lives in LDS as bits), G > 65535, a null pointer; G, H or W == 0 is a no-op.  G * H * W may exceed 2^31.
 * ---------------------------------------------------------------------------------------- */
int detops_polygon_mask_targets(const float* verts, const int32_t* poly_offset, const int32_t* inst_offset, int V, int P,
                                int G, const int64_t* slot_inst, const float* boxes, const int32_t* slot_wh, int S, int M,
                                float* out, detops_stream_t stream);
int detops_polygons_to_masks(const float* verts, const int32_t* poly_offset, const int32_t* inst_offset, int V, int P, int G,
                             int H, int W, unsigned char* out, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Detection evaluation (csrc/evaluate.hip; extensions: the reference stores every prediction, pastes and RLE-encodes the
 * masks on the CPU and hands them to pycocotools' COCOeval, data/datasets/evaluation/coco/coco_eval.py; its VOC
 * evaluation is data/datasets/evaluation/voc/voc_eval.py).  Here the detections and the ground truth of a batch are
 * matched on the device and only the match records are kept.
 *
 * The unit of work is a PROBLEM: the detections and the ground-truth instances of one (image, category) pair.  The
 * caller sorts the detections by problem and, inside a problem, by score descending (a stable sort: ties keep their
 * input order), and the ground truths by problem (input order inside).  dt_offset / gt_offset [P + 1] int32 delimit a
 * problem's detections and ground truths in those sorted arrays; iou_offset [P + 1] int64 is the exclusive sum of
 * D_p * G_p: the IoU matrix of problem p is D_p x G_p, row-major, at iou_offset[p]; total_pairs = iou_offset[P].  Every
 * per-detection / per-ground-truth argument below is in sorted order.
 *
 * detops_mask_pack — uint8 / bool planes to row-major bit rows.  Plane n is H x W = plane_hw[n] (int32 pairs) and
 *   starts plane_offset[n] bytes into `planes` (the planes of a batch differ in size); its rows of ceil(W / 64) 64-bit
 *   words start at words[word_offset[n]] (bit b of word c of a row is pixel 64 c + b; non-zero bytes are set pixels; bits
 *   at or beyond W are zero).  area [N] int32 receives the set-pixel count (H * W < 2^31), extent [N, 4] int32 the tight
 *   extents (first row, last row, first word column, last word column), (H, -1, ceil(W / 64), -1) for an empty plane.
 *   Counts and extents are combined with integer atomics: deterministic.  max_words: the largest H * ceil(W / 64) of
 *   the call (sizes the grid; speed only).  Every word is written exactly once.
 * detops_mask_pack_rle — the same five results from uncompressed RLE, no plane stored: counts
 *   [total] int32 and run_offset [N + 1] int64 as detops_paste_masks_rle_write or detops_rle_decode_write make them,
 *   plane_hw [N, 2].  Runs are column-major and start with a 0-run: pixel (y, x) is set iff position x * H + y lies in an
 *   odd-indexed run; zero-length runs are legal and only toggle; area is the sum of the odd runs.  Runs that do not sum to
 *   H * W are malformed: positions beyond the runs are 0, runs beyond H * W and negative runs are ignored.  words,
 *   word_offset, area and extent as detops_mask_pack (layout, zero bits at and beyond W, empty-plane extents), every word
 *   written exactly once, atomics for areas and extents only.  max_h / max_w: the largest H and W of the call.  THE
 *   LARGEST H SERVED IS DETOPS_MASK_PACK_RLE_MAX_H (a strip of 64 columns lives in LDS as bits): with max_h above it the
 *   entry point returns DETOPS_EUNSUPPORTED with nothing launched, and the caller packs that call on the host.
 *   workspace: >= detops_mask_pack_rle_workspace_bytes(total) bytes, else DETOPS_EWORKSPACE.
 * detops_mask_pair_counts — counts [total_pairs] int32: for every (detection, ground truth) pair of every problem, the
 *   pixels set in both planes: popcount of the AND over the words inside the intersection of the two extents.  Pairs
 *   with disjoint extents read no plane; a pair whose planes differ in (H, W) gets -1 and reads none.  Every element
 *   is written exactly once; no floating point.
 * detops_eval_iou — iou [total_pairs] fp64, every element written once.  Boxes are fp32 xyxy [*, 4].  mode:
 *   DETOPS_EVAL_COCO_SEGM  i / (area_d + area_g - i) from counts and the int32 areas, fp64; i / area_d for a crowd; a count
 *                          that is not positive gives 0, the -1 of a pair of planes of different sizes included;
 *   DETOPS_EVAL_COCO_BBOX  both boxes as BoxList.convert("xywh") makes them, fp32: w = (x2 - x1) + 1, h likewise; then fp64
 *                          with no further + 1: iw = min(x_d + w_d, x_g + w_g) - max(x_d, x_g), ih likewise, 0 unless both
 *                          are > 0; i = iw * ih; u = w_d h_d + w_g h_g - i, or w_d h_d for a crowd;
 *   DETOPS_EVAL_VOC        the reference's formula: + 1 on x2 and y2 of both boxes (fp32), then boxlist_iou's fp32
 *                          expression with TO_REMOVE = 1 (areas (x2 - x1 + 1)(y2 - y1 + 1), wh = max(rb - lt + 1, 0),
 *                          inter / ((area_d + area_g) - inter)), widened to fp64; gt_crowd is not read.
 *   A union of 0 gives IoU 0 in every mode.  pycocotools divides 0 by 0 there: the original has no defined answer for
 *   that case, and 0 is THIS LIBRARY'S CHOICE.  No operation is contracted.
 * detops_eval_match — greedy matching, one wave per problem.
 *   COCO modes (SEGM and BBOX match alike): a lane is an (area range a, threshold t) pair, iou_thrs [T] and
 *   area_rngs [A, 2] are fp64 INPUTS, A * T <= 4096.  Ground truth g is ignored in range a when gt_flag[g] (iscrowd), or
 *   gt_area[g] < lo_a, or gt_area[g] > hi_a.  The lane visits the non-ignored ground truths first and the ignored ones
 *   after, each group in input order, and for every detection d in score order runs
 *       iou = min(t, 1 - 1e-10); m = -1
 *       for g in visiting order:
 *           if matched[g] and not iscrowd[g]: continue
 *           if m > -1 and not ignored[m] and ignored[g]: break
 *           if IoU[d, g] < iou: continue
 *           iou = IoU[d, g]; m = g
 *       if m > -1: dt_match[a, t, d] = m; dt_ignore[a, t, d] = ignored[m]; matched[m] = 1
 *   a detection left unmatched is ignored when dt_area[d] lies outside [lo_a, hi_a].  Outputs: dt_match int32
 *   [A, T, D_total] (ground-truth index inside the problem, or -1), dt_ignore uint8 [A, T, D_total], gt_ignore uint8
 *   [A, G_total]; D_total = dt_offset[P] and G_total = gt_offset[P] are passed as host values (they size the outputs: a
 *   problem whose offsets reach beyond them is skipped).
 *   DETOPS_EVAL_VOC (calc_detection_voc_prec_rec): per detection g* = the first argmax of its IoU row; match 0 if that
 *   IoU < iou_thrs[0] (or G_p == 0); else -1 if gt_flag[g*] (difficult); else 1 if g* was not selected before and 0 if it
 *   was; g* is marked selected in the last two cases.  Output voc_match int8 [D_total]; areas and area_rngs are unused.
 *   THE LARGEST G_p SERVED IS DETOPS_EVAL_MAX_GT (the lanes' matched sets are 64-bit registers up to 64 ground truths and
 *   live in LDS above).  max_gt: the largest G_p of the call (host value; sizes LDS).  With max_gt above the cap the
 *   launch still serves every problem within it, leaves the outputs of the others untouched and returns DETOPS_EGTCAP,
 *   a code no other condition produces: the caller computes those problems on the host.
 * DETOPS_EINVAL: negative sizes, an unknown mode, a null pointer the mode needs (detops_eval_match: per-detection arrays
 * may be null only when D_total == 0, per-ground-truth arrays only when G_total == 0; iou is null when no problem has
 * a pair, which the entry point cannot tell, so it is not checked).
 * N, P or total_pairs == 0 is a no-op.
 * ---------------------------------------------------------------------------------------- */
#define DETOPS_EVAL_COCO_SEGM 0
#define DETOPS_EVAL_COCO_BBOX 1
#define DETOPS_EVAL_VOC 2
#define DETOPS_EVAL_MAX_GT 4096
int detops_mask_pack(const unsigned char* planes, const int64_t* plane_offset, const int32_t* plane_hw, int N,
                     int64_t max_words, const int64_t* word_offset, uint64_t* words, int32_t* area, int32_t* extent,
                     detops_stream_t stream);
#define DETOPS_MASK_PACK_RLE_MAX_H 4096
size_t detops_mask_pack_rle_workspace_bytes(int64_t total);
int detops_mask_pack_rle(const int32_t* counts, const int64_t* run_offset, int64_t total, const int32_t* plane_hw, int N,
                         int max_h, int max_w, const int64_t* word_offset, uint64_t* words, int32_t* area, int32_t* extent,
                         void* workspace, size_t workspace_bytes, detops_stream_t stream);
int detops_mask_pair_counts(const uint64_t* dt_words, const int64_t* dt_word_offset, const int32_t* dt_hw,
                            const int32_t* dt_extent, const uint64_t* gt_words, const int64_t* gt_word_offset,
                            const int32_t* gt_hw, const int32_t* gt_extent, const int32_t* dt_offset, const int32_t* gt_offset,
                            const int64_t* iou_offset, int P, int64_t total_pairs, int32_t* counts, detops_stream_t stream);
int detops_eval_iou(int mode, const int32_t* counts, const int32_t* dt_area, const int32_t* gt_area, const float* dt_boxes,
                    const float* gt_boxes, const unsigned char* gt_crowd, const int32_t* dt_offset, const int32_t* gt_offset,
                    const int64_t* iou_offset, int P, int64_t total_pairs, double* iou, detops_stream_t stream);
int detops_eval_match(int mode, const double* iou, const int32_t* dt_offset, const int32_t* gt_offset,
                      const int64_t* iou_offset, int P, int64_t D_total, int64_t G_total, int max_gt, const double* dt_area,
                      const double* gt_area,
                      const unsigned char* gt_flag, const double* iou_thrs, int T, const double* area_rngs, int A,
                      int32_t* dt_match, unsigned char* dt_ignore, unsigned char* gt_ignore, signed char* voc_match,
                      detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Keypoint evaluation (OKS) (csrc/eval_oks.hip; extension: the reference hands keypoints.json to pycocotools' COCOeval with
 * iouType "keypoints").  The similarity of a detection and a ground truth is the object keypoint similarity; the matching
 * around it is detops_eval_match, unchanged.
 *
 * The rules are a restatement of pycocotools.cocoeval (computeOks, the keypoint branches of _prepare, evaluateImg and
 * setKpParams, and loadRes for keypoint results), written from knowledge of that code.  **NOBODY HAS CHECKED THIS
 * RESTATEMENT AGAINST pycocotools**, which is not available where this project is built and tested; tests/oks_refs.py is
 * the literal, loop-by-loop form everything here is pinned to.
 *
 * A problem is as above (the detections and ground truths of one (image, category) pair, sorted arrays, dt_offset /
 * gt_offset / iou_offset), with the detections of a problem cut to 20.  Keypoints are fp32 [*, K, 3] rows of (x, y, v) as
 * Keypoints.keypoints stores them.  For detection d and ground truth g, in fp64 with no operation contracted:
 *     var[k] = (2 * sigma[k])^2                       sigma: fp64 [K], an INPUT
 *     k1     = the number of k with vg[k] > 0         (the ground truth's visibility flags)
 *     if k1 > 0:  dx[k] = xd[k] - xg[k];  dy[k] = yd[k] - yg[k]
 *     else:       x0 = bx - bw; x1 = bx + 2*bw; y0 = by - bh; y1 = by + 2*bh
 *                 dx[k] = max(0, x0 - xd[k]) + max(0, xd[k] - x1);  dy[k] likewise
 *     e[k]   = (dx[k]*dx[k] + dy[k]*dy[k]) / var[k] / (area_g + 2^-52) / 2        in this order
 *     oks    = (the sum over the k that count of exp(-e[k])) / (the number of k that count)
 *              the k that count: those with vg[k] > 0 when k1 > 0, all K otherwise
 *   - coordinates are widened from fp32 to fp64 before the subtraction; the detection's third column is never read;
 *   - (bx, by, bw, bh) is BoxList.convert("xywh") of the ground truth's fp32 xyxy box, w = (x2 - x1) + 1 in fp32 (the
 *     convention of DETOPS_EVAL_COCO_BBOX), then widened;
 *   - area_g is the ground truth's area as the evaluator has it: the `area` field, else the mask's pixel count, else the
 *     area of the xywh box;
 *   - THE SUM RUNS IN KEYPOINT ORDER, ONE TERM AFTER THE OTHER, starting from 0.  pycocotools calls np.sum, which adds in
 *     a blocked order of its own and differs from the sequential sum in the last bit for about half of random 17-term
 *     inputs: the last bits of an OKS are THIS LIBRARY'S CHOICE and can differ from pycocotools';
 *   - exp is the device library's fp64 exp (host path: the C library's).  Where every e[k] is 0 the result is exactly 1.
 *   The default sigma is the COCO person table, recalled and NOT CHECKED against pycocotools:
 *     [.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89] / 10.
 * dt_area [D_total] fp64, the detection's area for the "unmatched detection outside the area range" rule, is
 *   (max x - min x) * (max y - min y) over all K keypoints, the extents taken in fp32 and the two differences and the
 *   product in fp64 (loadRes makes the result's box and area from the keypoint extents).  A NaN coordinate makes it NaN.
 * Around it (the caller's part, data/datasets/evaluation/keypoint_oks.py):
 *   - a ground truth is ignored in an area range when it is a crowd, when it has no visible keypoint (k1 == 0; pycocotools
 *     reads the annotation's num_keypoints, here it is counted), or when its area lies outside the range;
 *   - a crowd may be matched again, a ground truth with k1 == 0 may not: detops_eval_match gets gt_flag = iscrowd and, for
 *     a ground truth with k1 == 0 that is no crowd, the area -1, which lies outside every range (the OKS above still
 *     divides by the real area);
 *   - area ranges all / medium / large = [[0, 1e10], [32^2, 96^2], [96^2, 1e10]], max detections (20,), the thresholds and
 *     recall levels of the other types; the ten statistics in order: AP, AP50, AP75, APm, APl, AR, AR50, AR75, ARm, ARl.
 *
 * detops_eval_oks — oks [total_pairs] fp64 in the layout of detops_eval_iou and dt_area [D_total] fp64, one launch.  Every
 *   output element is written exactly once, there are no atomics and no reduction tree: two runs give identical bits.  A
 *   pair index outside its problem's matrix (inconsistent offsets) writes 0 and reads nothing.  THE LARGEST K SERVED IS
 *   DETOPS_EVAL_OKS_MAX_K (a pair is half a wave, a lane per keypoint): above it the entry point returns
 *   DETOPS_EUNSUPPORTED with nothing launched, and the caller computes the call on the host.
 * DETOPS_EINVAL: K < 1, negative sizes, P > 0 with a null offsets array, total_pairs > 0 with P == 0 or a null dt_kpts,
 * gt_kpts, gt_boxes, gt_area, sigmas or oks, D_total > 0 with a null dt_kpts or dt_area.
 * total_pairs == 0 (P == 0 included) writes no oks, D_total == 0 no dt_area; both 0 is a no-op.
 * ---------------------------------------------------------------------------------------- */
#define DETOPS_EVAL_OKS_MAX_K 32
int detops_eval_oks(const float* dt_kpts, const float* gt_kpts, const float* gt_boxes, const double* gt_area,
                    const double* sigmas, int K, const int32_t* dt_offset, const int32_t* gt_offset,
                    const int64_t* iou_offset, int P, int64_t D_total, int64_t total_pairs, double* oks, double* dt_area,
                    detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Proposal recall (csrc/eval_proposals.hip; reference data/datasets/evaluation/coco/coco_eval.py, evaluate_box_proposals:
 * the average recall of RPN proposals, `box_only`).  For every image, every proposal limit and every area range the
 * reference runs a Python loop of min(P, G) rounds over the [P, G] IoU matrix; here all of them are one launch, and the
 * matrix never exists in memory.  Unlike the COCO-style rules above this is no restatement from memory: the reference's
 * function is plain torch, and tests/golden/box_proposals_reference.npz holds what it returned.
 *
 *   dt_boxes [D_total, 4] fp32 xyxy: the proposals of a batch, image after image; inside an image IN OBJECTNESS ORDER,
 *     descending (the caller sorts).  gt_boxes [G_total, 4] fp32 xyxy.  dt_offset / gt_offset [N + 1] int32.
 *   gt_valid [A, G_total] uint8: ground truth g counts in area range a (the caller compares the areas: fp32,
 *     (area >= lo) & (area <= hi), both ends inclusive.  The reference compares an fp32 tensor when the json areas are
 *     floats and an int64 tensor when they are all integers; the two differ only for areas above 2^24).
 *   limits [L] int32: <= 0 for no limit, else the number of leading proposals of an image that take part.
 *   overlaps [L, A, G_total] fp32, every element written exactly once.
 *
 * Per (image, limit l, range a):  P' = min(P, limits[l]) when limits[l] > 0, else P;  G' = the number of valid ground truths.
 *   IoU[p, g] is boxlist_iou's fp32 expression, no operation contracted:
 *     area = ((x2 - x1) + 1) * ((y2 - y1) + 1);   w, h = max((min(x2, X2) - max(x1, X1)) + 1, 0), likewise in y;
 *     inter = w * h;   iou = inter / ((area_p + area_g) - inter), the correctly rounded fp32 quotient.
 *   Then min(P', G') rounds: among the unused valid ground truths take the one whose largest IoU over the unused proposals
 *   is largest (ties: the lowest ground-truth index); for it the proposal that attains that IoU (ties: the lowest proposal
 *   index); write the IoU to the ground truth's slot and retire both.  This is the reference's overlaps.max(dim=0) /
 *   max_overlaps.max(dim=0) with the first maximum taken, which is what the fixture's built ties show torch to do.
 *   A valid ground truth no round reaches gets 0, a ground truth with gt_valid == 0 gets -1.
 *   Outside the contract: boxes with x2 < x1 - 1 or y2 < y1 - 1, NaN coordinates, and two boxes of area 0 (their IoU is 0 / 0,
 *   on which the reference's own assertion fails).  They may give any value; they never cause an access outside the arrays
 *   (a NaN IoU is never selected).
 *
 * One workgroup per (image, limit, range) holds the image's boxes in LDS and, per ground truth, the best (IoU, proposal)
 * among the unused proposals; a round is an argmax over those, and only the ground truths whose best was the retired
 * proposal are scanned again.  No atomics: two runs give identical bits.
 * max_dt / max_gt: the largest P' and the largest G of any image of the call, as the CALLER knows them on the host (they
 *   size the LDS; nothing is read back from the device).  THE LARGEST SERVED ARE DETOPS_EVAL_PROPOSALS_MAX_DT AND
 *   DETOPS_EVAL_PROPOSALS_MAX_GT: above either the entry point returns DETOPS_EUNSUPPORTED with nothing launched, and the
 *   caller computes the call on the host.  An image larger than stated is cut to max_dt proposals, and its ground truths
 *   from max_gt on are never matched (0 or -1); offsets that leave [0, D_total] / [0, G_total] make the image's workgroups
 *   write nothing.
 * DETOPS_EINVAL: N < 0, L < 1, A < 1, D_total < 0, G_total < 0, max_dt < 0, max_gt < 0, N * L * A >= 2^31; with N > 0 and
 * G_total > 0 a null dt_offset, gt_offset, gt_boxes, gt_valid, limits or overlaps, or a null dt_boxes with D_total > 0.
 * N == 0 or G_total == 0 is a no-op.  No workspace.
 * ---------------------------------------------------------------------------------------- */
#define DETOPS_EVAL_PROPOSALS_MAX_DT 2048
#define DETOPS_EVAL_PROPOSALS_MAX_GT 1024
int detops_eval_proposal_overlaps(const float* dt_boxes, const float* gt_boxes, const int32_t* dt_offset,
                                  const int32_t* gt_offset, const unsigned char* gt_valid, const int32_t* limits, int N, int L,
                                  int A, int64_t D_total, int64_t G_total, int max_dt, int max_gt, float* overlaps,
                                  detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Cityscapes evaluation (csrc/cityscapes_eval.hip; reference data/datasets/evaluation/cityscapes/eval_instances.py,
 * matchGtWithPred / prepareGtImage / preparePredImage).  For every instance and for every (ground truth, prediction) pair
 * whose boxes overlap the reference crops full-size planes to a window, multiplies, sums and calls .item(): one host round
 * trip each.  Here all the counts of one image are one call.  tests/golden/cityscapes_reference.npz holds what the
 * reference's functions returned.
 *
 *   dt_planes [D, H, W], gt_planes [G, H, W] bytes: a NON-ZERO byte is a set pixel (bool, 0/1 and 0/255 planes all serve).
 *   dt_box [D, 4], gt_box [G, 4] int32 (xmin, ymin, xmax, ymax): the reference's bbox.long() of the xyxy boxes.
 *   The window of a box: rows [ymin, ymax) and columns [xmin, xmax), THE MAXIMA EXCLUSIVE (the reference's slices: the last
 *     row and column of a tight box are left out, for ground truth and predictions alike), clamped to [0, H] x [0, W]
 *     (the reference lets a negative minimum wrap around as a Python index; this library's choice); empty when a maximum does
 *     not exceed its minimum.
 *   dt_count [D], gt_count [G] int32: the set pixels of the instance's plane inside the window of its own box (pixelCount).
 *   A pair (d, g) takes part iff isOverlapping: dt.xmin < gt.xmax && gt.xmin < dt.xmax && dt.ymin < gt.ymax &&
 *     gt.ymin < dt.ymax on the boxes as given (not clamped).  Then
 *       pair_box [d, g]  = (min(xmax) - max(xmin)) * (min(ymax) - max(ymin)) (boxIntersection; positive for boxes whose
 *                          minima lie below their maxima; formed in 64 bits and saturated to the int32 range),
 *       pair_mask [d, g] = the pixels set in BOTH planes inside the window of the UNION box (min of the minima, max of the
 *                          maxima), again exclusive and clamped (maskIntersection).
 *     Both are 0 for a pair that does not take part, and such a pair reads no plane.  pair_box, pair_mask [D, G] int32.
 *   Every output element is written for every input, whatever the memory held before: the entry point's first launch
 *   writes zeros and pair_box, the second adds the strips of every window with 32-bit integer atomics.  Integers only, so
 *   two runs give identical bits.  Plane offsets are 64-bit (D * H * W may pass 2^31).  No workspace.
 * DETOPS_EINVAL: D, G, H or W negative; H * W >= 2^31; D + G + D * G >= DETOPS_WINDOW_COUNTS_MAX_ITEMS (a work item is a
 *   workgroup column of the grid); a null dt_box / dt_count with D > 0, gt_box / gt_count with G > 0, pair_box / pair_mask
 *   with D * G > 0, dt_planes with D * H * W > 0 or gt_planes with G * H * W > 0.
 * D == 0 or G == 0 still fills the other side's counts; H * W == 0 gives zero counts (pair_box is still formed).
 * ---------------------------------------------------------------------------------------- */
#define DETOPS_WINDOW_COUNTS_MAX_ITEMS 16777216
int detops_window_counts(const unsigned char* dt_planes, const int32_t* dt_box, int D, const unsigned char* gt_planes,
                         const int32_t* gt_box, int G, int H, int W, int32_t* dt_count, int32_t* gt_count, int32_t* pair_box,
                         int32_t* pair_mask, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Batch image preparation (csrc/image_prep.hip; extension: the reference resizes every image on the CPU with
 * torchvision over Pillow, data/transforms/transforms.py, and copies the padded fp32 batch to the device).  One launch
 * takes the raw RGB uint8 HWC images of a batch to the zero-padded fp32 batch tensor: Resize, RandomHorizontalFlip,
 * RandomVerticalFlip, ToTensor, Normalize, to_image_list.
 *
 * The resize is Image.resize((ow, oh), Image.BILINEAR) of Pillow, which is integer arithmetic.  For one axis with input
 * size `in` and output size `out`, all in fp64, nothing contracted:
 *     scale = in / out;  fs = max(scale, 1.0);  support = 1.0 * fs;  ksize = ceil(support) * 2 + 1;  ss = 1.0 / fs
 *   and for output index xx:
 *     center = (xx + 0.5) * scale
 *     xmin = max(int(center - support + 0.5), 0)             (int: the C cast, truncation toward zero)
 *     n    = min(int(center + support + 0.5), in) - xmin
 *     w[x] = max(0, 1 - |(x + xmin - center + 0.5) * ss|)    for x < n
 *     ww   = the sum of the n weights, added in order;  w[x] = w[x] / ww when ww != 0
 *     k[x] = int(w[x] * 2^22 + 0.5)
 *     out[xx] = clip8((2^21 + sum_x in[xmin + x] * k[x]) >> 22)     in 32-bit integers, clip8 to [0, 255]
 *   The horizontal pass runs first; its uint8 result, rounded and clipped, is the input of the vertical pass.  A pass
 *   whose axis keeps its size is skipped (the bytes go through unchanged).
 * After the resize: a horizontal flip (flip bit 0) and a vertical flip (bit 1) mirror the RESIZED image; then
 *   out[i, c, y, x] = table[c][byte of channel (bgr ? 2 - c : c) at (y, x)]         for y < oh, x < ow, and +0.0 elsewhere.
 *   table [3, 256] fp32 is made by the caller with the framework's own expressions (t = float32(u8) / 255; t * 255 with
 *   TO_BGR255; (t - float32(mean[c])) / float32(std[c])), so the batch equals the host pipeline's bit for bit.
 *
 *   raw        the images back to back, image i at byte offsets[i] (int64 [N], device), raw_bytes in all
 *   geom       int32 [N, 5] per image: source h, w, destination oh, ow, flip bits; on the device, and the same records
 *              on the host as geom_host (the entry point validates them and sizes LDS without a device read)
 *   out        fp32 [N, 3, Hp, Wp] contiguous, or with channels_last the same tensor in torch.channels_last memory
 *              ([N, Hp, Wp, 3]).  Every element is written exactly once, the padding zeros included.  16-byte stores where
 *              a thread's four elements are 16-byte aligned (every row when Wp % 4 == 0), 4-byte stores elsewhere.
 * THE LARGEST ksize SERVED IS DETOPS_IMAGE_PREP_MAX_KSIZE: a downscale by up to 8 per axis.  A batch with an axis beyond it
 * returns DETOPS_EINVAL with nothing launched; the caller prepares that batch on the host.
 * DETOPS_EINVAL also: N < 0 or > 65535, negative sizes, Hp > 65535 * 16, a record with a size < 1 or oh > Hp or ow > Wp,
 * a null pointer.  N, Hp or Wp == 0 is a no-op.  A record on the device that differs from its host copy cannot make the
 * kernel leave its buffers: an image it cannot serve is written as zeros.
 * ---------------------------------------------------------------------------------------- */
#define DETOPS_IMAGE_PREP_MAX_KSIZE 17
int detops_image_batch_u8(const uint8_t* raw, int64_t raw_bytes, const int64_t* offsets, const int32_t* geom,
                          const int32_t* geom_host, int N, const float* table, int bgr, int Hp, int Wp, int channels_last,
                          float* out, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Colour jitter of the raw images of a batch (csrc/color_jitter.hip; the reference's data/transforms/transforms.py
 * ColorJitter hands the PIL image to torchvision's, which is a thin layer over Pillow: ImageEnhance.Brightness / Contrast /
 * Color, i.e. Image.blend against a degenerate image, and an add on the H plane of convert("HSV")).  IN PLACE on the
 * device copy of the raw bytes detops_image_batch_u8 reads afterwards.
 *
 * An image is h x w RGB bytes.  It has up to four steps, each operation at most once, in a per-image order.  Everything
 * is evaluated exactly as written, nothing contracted into an FMA.
 *   blend(d, x, a), per byte; a = the factor rounded to fp32, d the "degenerate" byte, x the image byte:
 *     t = float(d) + a * float(x - d)          (the INTEGER difference is converted; one fp32 multiply, one fp32 add)
 *     0 <= a <= 1:  uint8(trunc(t));   otherwise 0 for t <= 0, 255 for t >= 255, else uint8(trunc(t))
 *   L(r, g, b) = (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16                                       (convert("L"))
 *   brightness(f):  blend(0, x, f)
 *   saturation(f):  blend(L(pixel), x, f) on each channel
 *   contrast(f):    blend(m, x, f);  m = int(S / (h * w) + 0.5) in fp64, S the integer sum of L over the whole image AS IT
 *                   IS WHEN THE STEP IS REACHED, i.e. after the steps in front of it
 *   hue(k), k in 0 .. 255:  RGB -> HSV,  H = (H + k) & 255,  HSV -> RGB
 *   RGB -> HSV:  maxc, minc = the largest and smallest byte;  V = maxc;  minc == maxc: H = S = 0.  Otherwise in fp32
 *     cr = float(maxc - minc);  s = cr / float(maxc);  rc = float(maxc - r) / cr, gc and bc likewise;
 *     r == maxc: h = bc - gc (fp32);  else g == maxc: h = float(2.0 + rc - bc);  else h = float(4.0 + gc - rc)   (the last
 *     two in fp64, left to right, rounded to fp32 once);  h = float(fmod(double(h) / 6.0 + 1.0, 1.0));
 *     H = clip8(int(double(h) * 255.0));  S = clip8(int(double(s) * 255.0))                          (int: the C cast)
 *   HSV -> RGB:  S == 0: (V, V, V).  Otherwise h6 = double(H) * 6.0 / 255.0;  i = floor(h6);  f = float(h6 - float(i));
 *     fs = float(double(S) / 255.0);  in fp64, round = half away from zero, then clip8:
 *     p = round(V * (1.0 - fs));  q = round(V * (1.0 - fs * f));  t = round(V * (1.0 - fs * (1.0 - f)))
 *     (R, G, B) by i % 6:  0 (V,t,p)  1 (q,V,p)  2 (p,V,t)  3 (p,q,V)  4 (t,p,V)  5 (V,p,q)       (H = 255: i = 6, case 0)
 * WHAT WAS CHECKED: this arithmetic equals Pillow 12.2.0 (x86-64) on all 2^24 RGB colours for convert("L"), the three
 * enhancers at seven factors and RGB -> HSV, and on all 2^24 HSV triples for HSV -> RGB, with no differing byte
 * (tests/golden/make_golden_color_jitter.py, profiles/color_jitter_exhaustive.txt).  Pillow's C code is compiled without
 * FMA contraction on x86-64; a Pillow build for another host may contract the blend and differ in the last bit.
 * WHAT WAS NOT: the parameters (data/transforms/transforms.py RawColorJitter).  A number v >= 0 for brightness, contrast
 * or saturation means a factor uniform in [max(0, 1 - v), 1 + v], hue 0 <= v <= 0.5 uniform in [-v, v], a (lo, hi) pair is
 * taken as given; a range that is the identity disables the operation, which then makes no draw; k = int(f * 255) mod 256
 * (fp64 product, truncated toward zero).  Draws from Python's `random`: one uniform per enabled operation in the order
 * brightness, contrast, saturation, hue, then one shuffle of the enabled operations.  This draw order is THIS LIBRARY'S
 * DEFINITION, written as torchvision's ColorJitter.get_params is recalled; it was not checked against torchvision.
 *
 *   raw, offsets, geom, geom_host   as detops_image_batch_u8 (h and w are read from the records; raw is WRITTEN)
 *   jitter     int32 [N, DETOPS_COLOR_JITTER_FIELDS] per image: four step codes in the order they run (0 none,
 *              1 brightness, 2 contrast, 3 saturation, 4 hue; the list ends at the first 0 and only 0 may follow it), then
 *              the four parameters at the same positions: the fp32 bits of the factor, or k.  On the device, and the same
 *              records on the host as jitter_host (validated before anything is launched).
 *   workspace  N * 8 bytes on the device (the images' sums of L, 64-bit: 255 h w passes 2^32 from 16.8 M pixels); only
 *              used, and only required, when some image has a contrast step.
 * At most two kernel launches (and one 8 N byte memset in front of the first): a sum pass when some image has a contrast
 * step (the steps in front of contrast are applied on the fly, nothing is written to the images), then the apply pass.
 * Every byte of every image with at least one step is written exactly once; no other byte of `raw` is written.
 * DETOPS_EINVAL with nothing launched: N < 0, raw_bytes < 0, a null pointer (workspace: only with a contrast step), a
 * record with h or w < 1, an unknown step code, a code after the end of the list, an operation given twice, k outside
 * 0 .. 255, a non-finite factor.  DETOPS_EWORKSPACE: a workspace under N * 8 bytes with a contrast step.  N == 0 or no
 * image with a step is a no-op with no launch.  The kernel bounds every access by the image's own byte range and by
 * raw_bytes: a record on the device that differs from its host copy cannot make it leave the buffer (an image it cannot
 * serve is skipped).
 * ---------------------------------------------------------------------------------------- */
#define DETOPS_COLOR_JITTER_FIELDS 8
#define DETOPS_COLOR_JITTER_MAX_STEPS 4
int detops_color_jitter_u8(uint8_t* raw, int64_t raw_bytes, const int64_t* offsets, const int32_t* geom,
                           const int32_t* geom_host, const int32_t* jitter, const int32_t* jitter_host, int N,
                           void* workspace, size_t workspace_bytes, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Merge of test-time box augmentation (csrc/bbox_aug.hip; the reference's engine/bbox_aug.py maps every pass's BoxList
 * back with BoxList.transpose / resize, concatenates them per image and runs filter_results' per-class loop).  The passes
 * of a batch hand in their unfiltered per-class boxes; the merge maps them to the frame of the image's first pass and
 * compacts the pairs above the score threshold into one NMS segment per (image, class).
 *
 *   boxes [R, 4C] fp32, scores [R, C] fp32: the rows of every (image, pass) group, image-major, the T passes of an image in
 *   order; group g = image * T + pass holds rows row_offset[g] .. row_offset[g + 1] (int32 [N*T + 1] on the device, and the
 *   same values on the host as row_offset_host: the entry points validate them and size the grid without a device read).
 *   group_geom int32 [N*T, 3]: the group's frame (w, h) and its flip bit;  group_ratio fp32 [N*T, 2]: float(w0) / float(w),
 *   float(h0) / float(h) rounded to fp32, (w0, h0) the frame of the image's first pass.
 * Per box, in fp32, nothing contracted:
 *     x1, x2 clamped to [0, w - 1], y1, y2 to [0, h - 1]                      (clip_to_image; a NaN stays a NaN)
 *     flip bit:  x1' = (w - x2) - 1,  x2' = (w - x1) - 1                      (BoxList.transpose(FLIP_LEFT_RIGHT))
 *     pass > 0:  x * ratio_w, y * ratio_h, one multiply per coordinate        (BoxList.resize; the first pass is not scaled)
 * (row, class j >= 1) is a candidate when scores[row, j] > score_thresh.  Segment s = image * (C - 1) + (j - 1) holds the
 * candidates of class j of the image in row order, which is pass order, then row order.
 *
 * detops_bbox_aug_merge_count writes seg_offsets int32 [N*(C-1) + 1] (exclusive prefix of the segment lengths) and
 * totals int32 [2] = {M, the longest segment}; the caller reads totals once, allocates cand_boxes [M, 4] and cand_scores [M]
 * and calls detops_bbox_aug_merge_write with the SAME inputs, seg_offsets and workspace (capacity = the rows allocated: a
 * position beyond it is not written).  The order comes from prefix sums (wave ballots, a fixed scan), never from atomics:
 * two runs write identical bytes.  Every output element is written exactly once; the workspace needs no initialisation.
 * R == 0, M == 0, N == 0, C == 1 and empty groups are served (seg_offsets all zero where nothing passes).
 * boxes and cand_boxes are read and written one box per 16-byte access: BOTH MUST BE 16-BYTE ALIGNED (DETOPS_EINVAL if not).
 * DETOPS_EINVAL: negative sizes, T < 1, N > 65535, R * C >= 2^31, a null pointer that is needed, a row_offset_host that does
 * not start at 0, end at R or decreases.  A device row_offset that differs from its host copy cannot make the kernels leave
 * their buffers.
 * ---------------------------------------------------------------------------------------- */
size_t detops_bbox_aug_merge_workspace_bytes(int N, int C, int max_image_rows);
int detops_bbox_aug_merge_count(const float* scores, const int32_t* row_offset, const int32_t* row_offset_host, int R, int C,
                                int N, int T, float score_thresh, int32_t* seg_offsets, int32_t* totals, void* workspace,
                                size_t workspace_bytes, detops_stream_t stream);
int detops_bbox_aug_merge_write(const float* boxes, const float* scores, const int32_t* row_offset,
                                const int32_t* row_offset_host, const int32_t* group_geom, const float* group_ratio, int R,
                                int C, int N, int T, float score_thresh, const int32_t* seg_offsets, int64_t capacity,
                                float* cand_boxes, float* cand_scores, const void* workspace, size_t workspace_bytes,
                                detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused FrozenBatchNorm2d affine (+ residual) (+ ReLU) — the elementwise tail of every backbone
 * convolution: layers/batch_norm.py:19-31 (`x * scale + bias`), then `F.relu_`, and in the
 * bottleneck tail `out += identity; relu` (modeling/backbone/resnet.py:343-366).
 *   x, residual (nullable), y: [N, C, HW] contiguous (NCHW), dtype code as above (fp32 arithmetic)
 *   scale, bias: fp32 [C]   (scale = weight * rsqrt(running_var), bias = bias - running_mean * scale)
 *   forward : y = [relu]( x * scale[c] + bias[c] [+ residual] )
 *   backward: g = relu ? (y > 0 ? grad_y : 0) : grad_y;  grad_x = g * scale[c];
 *             grad_residual (nullable) = g
 * ---------------------------------------------------------------------------------------- */
int detops_frozen_bn_act_forward(const void* x, const float* scale, const float* bias,
                                 const void* residual, void* y, int dtype, int N, int C, int HW,
                                 int relu, detops_stream_t stream);

int detops_frozen_bn_act_backward(const void* grad_y, const void* y, const float* scale,
                                  void* grad_x, void* grad_residual, int dtype, int N, int C,
                                  int HW, int relu, detops_stream_t stream);

/* The same pair for channels-last activations ([rows = N*H*W, C], the channel the fastest index — what MIOpen's NHWC
 * convolution kernels read and write without a layout transpose): same arithmetic, same rounding. */
int detops_frozen_bn_act_forward_nhwc(const void* x, const float* scale, const float* bias,
                                      const void* residual, void* y, int dtype, int64_t rows, int C,
                                      int relu, detops_stream_t stream);

int detops_frozen_bn_act_backward_nhwc(const void* grad_y, const void* y, const float* scale,
                                       void* grad_x, void* grad_residual, int dtype, int64_t rows, int C,
                                       int relu, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 1x1 convolution with the FrozenBatchNorm affine (+ residual) (+ ReLU) as its epilogue (csrc/conv1x1_bn.hip): the
 * backbone bottleneck's conv1 + bn1, conv3 + bn3 (+ identity) and projection shortcut in ONE launch each, fp32, channels-last:
 *   y[n, ho, wo, k] = [relu]( (sum_c x[n, ho*stride, wo*stride, c] * w[k, c]) * scale[k] + bias[k] [+ residual[n, ho, wo, k]] )
 * with Ho = (H - 1) / stride + 1, Wo likewise.  The sum runs on the fp32 matrix units (no reduced-precision mode); the
 * epilogue rounds like detops_frozen_bn_act_forward_nhwc (product, sum and residual add rounded separately), so the result
 * differs from convolution + that call only by the convolution's own summation order.
 *   x [N, H, W, C]; w [K, C] (a [K, C, 1, 1] weight in either memory format); scale, bias [K]; residual (nullable), y
 *   [N, Ho, Wo, K]; all fp32, dense, 16-byte aligned; groups 1, no padding, no dilation; stride 1 | 2 (2: no residual);
 *   C % 4 == 0, K % 4 == 0, every tensor below 2^31 elements.
 *   config: 0 = the library's per-shape routing table, 1 = 64 x 128 tile (32x32x2 MFMA), 2 = 64 x 64 tile (16x16x4 MFMA).
 * detops_conv1x1_frozen_bn_act_supported -> the tile configuration that serves the shape (1 | 2), or 0: with config 0 also
 *   when the table keeps the shape on the two-launch path (measured not slower there); always 0 in a build without the
 *   composable_kernel headers.  Needs a current HIP device.
 * _forward_nhwc_f32: DETOPS_EUNSUPPORTED with nothing launched for whatever `_supported` answers 0 to and for a misaligned
 *   pointer.  Puts nothing on the stream but the one kernel launch (no allocation, memset or synchronisation).
 * ---------------------------------------------------------------------------------------- */
int detops_conv1x1_frozen_bn_act_supported(int N, int C, int H, int W, int K, int stride, int residual, int config);
int detops_conv1x1_frozen_bn_act_forward_nhwc_f32(const float* x, const float* w, const float* scale, const float* bias,
                                                  const float* residual, float* y, int N, int C, int H, int W, int K,
                                                  int stride, int relu, int config, detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bias (+ ReLU) behind a channels-last convolution (csrc/bias_act.hip) — `conv + bias [+ relu]` of the detector's biased
 * convolutions (reference modeling/backbone/fpn.py:30-40, modeling/rpn/rpn.py:61-76, roi_heads/mask_head): the forward is
 * detops_frozen_bn_act_forward_nhwc with scale 1; the backward is one pass over the gradient:
 *   g = relu ? (y > 0 ? grad_y : 0) : grad_y ;  grad_x = g (may alias grad_y when relu = 0) ;  grad_bias[c] = sum_rows g[., c]
 * x, y, grad_* are [rows = N*H*W, C] fp32 (16-byte aligned); C must satisfy detops_bias_act_supported (a multiple of 4
 * dividing 1024); deterministic (per-workgroup partial sums added in index order: `workspace` of
 * detops_bias_act_backward_workspace_bytes(rows, C) bytes), no atomics.
 * ---------------------------------------------------------------------------------------- */
int detops_bias_act_supported(int C);
size_t detops_bias_act_backward_workspace_bytes(int64_t rows, int C);
int detops_bias_act_backward_nhwc_f32(const float* grad_y, const float* y, float* grad_x, float* grad_bias, int64_t rows,
                                      int C, int relu, void* workspace, size_t workspace_bytes, detops_stream_t stream);
/* the same with fp32 / fp16 / bf16 storage (dtype code; grad_bias and the partial sums stay fp32): the autocast configurations */
int detops_bias_act_backward_nhwc(const void* grad_y, const void* y, void* grad_x, float* grad_bias, int dtype, int64_t rows,
                                  int C, int relu, void* workspace, size_t workspace_bytes, detops_stream_t stream);
/* out[c] = sum_r x[r, c] of a row-major [rows, C] fp32 matrix, any C <= 256 (bias gradients of the channel counts the fused
 * pass does not serve: the RPN's 3 / 12, the mask logits' 81); deterministic; workspace of detops_column_sum_workspace_bytes. */
size_t detops_column_sum_workspace_bytes(int64_t rows, int C);
int detops_column_sum_f32(const float* x, float* out, int64_t rows, int C, void* workspace, size_t workspace_bytes,
                          detops_stream_t stream);
int detops_column_sum(const void* x, float* out, int dtype, int64_t rows, int C, void* workspace, size_t workspace_bytes,
                      detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GroupNorm (+ residual) (+ ReLU) on channels-last activations (csrc/group_norm.hip) — the normalisation of the reference's
 * gn_baselines models (modeling/make_layers.py:24-39, backbone/resnet.py BottleneckWithGN / StemWithGN).
 *   x, residual (nullable), y, grad_*: [N, HW, C], the channel the fastest index; dtype code as above (fp32 arithmetic)
 *   G groups of C / G ADJACENT channels; gamma, beta (nullable: 1 / 0), grad_gamma, grad_beta: fp32 [C]
 *   mean, rstd: fp32 [N, G], rstd = 1 / sqrt(var + eps) with the biased variance of the group's HW * C / G elements
 *   forward : y = [relu]( (x - mean[n, g]) * rstd[n, g] * gamma[c] + beta[c] [+ residual] )
 *   backward: g = relu ? (y > 0 ? grad_y : 0) : grad_y  (y is read only with relu);  grad_residual (nullable) = g;
 *             grad_x = rstd * (gamma * g - mean_group(gamma * g) - xhat * mean_group(gamma * g * xhat));
 *             grad_gamma[c] = sum g * xhat, grad_beta[c] = sum g  (each nullable: not wanted)
 * The variance comes from (count, mean, M2) triples merged by Chan's formula in a fixed order, never from a sum of
 * squares; no atomics: two calls give identical bits.  Any pointer alignment (narrower vectors below 16 bytes).
 * detops_group_norm_supported: 1 when C % G == 0 and C / G is a power of two <= 256, else 0.  An unserved (C, G) returns
 * DETOPS_EUNSUPPORTED with nothing launched; N == 0 or HW == 0 returns 0 with nothing launched or written.
 * workspace: >= detops_group_norm_workspace_bytes(N, HW, C, G) bytes (serves either direction), else DETOPS_EWORKSPACE.
 * ---------------------------------------------------------------------------------------- */
int detops_group_norm_supported(int C, int G);
size_t detops_group_norm_workspace_bytes(int N, int64_t HW, int C, int G);
int detops_group_norm_forward_nhwc(const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                                   float* mean, float* rstd, int dtype, int N, int64_t HW, int C, int G, float eps, int relu,
                                   void* workspace, size_t workspace_bytes, detops_stream_t stream);
int detops_group_norm_backward_nhwc(const void* grad_y, const void* x, const void* y, const float* gamma, const float* mean,
                                    const float* rstd, void* grad_x, void* grad_residual, float* grad_gamma, float* grad_beta,
                                    int dtype, int N, int64_t HW, int C, int G, int relu, void* workspace,
                                    size_t workspace_bytes, detops_stream_t stream);

/* RPN loss in one pass over the head outputs (reference modeling/rpn/loss.py:92-127 with
 * modeling/box_coder.py:27-51 and modeling/rpn/utils.py:9-45): objectness = BCE-with-logits over the sampled
 * anchors, box = smooth-L1(beta) against BoxCoder.encode(matched gt, anchor) over the sampled positives, both
 * divided by max(#sampled, 1).
 *   objectness[l] [N, A, H_l, W_l], box_regression[l] [N, 4A, H_l, W_l]: the per-level head outputs as written by
 *   the heads (HOST arrays of device pointers); anchors [T, 4], T = A * sum_l H_l W_l, ordered level, y, x, a;
 *   matched_idxs [N, T] (Matcher output), pos_mask / neg_mask [N, T] (sampler output), gt_boxes [N, M, 4].
 *   grad_*[l]: same shapes as the inputs, OVERWRITTEN with d(sum of the per-anchor losses) / d(input);
 *   losses3 (device, 3 floats) = {objectness loss, box loss, 1 / max(#sampled, 1)}.
 * detops_rpn_loss_backward_f32 scales the stored gradients in place by upstream * losses3[2] (device scalars). */
size_t detops_rpn_loss_workspace_bytes(void);
int detops_rpn_loss_f32(const float* const* objectness_host, const float* const* box_regression_host,
                        const int* H_host, const int* W_host, int num_levels, int anchors_per_location,
                        const float* anchors, const int64_t* matched_idxs, const uint8_t* pos_mask,
                        const uint8_t* neg_mask, const float* gt_boxes, int N, int M, int T, float beta,
                        const float* weights4_host, float* const* grad_objectness_host,
                        float* const* grad_box_regression_host, float* losses3, void* workspace,
                        size_t workspace_bytes, detops_stream_t stream);
int detops_rpn_loss_backward_f32(float* const* grad_objectness_host, float* const* grad_box_regression_host,
                                 const int* H_host, const int* W_host, int num_levels, int anchors_per_location,
                                 int N, int T, const float* upstream_objectness, const float* upstream_box,
                                 const float* inv_count, detops_stream_t stream);

/* Sparse backward of the RPN head (modeling/rpn/rpn.py: t = relu(conv3x3(x) + b), objectness = 1x1(t), deltas = 1x1(t),
 * one set of weights over every level) for a loss gradient that is zero except at a bounded number of anchors (the
 * sampled RPN loss: <= N * BATCH_SIZE_PER_IMAGE rows).  Mathematically the dense backward — exact zeros contribute
 * nothing — at the cost of the non-zero rows only; deterministic, no atomics on floating-point data, no host read-back.
 *   grad_objectness[l] [N, A, H_l, W_l], grad_box_regression[l] [N, 4A, H_l, W_l]: the incoming gradients (fp32,
 *   contiguous); x[l], t[l]: the head's input and hidden activation, CHANNELS-LAST [N, H_l, W_l, C]; grad_x[l]: same
 *   layout, written in full (zero outside the 3x3 neighbourhoods of the non-zero rows).  HOST arrays of device pointers.
 *   w_conv [C, 3, 3, C] (output channel, ky, kx, input channel: the channels-last storage of the [C, C, 3, 3] parameter),
 *   w_cls [A, C], w_box [4A, C]; grad_w_conv / grad_w_cls / grad_w_box in the same layouts, grad_b_* [C] / [A] / [4A].
 *   C must be a multiple of 4 (16-byte aligned rows); N * T and the batch's pixel count must stay below 2^31.
 *   max_rows: static capacity of the row list.  A launch that finds MORE non-zero rows stays in bounds, fills
 *   grad_w_conv with NaN (never a silently wrong step) and adds 1 to *overflow_count (device int32, never cleared by
 *   the library, may be NULL).  workspace: detops_rpn_head_backward_workspace_bytes(N, T, max_rows, C) bytes,
 *   T = A * sum_l H_l W_l. */
size_t detops_rpn_head_backward_workspace_bytes(int N, int T, int max_rows, int C);
int detops_rpn_head_backward_f32(const float* const* grad_objectness_host, const float* const* grad_box_regression_host,
                                 const float* const* x_host, const float* const* t_host, float* const* grad_x_host,
                                 const int* H_host, const int* W_host, int num_levels, int anchors_per_location, int N,
                                 int C, int T, int max_rows, const float* w_conv, const float* w_cls, const float* w_box,
                                 float* grad_w_conv, float* grad_b_conv, float* grad_w_cls, float* grad_b_cls,
                                 float* grad_w_box, float* grad_b_box, int32_t* overflow_count, void* workspace,
                                 size_t workspace_bytes, detops_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * CPU branch — HOST pointers, no stream.  The reference `_C` serves exactly two operators for CPU tensors
 * (csrc/nms.h:19-27 -> csrc/cpu/nms_cpu.cpp, csrc/ROIAlign.h:19-24 -> csrc/cpu/ROIAlign_cpu.cpp) and raises
 * "Not implemented on the CPU" for the rest; so does this library.  These are NOT a fallback of the device entry
 * points (which never call them and fail when there is no GPU); they exist so that a caller holding CPU tensors
 * gets the reference's behaviour from the drop-in.
 *   detops_nms_cpu_f32: keep[n] receives the kept ORIGINAL indices in ascending order, *num_keep their count.
 * ---------------------------------------------------------------------------------------- */
int detops_nms_cpu_f32(const float* boxes, const float* scores, int n, float iou_threshold,
                       int64_t* keep, int32_t* num_keep);
int detops_roi_align_forward_cpu_f32(const float* input, const float* rois, float* output, int N, int C,
                                     int H, int W, int K, int PH, int PW, float spatial_scale,
                                     int sampling_ratio);

/* ------------------------------------------------------------------------------------------
 * Deformable convolution, channels-last pipeline (extension; what the layers use for the model's shapes).
 *   reference: the same operators as above (csrc/cuda/deform_conv_cuda.cu:158-691), restructured so that every
 *   per-sampling-point operand is channel-fastest and the GEMMs are plain library GEMMs on those layouts:
 *     xT [B, H*W, C] = NHWC copy of the input                       detops_nchw_to_nhwc
 *     colT [B*Ho*Wo, kh*kw, C] deformed (and modulated) columns     detops_deformable_im2col_nhwc
 *     offset / mask gradients from colsG_T [B*Ho*Wo, kh*kw, C]      detops_deformable_coord_nhwc
 *     S_T [B*H*W, kh*kw, Cout] = transposed sampling of gT [B, Ho*Wo, Cout] (the NHWC output gradient):
 *     grad_input[b] = W2T [C, kh*kw*Cout] x S_T[b]^T                 detops_deformable_transposed_sample
 *   detops_deformable_nhwc_supported: 1 when these kernels serve the shape (deformable_group == 1, C and Cout
 *   16-byte-vector counts that are powers of two in [16, 256]); otherwise use the reference-layout entry points.
 *   dtype: DETOPS_F32 / F16 / BF16; offset [B, 2*kh*kw, Ho, Wo] and mask [B, kh*kw, Ho, Wo] (NULL = v1) as above.
 * ---------------------------------------------------------------------------------------- */
int detops_nchw_to_nhwc(const void* in, void* out, int dtype, int B, int C, int HW, detops_stream_t stream);
int detops_deformable_nhwc_supported(int dtype, int C, int Cout, int deformable_group);
int detops_deformable_im2col_nhwc(const void* xT, const void* offset, const void* mask, void* colT, int dtype,
                                  int B, int C, int H, int W, int kh, int kw, int pad_h, int pad_w, int stride_h,
                                  int stride_w, int dil_h, int dil_w, int deformable_group, detops_stream_t stream);
int detops_deformable_coord_nhwc(const void* colsG_T, const void* xT, const void* offset, const void* mask,
                                 void* grad_offset, void* grad_mask, int dtype, int B, int C, int H, int W, int kh,
                                 int kw, int pad_h, int pad_w, int stride_h, int stride_w, int dil_h, int dil_w,
                                 int deformable_group, detops_stream_t stream);
size_t detops_deformable_transposed_sample_workspace_bytes(int B, int C, int H, int W, int kh, int kw, int pad_h, int pad_w,
                                                 int stride_h, int stride_w, int dil_h, int dil_w, int deformable_group);
int detops_deformable_transposed_sample(const void* gT, const void* offset, const void* mask, void* S_T, int dtype, int B, int C,
                              int H, int W, int Cout, int kh, int kw, int pad_h, int pad_w, int stride_h, int stride_w,
                              int dil_h, int dil_w, int deformable_group, void* workspace, size_t workspace_bytes,
                              detops_stream_t stream);
/* grad_in_T [B, H*W, C] = col2im of the channel-fastest column gradient colsG_T [B*Ho*Wo, kh*kw, C] as a gather over the same
 * inverted index (reference col2im: csrc/cuda/deform_conv_kernel_cuda.cu:353-413, an atomic scatter): no S_T, no second GEMM.
 * workspace: detops_deformable_transposed_sample_workspace_bytes(...). */
int detops_deformable_col2im_nhwc(const void* colsG_T, const void* offset, const void* mask, void* grad_in_T, int dtype, int B,
                                  int C, int H, int W, int kh, int kw, int pad_h, int pad_w, int stride_h, int stride_w,
                                  int dil_h, int dil_w, int deformable_group, void* workspace, size_t workspace_bytes,
                                  detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The data-parallel step's bucket kernels (csrc/optim.hip) — replace, per gradient bucket of engine/ddp_step.py, the
 * multi-tensor copy into the bucket and torch.optim.SGD's update (reference: tools/train_net.py:45-54 wraps the model in
 * DistributedDataParallel, engine/trainer.py:93-99 `optimizer.step()`, solver/build.py:7-20 the two hyper-parameter
 * groups).  A bucket is three flat fp32 arrays of one layout: parameters, gradients, momentum.
 *   detops_pack_f32: dst[dst_offsets[i] .. + counts[i]) = srcs[i][0 .. counts[i]) for i < n <= detops_pack_max_tensors();
 *     srcs / counts / dst_offsets are HOST arrays (the pointers travel in the kernel arguments), srcs[i] device pointers.
 *   detops_sgd_momentum_flat_f32: for every element  g' = g + wd * p;  m = momentum * m + g';  p = p - lr * m
 *     (torch.optim.SGD with dampening 0, no Nesterov; the momentum array starts as zeros, which makes the first step
 *     m = g' like torch's), with (lr, wd) = the weights' pair on [0, split) and the biases' pair on [split, n);
 *     split a multiple of 4, all three arrays 16-byte aligned.
 * ---------------------------------------------------------------------------------------- */
int detops_pack_max_tensors(void);
int detops_pack_f32(const void* const* srcs, const int64_t* counts, const int64_t* dst_offsets, int n, float* dst,
                    detops_stream_t stream);
int detops_sgd_momentum_flat_f32(float* params, const float* grads, float* momentum_buf, int64_t n, int64_t split,
                                 float lr_weights, float wd_weights, float lr_biases, float wd_biases, float momentum,
                                 detops_stream_t stream);
/* Measurement tool (not on the training path): `workgroups` workgroups of 1024 threads hold their CUs' wave slots for
 * `microseconds` on `stream` — a one-GPU stand-in for the CUs a ring all-reduce kernel occupies beside the compute stream at
 * N > 1 (engine/ddp_step.py: DETOPS_DDP_STANDIN, profiles/r06_ddp_contention.txt). */
int detops_debug_occupy(int workgroups, int microseconds, detops_stream_t stream);
/* diagnosis: wall-clock timeline (10 ns ticks) of segment 0 in the last single-launch NMS that ran with tuning nms_debug & 4
 * (csrc/nms.hip g_nms_timeline); host_out: n <= 6464 words.  Synchronises the device. */
int detops_debug_nms_timeline(int64_t* host_out, int n);

/* ------------------------------------------------------------------------------------------
 * FPN top-down step (csrc/fpn_topdown.hip) — replaces the pair `F.interpolate(last_inner, mode="nearest")` +
 * `inner_lateral + inner_top_down` of reference modeling/backbone/fpn.py:59-64 (and its backward: identity towards the
 * lateral, block sum towards the coarser map).  NCHW planes (= N * C), lateral / out [planes, H, W], top [planes, h, w];
 * dtype DETOPS_F32 / F16 / BF16 for all tensors of a call, fp32 arithmetic; nearest index = ATen's
 * min(int(floorf(dst * (float)in / out)), in - 1).  backward: grad_top [planes, h, w] is OVERWRITTEN.
 * ---------------------------------------------------------------------------------------- */
int detops_fpn_topdown_forward(const void* lateral, const void* top, void* out, int dtype, int planes, int H, int W, int h, int w,
                               detops_stream_t stream);
int detops_fpn_topdown_backward(const void* grad_out, void* grad_top, int dtype, int planes, int H, int W, int h, int w,
                                detops_stream_t stream);
/* channels-last form: lateral / out / grad_out [N, H, W, C], top / grad_top [N, h, w, C] */
int detops_fpn_topdown_forward_nhwc(const void* lateral, const void* top, void* out, int dtype, int N, int C, int H, int W,
                                    int h, int w, detops_stream_t stream);
int detops_fpn_topdown_backward_nhwc(const void* grad_out, void* grad_top, int dtype, int N, int C, int H, int W, int h, int w,
                                     detops_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Double precision (csrc/f64_ops.hip, csrc/cpu_branch.hip) — the reference dispatches these operators over
 * AT_DISPATCH_FLOATING_TYPES, i.e. float AND double (csrc/cuda/ROIAlign_cuda.cu:283,329, ROIPool_cuda.cu:137,185,
 * SigmoidFocalLoss_cuda.cu:129,173, csrc/cpu/ROIAlign_cpu.cpp:242, csrc/cpu/nms_cpu.cpp:71).  Same argument meaning as the
 * _f32 entry points; plain one-thread-per-element kernels with the reference's arithmetic in double (API completeness: no
 * configuration of the training path computes in double).  detops_nms_sorted_f64 takes boxes already sorted by descending
 * score and returns a byte per sorted box (1 = kept); the two *_cpu_f64 entry points are host code for CPU tensors.
 * ---------------------------------------------------------------------------------------- */
int detops_roi_align_forward_f64(const double* input, const double* rois, double* output, int N, int C, int H, int W, int K,
                                 int PH, int PW, float spatial_scale, int sampling_ratio, detops_stream_t stream);
int detops_roi_align_backward_f64(const double* grad_out, const double* rois, double* grad_in, int N, int C, int H, int W,
                                  int K, int PH, int PW, float spatial_scale, int sampling_ratio, int zero_grad_in,
                                  detops_stream_t stream);
int detops_roi_pool_forward_f64(const double* input, const double* rois, double* output, int32_t* argmax, int N, int C, int H,
                                int W, int K, int PH, int PW, float spatial_scale, detops_stream_t stream);
int detops_roi_pool_backward_f64(const double* grad_out, const double* rois, const int32_t* argmax, double* grad_in, int N,
                                 int C, int H, int W, int K, int PH, int PW, int zero_grad_in, detops_stream_t stream);
int detops_sigmoid_focal_loss_forward_f64(const double* logits, const int32_t* targets, double* losses, int num_rows,
                                          int num_classes, float gamma, float alpha, detops_stream_t stream);
int detops_sigmoid_focal_loss_backward_f64(const double* logits, const int32_t* targets, const double* d_losses,
                                           double* d_logits, int num_rows, int num_classes, float gamma, float alpha,
                                           detops_stream_t stream);
size_t detops_nms_sorted_f64_workspace_bytes(int n);
int detops_nms_sorted_f64(const double* sorted_boxes, int n, float iou_threshold, unsigned char* keep_sorted, void* workspace,
                          size_t workspace_bytes, detops_stream_t stream);
int detops_roi_align_forward_cpu_f64(const double* input, const double* rois, double* output, int N, int C, int H, int W,
                                     int K, int PH, int PW, float spatial_scale, int sampling_ratio);
int detops_nms_cpu_f64(const double* boxes, const double* scores, int n, float iou_threshold, int64_t* keep,
                       int32_t* num_keep);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* DETOPS_H_ */
