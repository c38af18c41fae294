/*
 * sniper_hip.h -- C ABI of libsniper_hip.so, the MI355X (gfx950) kernel library behind the SNIPER
 * hot path.  Plain C: pointers, sizes, no C++/torch types.
 *
 * Conventions ("Inner boundary"):
 *   - every pointer named d_* / documented "device" is a HIP device pointer owned by the caller;
 *   - no allocation and no synchronisation inside any call: kernels are enqueued on `stream` (a hipStream_t passed
 *     as void*; NULL = default stream) and the call returns; the calls are re-entrant per stream and per device;
 *   - process-wide state is limited to the explicit test / tuning hooks sn_debug_option, sn_conv_tune,
 *     sn_conv_wgrad_impl, sn_conv_trace and sn_conv_wgrad_trace (atomics, defaults = production behaviour; their
 *     environment-variable spellings are read ONCE at load time) -- no hot call reads the environment or mutates a
 *     global; the per-device "large LDS" opt-in of two kernels is applied once per (kernel, device) under a mutex;
 *   - scratch memory comes from the caller: sn_*_workspace_bytes() tells how much;
 *   - return value: 0 = ok, SN_ERR_* otherwise (argument errors are detected before any launch).
 * The only native ABI the reference itself defines is
 *     void _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
 *               float nms_overlap_thresh, int device_id);            (lib/nms/gpu_nms.hpp:1-2)
 * which sn_nms_host() replaces one-to-one; everything else replaces a Cython/C++ extension entry
 * point or an operator of the un-vendored SNIPER-mxnet fork and cites it below.
 */
#ifndef SNIPER_HIP_H
#define SNIPER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *sn_stream_t; /* hipStream_t */

enum { SN_OK = 0, SN_ERR_ARG = 1, SN_ERR_HIP = 2, SN_ERR_WORKSPACE = 3, SN_ERR_UNSUPPORTED = 4 };

/* Library / device sanity. */
int sn_version(void);
const char *sn_last_error(void); /* thread-local text of the last failure */
/* Test switch (process-wide, atomic; no reference counterpart): "proposal_full_sort" = 1 orders the proposals with the
 * general global-memory bitonic sort instead of radix select + LDS sort, "nms_full_mask" = 1 runs the full bitmask + scan
 * instead of the lazy kernel, "conv_no_persist" = 1 gives every convolution workgroup one output tile (no persistent tile loop),
 * "softmax_strided" = 1 sends the inner == 1 calls of sn_softmax_fwd / sn_softmax_output_bwd down the one-thread-per-position
 * kernels instead of the row-block kernels.  Results are identical either way (that is what the tests use it for; environment
 * spellings, read once at load: SNIPER_FULL_SORT, SNIPER_NMS_FULL, SNIPER_CONV_NO_PERSIST, SNIPER_SOFTMAX_STRIDED).  Any other
 * name is an error. */
int sn_debug_option(const char *name, int value);

/* ------------------------------------------------------------------ box geometry ------------- */
/* bbox_overlaps_cython / ignore_overlaps_cython (lib/bbox/bbox.pyx:17-57, 59-95).
 * boxes (N,4) f64, query (K,4) f64 -> out (N,K) f64 row-major.  mode 0 = IoU, 1 = intersection/query-area. */
int sn_iou_f64(const double *d_boxes, int N, const double *d_query, int K, double *d_out, int mode, sn_stream_t stream);

/* ------------------------------------------------------------------ chip generation ---------- */
/* chips::cgenerate (lib/chips/cchips.cpp:54-177) for a ragged batch of U (image, scale) units.
 *   d_boxes       (total_boxes,4) f32, already scaled + clipped (chip_generator.py:24);
 *   d_box_off     (U+1) i32 prefix offsets into d_boxes;
 *   d_meta        (U,4) i32 = width, height, chipsize, stride;
 *   d_perm        (total_cand) i32 candidate order after the shuffle of cchips.cpp:117, or NULL for identity;
 *   d_cand_off    (U+1) i32 prefix offsets into d_perm (= candidate counts, sn_chips_num_candidates);
 *   d_mask_ws     workspace, sn_chips_workspace_bytes(total_cand, max_boxes_per_unit);
 *   d_out_chips   (total_boxes,4) f32: unit u writes its chips at row d_box_off[u] (a unit never
 *                 selects more chips than it has boxes);  d_out_ids same layout, slot index in the
 *                 shuffled candidate list;  d_out_count (U) i32.
 */
int sn_chips_num_candidates(int width, int height, int chipsize, int stride);
size_t sn_chips_workspace_bytes(int total_cand, int max_boxes_per_unit);
int sn_chips_generate_batch(const float *d_boxes, const int32_t *d_box_off, const int32_t *d_meta, const int32_t *d_perm,
                            const int32_t *d_cand_off, int U, int max_boxes_per_unit, void *d_mask_ws, float *d_out_chips,
                            int32_t *d_out_ids, int32_t *d_out_count, sn_stream_t stream);

/* Box -> chip assignment of chip_worker.box_assigner (lib/data_utils/data_workers.py:516-535, 557-572) for a
 * ragged batch of U (image, scale) units: d_chips (total_chips,4) f64 + d_chip_off (U+1); d_boxes (total_boxes,4)
 * f64 + d_box_off (U+1) + d_unit_of_box (total_boxes); d_range (U,2) f64 valid range; d_mode (U) 0 = coarsest
 * (area >= lo), 1 = area <= hi, 2 = area < hi.  d_out_chip (total_boxes): chip index inside the unit or -1. */
int sn_assign_boxes_batch(const double *d_chips, const int32_t *d_chip_off, const double *d_boxes, const int32_t *d_box_off,
                          const double *d_range, const int32_t *d_mode, const int32_t *d_unit_of_box, int U, int total_boxes,
                          int32_t *d_out_chip, sn_stream_t stream);

/* ------------------------------------------------------------------ RPN anchor labelling ----- */
/* anchor_worker.worker (lib/data_utils/data_workers.py:164-371) + the dense scatter of
 * MNIteratorE2E._get_batch (lib/iterators/MNIteratorE2E.py:175-194), batched over B chips.
 * Geometry is fixed per call: F x F feature cells, A anchors per cell, d_base_anchors (A,4) f64 =
 * generate_anchors() output, feat_stride, chip height/width (im_info).
 * Per chip b:
 *   d_gt         (B,G,4) f32 GT boxes in image coordinates (rows >= d_ngt[b] ignored), G <= 128
 *   d_gt_cls     (B,G)   f32 class id
 *   d_gt_inchip  (B,G)   u8  1 if that GT row is in props_in_chips of this chip (gtids ∩ nids)
 *   d_ngt        (B)     i32
 *   d_crop       (B,2)   f64 chip origin x,y in image coordinates;  d_scale (B) f32 im_scale
 * Sub-sampling (data_workers.py:327-338): the kept fg / bg anchors are those with the smallest
 * 47-bit key (d_keys[b][anchor] << 15 | anchor); d_keys (B, A*F*F) u32 in reference anchor order
 * (cell-major, anchor-minor) is either supplied by the host (bit-exact replay of numpy's draws) or
 * NULL, in which case keys come from a counter-based hash of (seed, b, anchor).
 * Outputs (all device, layouts of the reference batch tensors):
 *   d_label (B, A*F*F) f32 in (a,y,x) order, values {-1,0,1};
 *   d_bbox_target, d_bbox_weight (B, 4A, F, F) f32;  d_gt_out (B,100,5) f32 (-1 padded);
 *   d_counts (B,4) i32 = n_inside, n_fg_before, n_bg_before, n_valid_gt  (diagnostics / host RNG replay);
 *   d_label_pre (B, A*F*F) i8 optional (may be NULL): labels before sub-sampling in reference
 *   anchor order, -2 for anchors outside the chip.
 */
size_t sn_anchor_workspace_bytes(int B, int A, int F, int G);
int sn_anchor_assign(const float *d_gt, const float *d_gt_cls, const uint8_t *d_gt_inchip, const int32_t *d_ngt,
                     const double *d_crop, const float *d_scale, int B, int G, const double *d_base_anchors, int A, int F,
                     int feat_stride, int im_h, int im_w, double pos_thresh, double neg_thresh, int rpn_batch, int num_fg,
                     const uint32_t *d_keys, uint64_t seed, void *d_ws, float *d_label, float *d_bbox_target,
                     float *d_bbox_weight, float *d_gt_out, int32_t *d_counts, int8_t *d_label_pre, sn_stream_t stream);

/* AutoFocus FocusPixel labels (gen_mask, lib/data_utils/data_workers.py:165-192) for the same chip batch: d_mask (B, F*F) f32
 * in {1, -1, 0} = small object / don't care / background; thresholds TRAIN.AUTO_FOCUS_DC_LOW, _SMALL_THRESH, _DC_HIGH. */
int sn_focus_mask(const float *d_gt, const int32_t *d_ngt, const double *d_crop, const float *d_scale, int B, int G, int F,
                  int feat_stride, int im_h, int im_w, float dc_low, float small_thresh, float dc_high, float *d_mask,
                  sn_stream_t stream);

/* ------------------------------------------------------------------ NMS ----------------------- */
/* Bitmask hard NMS (lib/nms/nms_kernel.cu:34-78 mask, :118-140 scan; IoU > thresh suppresses),
 * batched: d_boxes (B, N, dim) f32 sorted by descending score, rows >= d_n[b] ignored (d_n may be
 * NULL = all N).  Keeps at most max_keep survivors (<=0: N).  d_keep (B, max_keep) i32 row indices,
 * d_nkeep (B) i32.  The mask never leaves the device. */
size_t sn_nms_workspace_bytes(int B, int N);
int sn_nms_batch(const float *d_boxes, const int32_t *d_n, int B, int N, int dim, float thresh, int max_keep, void *d_ws,
                 int32_t *d_keep, int32_t *d_nkeep, sn_stream_t stream);
/* Drop-in for the reference's _nms() (host buffers, synchronous, allocates like the original).
 * Returns 0/err; keep_out[num_out] are row indices into the (sorted) input. */
int sn_nms_host(int *keep_out, int *num_out, const float *boxes_host, int boxes_num, int boxes_dim,
                float nms_overlap_thresh, int device_id);

/* Soft-NMS (cpu_soft_nms, lib/nms/cpu_nms.pyx:17-110; method 1 linear, 2 gaussian, else hard) for P independent
 * problems: d_boxes (total_rows,5) f32 [x1,y1,x2,y2,score], problem p owns rows [d_off[p], d_off[p+1]), max_n = the
 * largest problem.  No size cap, like the reference: problems of at most sn_soft_nms_max_boxes() boxes run out of one
 * workgroup's LDS; larger ones run the same phases in global memory and need d_ws =
 * sn_soft_nms_workspace_bytes(total_rows) of scratch (NULL is accepted when max_n fits).  In place, like the reference: on
 * return rows [d_off[p], d_off[p] + d_count[p]) are the surviving boxes in the reference's order with their decayed scores. */
size_t sn_soft_nms_max_boxes(void);
size_t sn_soft_nms_workspace_bytes(size_t total_rows);
int sn_soft_nms_batch(float *d_boxes, const int32_t *d_off, int P, int max_n, size_t total_rows, float sigma, float Nt,
                      float threshold, int method, void *d_ws, int32_t *d_count, sn_stream_t stream);

/* ------------------------------------------------------------------ test-time host loops ----- */
/* im_worker.worker / worker_autofocus after the decode (lib/data_utils/data_workers.py:49-121): d_src_bgr (H,W,3) u8,
 * flip, crop [x1,x2) x [y1,y2) (clamped to the image), cv2.resize(fx = fy = scale, INTER_LINEAR) in OpenCV's 8-bit
 * fixed-point arithmetic (scale is the double the reference passes as fx / fy), zero padded (3,out_h,out_w) f32 with
 * channel j = BGR[2-j] - pixel_means_bgr3[2-j] (host array of 3 doubles: numpy subtracts in float64).  resized_hw2
 * (host, may be NULL) receives the resized height, width (im_info).  Bit-exact against oracle/cv_resize.py, the
 * restatement of OpenCV's published algorithm. */
int sn_im_prepare(const uint8_t *d_src_bgr, int src_h, int src_w, int crop_x1, int crop_y1, int crop_x2, int crop_y2, double scale,
                  int flip, const double *pixel_means_bgr3, float *d_out, int out_h, int out_w, int32_t *resized_hw2,
                  sn_stream_t stream);
/* bbox_pred + clip_boxes + /scale as applied per chip by lib/inference.py:127-131 (lib/bbox/bbox_transform.py:93-130,35-50):
 * rois (B*R,5) f32 with rows of chip b contiguous, deltas (B,R,4) f32, im_info (B,3) f32 -> boxes (B,R,4) f64. */
int sn_bbox_decode(const float *d_rois, const float *d_deltas, const float *d_im_info, double *d_boxes, int B, int R,
                   sn_stream_t stream);
/* Bounding rectangles (x, y, w, h) of the contours cv2.findContours(mask, RETR_LIST) reports for a 0 / non-zero HOST mask, with
 * cv2.boundingRect: mode 0 = border following (Suzuki & Abe 1985, OpenCV contours.cpp), in cv2's order (newest contour first) --
 * what sn_focus_chips_host walks; mode 1 = 8-connected components + enclosed 4-connected background components grown by one cell,
 * raster order (the independent cross-check: same rectangles).  rects_xywh (cap,4) i32. */
int sn_focus_rects_host(const uint8_t *mask_hw, int H, int W, int mode, int32_t *rects_xywh, int cap, int32_t *n_rects);
/* `gmask` of lib/chips/chips_inference.py:12-89 on the HOST (no device work, no stream): FocusPixel map (H,W) f32 -> FocusChips.
 * threshold (>= thresh), cv2.dilate d x d, bounding rectangles of the RETR_LIST contours (8-connected components + holes), minimum
 * side ms cells, paint-and-repeat until the chip count is stable, x16, clamp to (im_width, im_height), / cscale.
 * chips_xyxy (max_chips,4) f64 host, n_chips host.  Restatement of the cv2 calls: parity unpinned (no OpenCV here). */
int sn_focus_chips_host(const float *map_hw, int H, int W, int d, float thresh, int ms, double im_width, double im_height,
                        double cscale, double *chips_xyxy, int max_chips, int32_t *n_chips);
/* The regrouping half of Tester.aggregate (lib/inference.py:166-190) on the HOST in one pass: parts = the chips of all scales as
 * sn_det_compact returned them (part_rows[p] = address of float64 (n_p,5) rows grouped by class, lens (P,nc) rows per class), the
 * parts of image i = part_of_image[i] .. part_of_image[i+1]-1 in (scale, chip) order, range2 (P,2) f32 = the scale's valid range
 * squared (<= 0: no bound; areas and comparisons in float32, _valid_range_filter :176-186).  -> out_rows (total,5) f32: the rows of
 * all (image, class) problems back to back in (image, class, scale, chip, row) order; out_sizes (num_images*nc) rows per problem. */
int sn_aggregate_problems_host(const uint64_t *part_rows, const int64_t *lens, const int32_t *part_of_image, const float *range2,
                               int P, int nc, int num_images, float *out_rows, long capacity_rows, int64_t *out_sizes,
                               int64_t *total_rows);
/* The same regrouping ON THE DEVICE, over the rows sn_det_compact left in HBM (Tester.aggregate, lib/inference.py:166-190): d_parts
 * = P records {const double *rows; const int32_t *counts; float lo2, hi2;} (device addresses of one chip's float64 rows grouped
 * by class and its nc rows-per-class; the scale's valid range squared as float32, <= 0: no bound), in (image, scale, chip) order.
 * sn_aggregate_count -> d_kept (P,nc) i32: rows of (part, class) inside the range; the caller scans them into d_dst_off (P,nc):
 * first row of (part, class) in the stacked output, (image, class, scale, chip) order; sn_aggregate_scatter writes the rows that
 * pass, narrowed to float32, there in order -- the array sn_soft_nms_batch takes.  Equal to sn_aggregate_problems_host. */
int sn_aggregate_count(const void *d_parts, int P, int nc, int32_t *d_kept, sn_stream_t stream);
int sn_aggregate_scatter(const void *d_parts, int P, int nc, const int32_t *d_dst_off, float *d_out_rows, sn_stream_t stream);
/* TEST.MAX_PER_IMAGE (lib/inference.py:203-211) on the device, after the NMS: problems q = image*nc + class hold d_count[q] rows
 * at d_off[q]; an image with more than max_per_image rows over its classes keeps, per class, the rows whose score reaches the
 * max_per_image-th best score of the image (ties stay) -- in place, in order; d_count is updated. */
int sn_det_cap_per_image(float *d_rows, const int32_t *d_off, int32_t *d_count, int num_images, int nc, int max_per_image,
                         sn_stream_t stream);
/* The per-class score threshold of Tester.get_detections (lib/inference.py:289-295: inds = where(scores[:, j] > thresh), rows
 * hstack(boxes[inds, 0:4], scores[inds, j])) and, when h_crops != NULL, the AutoFocus border pruning that follows it (:336-353,
 * check_valid :236-259: rows shifted by the chip origin, dropped within `delta` px of a chip border that is not an image
 * border), for the B <= 64 chips of a batch.  scores (B,R,NC) f32, boxes (B,R,4) f64 (sn_bbox_decode); h_crops (B,4) f64 and
 * h_im_wh (B,2) f64 are HOST arrays (chip [x1,y1,x2,y2] in image coordinates; image width, height), passed to the kernel by
 * value.  -> rows (B,(NC-1)*R,5) f64: the surviving rows of chip b, grouped by class 1..NC-1, RoIs ascending inside a class;
 * counts (B,NC-1) i32 rows per class.  float64 adds and compares only: bit-exact with the numpy loops. */
int sn_det_compact(const float *d_scores, const double *d_boxes, const double *h_crops, const double *h_im_wh, float thresh,
                   double delta, int B, int R, int NC, double *d_rows, int32_t *d_counts, sn_stream_t stream);

/* ================================================================ network operators ===========
 * The graph operators of the un-vendored SNIPER-mxnet fork, at the call sites of
 * symbols/faster/resnet_mx_101_e2e.py / mobilenetv2_e2e.py.  Activations are channels-last fp16
 * ("NHWC", explicit pixel stride in elements so a tensor may be a channel slice of a wider buffer);
 * loss-side tensors are fp32 in the reference's NCHW order.  Weights are [Cout][KH*KW][Cin].
 * dtype codes: 0 = fp16, 1 = fp32. */

/* Convolution / FullyConnected forward (resnet_mx_101_e2e.py:43-66,147-155,256,288-303).
 * y[n,oy,ox,co] = bias[co] + residual + sum x[n, oy*s-p+kh*d, ox*s-p+kw*d, ci] * w[co][kh*KW+kw][ci];
 * optional ReLU; output fp16 or fp32.  FC = 1x1 convolution over H=W=1. */
int sn_conv_fwd(const void *x, const void *w, const float *bias, const void *residual, void *y, int N, int H, int W, int Cin,
                int in_pix_stride, int Cout, int out_pix_stride, int res_pix_stride, int KH, int KW, int stride, int pad, int dil,
                int relu, int out_f32, sn_stream_t stream);
/* sn_conv_fwd (fp16 output) with the contraction split over several copies of the tile grid, for launches with far fewer output
 * tiles than CUs (test-time batches of two FocusChips: 82 tiles on 256 CUs, each a latency-bound chain of K-steps): fp32 partial
 * tiles in `ws`, added in split order together with bias / residual / ReLU (deterministic).  The workspace query returns 0 when the
 * layer would not be split (enough tiles, a short contraction, a layer the pipelined kernel does not take): call sn_conv_fwd then --
 * sn_conv_fwd_splitk itself also falls back to it.  Same operator as sn_conv_fwd (symbols/faster/resnet_mx_101_e2e.py:43-66 at
 * test time, BatchNorm folded); the sum is formed in fp32 across the splits and rounded once. */
size_t sn_conv_fwd_splitk_workspace_bytes(int N, int H, int W, int Cin, int in_pix_stride, int Cout, int out_pix_stride,
                                          int res_pix_stride, int KH, int KW, int stride, int pad, int dil);
int sn_conv_fwd_splitk(const void *x, const void *w, const float *bias, const void *residual, void *y, int N, int H, int W, int Cin,
                       int in_pix_stride, int Cout, int out_pix_stride, int res_pix_stride, int KH, int KW, int stride, int pad,
                       int dil, int relu, void *ws, size_t ws_bytes, sn_stream_t stream);
/* ... with an fp32 result and no residual (sn_conv_fwd's out_f32 = 1): the offset FullyConnected of the deformable RoI pooling
 * (resnet_mx_101_e2e.py:288-291: 2 x 7 x 7 = 98 outputs over the RoIs of a test batch -- 10 tiles, 196 K-steps each -- read as the
 * pooling's fp32 `trans`).  Any Cout; same workspace query. */
int sn_conv_fwd_splitk_f32(const void *x, const void *w, const float *bias, float *y, int N, int H, int W, int Cin, int in_pix_stride,
                           int Cout, int out_pix_stride, int KH, int KW, int stride, int pad, int dil, int relu, void *ws,
                           size_t ws_bytes, sn_stream_t stream);
/* Forward convolution with a SECOND output (test-time residual units): y as sn_conv_fwd / sn_conv_fwd_splitk write it (fp16) and
 * y2 = act(y2_scale * y + y2_shift) of the stored y, fp16, pixel stride y2_pix_stride -- the moving-statistics BatchNorm + ReLU that
 * opens the next pre-activation unit (resnet_mx_101_e2e.py:38-40) and reads the residual sum this epilogue writes.  ws / ws_bytes:
 * the split-K scratch of sn_conv_fwd_splitk_workspace_bytes (0 / NULL: never split).  sn_conv_fwd_dual_ok -> 1 when the layer
 * qualifies (pipelined kernel, 16-byte rows), else use sn_conv_fwd + sn_bn_apply. */
int sn_conv_fwd_dual_ok(int N, int H, int W, int Cin, int in_pix_stride, int Cout, int out_pix_stride, int res_pix_stride, int KH,
                        int KW, int stride, int pad, int dil, int y2_pix_stride);
int sn_conv_fwd_dual(const void *x, const void *w, const float *bias, const void *residual, void *y, int N, int H, int W, int Cin,
                     int in_pix_stride, int Cout, int out_pix_stride, int res_pix_stride, int KH, int KW, int stride, int pad, int dil,
                     int relu, void *y2, int y2_pix_stride, const float *y2_scale, const float *y2_shift, int y2_relu, void *ws,
                     size_t ws_bytes, sn_stream_t stream);
/* Kernel-selection override for sn_conv_fwd / sn_conv_dgrad (tuning hook, tools/conv_tune.py; no reference counterpart):
 * -1 = built-in per-layer table (default), 0 = the register-staged kernel only, 4 / 5 / 6 / 7 / 14 / 16 / 18 = that LDS-DMA tile
 * configuration for every layer that qualifies (see conv_dma.hip; other numbers are rejected).  Results are identical up to fp32 summation order inside a tile's K loop
 * (the K order itself does not change).  Process-wide; set it while no launch is in flight. */
int sn_conv_tune(int cfg);

/* sn_conv_fwd that also emits the BatchNorm statistics of its fp16 output (sum and sum of squares of the STORED values per
 * row tile): stats (blocks, 2, Cout) fp32, blocks = sn_conv_fwd_stats_blocks(...) (0: the layer does not qualify -- narrow or
 * unaligned layers -- use sn_conv_fwd + sn_bn_stats).  Consumed by sn_bn_finalize_blocks: the batch-statistics pass of
 * BatchNorm(train) after a convolution (resnet_mx_101_e2e.py:38-66) costs no extra read of the tensor. */
int sn_conv_fwd_stats_blocks(int N, int H, int W, int Cin, int in_pix_stride, int Cout, int out_pix_stride, int res_pix_stride,
                             int KH, int KW, int stride, int pad, int dil);
int sn_conv_fwd_stats(const void *x, const void *w, const float *bias, const void *residual, void *y, int N, int H, int W, int Cin,
                      int in_pix_stride, int Cout, int out_pix_stride, int res_pix_stride, int KH, int KW, int stride, int pad,
                      int dil, int relu, float *stats, sn_stream_t stream);
/* conv0 on the packed stem input (xp (N,Hp,Wp,4) fp16 from sn_pack_stem_input; w [Cout][KH][KWP*4]). */
int sn_conv_stem_fwd(const void *xp, const void *w, const float *bias, void *y, int N, int Hp, int Wp, int Ho, int Wo, int Cout,
                     int out_pix_stride, int KH, int KWP, int stride, int relu, int out_f32, sn_stream_t stream);
/* Weight gradient of the stem convolution, accumulated into the packed fp32 weight [Cout][KH][KWP*4].  The pixel range is
 * split over workgroups whose partials go to `ws` (sn_conv_stem_wgrad_workspace_bytes) and are summed in split order --
 * deterministic, no atomics; without scratch the layer runs unsplit. */
size_t sn_conv_stem_wgrad_workspace_bytes(int N, int Ho, int Wo, int Cout, int KH, int KWP);
int sn_conv_stem_wgrad(const void *dy, const void *xp, float *dw, int N, int Hp, int Wp, int Ho, int Wo, int Cout, int dy_pix_stride,
                       int KH, int KWP, int stride, void *ws, size_t ws_bytes, sn_stream_t stream);
/* Data gradient; wt = weights as [Cin][KH*KW][Cout] fp16; `accumulate` (fp16, may alias dx) is added. */
int sn_conv_dgrad(const void *dy, const void *wt, const void *accumulate, void *dx, int N, int H, int W, int Cin,
                  int dx_pix_stride, int Cout, int dy_pix_stride, int acc_pix_stride, int KH, int KW, int stride, int pad, int dil,
                  int out_f32, sn_stream_t stream);
/* Test / A-B switch (process-wide, atomic): 1 (default) = the data gradient of a stride-2, dilation-1 convolution with even
 * destination dims walks its destination pixels parity class by parity class, each class only the taps that reach it (9 tap visits
 * instead of 36 for a 3x3 kernel, 1 instead of 4 for a 1x1 shortcut; same sums in the same order per pixel); 0 = every tap for
 * every pixel.  Affects the row-tile count sn_conv_dgrad_bn_blocks reports: set it before that query. */
int sn_conv_dgrad_by_class(int on);
/* sn_conv_dgrad that also emits the reduction of the BatchNorm(+activation) backward below it: dx is dL/dy of
 * y = act(BN(bn_x)) (bn_act: 0 none, 1 ReLU, 2 ReLU6), partials (blocks, 2, Cin) fp32 = per row tile sum g and sum g*(bn_x - mean)
 * with g = the stored dx masked by the activation; blocks = sn_conv_dgrad_bn_blocks(...) (0: the layer does not qualify).
 * Only valid when this convolution is y's only consumer (dx complete).  Consumed by sn_bn_backward_blocks. */
int sn_conv_dgrad_bn_blocks(int N, int H, int W, int Cin, int dx_pix_stride, int Cout, int dy_pix_stride, int acc_pix_stride, int KH,
                            int KW, int stride, int pad, int dil);
int sn_conv_dgrad_bn(const void *dy, const void *wt, const void *accumulate, void *dx, int N, int H, int W, int Cin, int dx_pix_stride,
                     int Cout, int dy_pix_stride, int acc_pix_stride, int KH, int KW, int stride, int pad, int dil, const void *bn_x,
                     int bn_x_pix_stride, const float *bn_scale, const float *bn_shift, const float *bn_mean, int bn_act,
                     float *partials, sn_stream_t stream);
/* Weight gradient, accumulated (+=) into dw fp32 [Cout][KH*KW][Cin].  Layers whose weight tensor is small relative to
 * the pixel count are split over K; with ws = sn_conv_wgrad_workspace_bytes(...) bytes of scratch the partials are
 * reduced in split order without atomics (deterministic).  ws may be NULL, or smaller than the query: the layer then
 * runs unsplit, one owner per dw element -- slower, still no atomics, the same sums in another order. */
size_t sn_conv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int x_pix_stride, int Cout, int dy_pix_stride, int KH, int KW,
                                     int stride, int pad, int dil);
int sn_conv_wgrad(const void *dy, const void *x, float *dw, int N, int H, int W, int Cin, int x_pix_stride, int Cout,
                  int dy_pix_stride, int KH, int KW, int stride, int pad, int dil, void *ws, size_t ws_bytes, sn_stream_t stream);
/* Several layers' weight gradients in ONE launch (same result as n calls of sn_conv_wgrad): a layer alone has too few output tiles
 * for 256 CUs and needs split-K partial slabs; a table of layers fills the chip with whole-K jobs.  descs: n entries of sn_wgrad_desc in host
 * memory, read during the call); scratch from sn_conv_wgrad_batch_workspace_bytes on the same table.  Replaces the weight-gradient
 * half of the fork's Convolution / FullyConnected backward (symbols/faster/resnet_mx_101_e2e.py:43-66,147-155,288-303). */
typedef struct sn_wgrad_desc {
  const void *dy, *x;
  float *dw;
  int N, H, W, Cin, x_pix_stride, Cout, dy_pix_stride, KH, KW, stride, pad, dil;
} sn_wgrad_desc;
size_t sn_conv_wgrad_batch_workspace_bytes(const sn_wgrad_desc *descs, int n);
int sn_conv_wgrad_batch(const sn_wgrad_desc *descs, int n, void *ws, size_t ws_bytes, sn_stream_t stream);
/* A/B and tuning hook: impl 1 = wave-specialised batched kernel (default), 0 = the gather kernel every layer can run on (the
 * fallback for operands that are not 16-byte addressable); job_steps = longest job in
 * 64-pixel K-steps (0 = built-in).  Set before the workspace query of the launches it affects. */
int sn_conv_wgrad_impl(int impl, int job_steps);
/* diagnostics (tools/wgrad_batch_bench.py --trace): per-job phase cycles [jobs][8] x uint64 into buf; NULL = off */
int sn_conv_wgrad_trace(void *buf);
/* diagnostics (tools/conv_trace.py): per-workgroup phase cycles [grid][8] x uint64 of the LDS-DMA forward / data-gradient
 * launches that follow into buf; NULL = off (default) */
int sn_conv_trace(void *buf);
/* bias gradient: db[c] += sum_rows dy[r][c].  Row blocks leave partial sums in `ws` (sn_bias_grad_workspace_bytes) and are added in
 * block order -- deterministic, no atomics; without scratch one block per 64 channels walks all rows. */
size_t sn_bias_grad_workspace_bytes(long rows, int C);
int sn_bias_grad(const void *dy, float *db, long rows, int C, int ld, int dtype, void *ws, size_t ws_bytes, sn_stream_t stream);

/* Stem: NCHW fp32 images -> zero padded NHWC4 fp16 with the bn_data affine folded in (:402-404). */
int sn_pack_stem_input(const float *x_nchw, void *out, int N, int C, int H, int W, int Hp, int Wp, int pad_t, int pad_l,
                       const float *scale, const float *shift, sn_stream_t stream);

/* BatchNorm (eps, momentum; :38-58).  Training statistics: sn_bn_stats writes fp32 per-row-block partials into ws
 * (sn_bn_workspace_bytes(M, C), no atomics, fixed summation order), sn_bn_finalize reduces them in double to
 * scale = gamma*invstd, shift = beta - mean*scale, the saved batch statistics and the moving averages.
 * sn_bn_backward: gradients through relu?(BN_train(x)); dgamma/dbeta are accumulated (+=); same ws size. */
size_t sn_bn_workspace_bytes(int M, int C);
int sn_bn_stats(const void *x, int M, int C, int ps, void *ws, sn_stream_t stream);
int sn_bn_finalize(const void *ws, int M, int C, float eps, float momentum, const float *gamma, const float *beta,
                   float *run_mean, float *run_var, float *scale, float *shift, float *save_mean, float *save_invstd,
                   sn_stream_t stream);
int sn_bn_finalize_blocks(const float *partials, int nblk, int M, int C, float eps, float momentum, const float *gamma,
                          const float *beta, float *run_mean, float *run_var, float *scale, float *shift, float *save_mean,
                          float *save_invstd, sn_stream_t stream);
int sn_bn_global_scale_shift(const float *gamma, const float *beta, const float *mean, const float *var, int C, float eps,
                             float *scale, float *shift, sn_stream_t stream);
int sn_bn_apply(const void *x, void *y, int M, int C, int ps_in, int ps_out, const float *scale, const float *shift, int relu,
                sn_stream_t stream); /* relu: 0 none, 1 ReLU, 2 ReLU6 = clip(0,6); same code in sn_bn_backward */
/* sn_bn_finalize_blocks + sn_bn_apply (two launches); sn_bn_backward_blocks likewise issues its finalize, then the dx pass.
 * (Folding the finalize into the applying pass measured 1.1 ms per step slower, profiles/r06_ab_bn_fused.txt, and was removed.) */
int sn_bn_apply_blocks(const float *partials, int nblk, const void *x, void *y, int M, int C, int ps_in, int ps_out, float eps,
                       float momentum, const float *gamma, const float *beta, float *run_mean, float *run_var, float *scale,
                       float *shift, float *save_mean, float *save_invstd, int relu, sn_stream_t stream);
int sn_bn_backward(const void *dy, const void *x, const void *accumulate, void *dx, int M, int C, int ps_dy, int ps_x, int ps_acc,
                   int ps_dx, const float *scale, const float *shift, const float *mean, const float *invstd, int relu, void *ws,
                   float *dgamma, float *dbeta, sn_stream_t stream);
int sn_bn_backward_blocks(const float *partials, int nblk, const void *dy, const void *x, const void *accumulate, void *dx, int M,
                          int C, int ps_dy, int ps_x, int ps_acc, int ps_dx, const float *scale, const float *shift, const float *mean,
                          const float *invstd, int relu, void *ws, float *dgamma, float *dbeta, sn_stream_t stream);
/* Moving-statistics BatchNorm (use_global_stats=True) inside a TRAINING graph (fix_bn): y = act(x*scale + shift) with constant
 * statistics, so dx = scale * g [+ accumulate] (g = dy where the activation passes), dbeta += sum g,
 * dgamma += sum g * (x - mean) / sqrt(var + eps).  One pass over dy and x produces dx and the per-row-block partial sums
 * (ws = sn_bn_workspace_bytes(M, C), fixed summation order, no atomics), a small finalize adds them into dgamma / dbeta.
 * dx == NULL: parameter gradients only; dgamma == dbeta == NULL: dx only (mean, var, ws unused).  scale / shift as
 * sn_bn_global_scale_shift wrote them; mean / var are read, never written. */
int sn_bn_frozen_backward(const void *dy, const void *x, const void *accumulate, void *dx, int M, int C, int ps_dy, int ps_x,
                          int ps_acc, int ps_dx, const float *scale, const float *shift, const float *mean, const float *var,
                          float eps, int relu, void *ws, float *dgamma, float *dbeta, sn_stream_t stream);
/* sn_bn_global_scale_shift for a table of layers in one launch; bit-equal results.  desc: n_desc records of 56 bytes on the
 * device, {const float *gamma (NULL = 1), *beta, *mean, *var; float *scale, *shift; int C; float eps}. */
int sn_bn_global_scale_shift_batch(const void *desc, int n_desc, sn_stream_t stream);

/* Depthwise 3x3 convolution (Convolution with num_group == channels; mobilenetv2_e2e.py:27-43,57-66), channels-last
 * fp16, weights [C][KH*KW] fp16.  dgrad adds `accumulate` (may be NULL / alias dx); wgrad accumulates (+=) into fp32
 * dw [C][KH*KW] through per-block partials in `ws` summed in block order (deterministic, no atomics). */
int sn_dwconv_fwd(const void *x, const void *w, void *y, int N, int H, int W, int C, int in_pix_stride, int out_pix_stride, int KH,
                  int KW, int stride, int pad, int dil, sn_stream_t stream);
int sn_dwconv_dgrad(const void *dy, const void *w, const void *accumulate, void *dx, int N, int H, int W, int C, int dy_pix_stride,
                    int acc_pix_stride, int dx_pix_stride, int KH, int KW, int stride, int pad, int dil, sn_stream_t stream);
size_t sn_dwconv_wgrad_workspace_bytes(int N, int H, int W, int C, int KH, int KW, int stride, int pad, int dil);
int sn_dwconv_wgrad(const void *dy, const void *x, float *dw, int N, int H, int W, int C, int dy_pix_stride, int x_pix_stride,
                    int KH, int KW, int stride, int pad, int dil, void *ws, size_t ws_bytes, sn_stream_t stream);
/* Grouped convolution (Convolution with 1 < num_group < channels; the ResNeXt 3x3 with num_group = 64), channels-last fp16
 * with pixel pitches, fp32 accumulation.  Weights are the compact [O][KH*KW][C/groups] fp16 layout for the forward pass AND the
 * data gradient (no transposed copy).  Cg == Og in {4, 8, 16, 32} with C % 32 == 0, a 1x1 or 3x3 kernel and stride 1 or 2 run on
 * the matrix cores; every other shape with C % groups == O % groups == 0 takes a plain kernel.  groups == 1 (sn_conv_*) and
 * groups == C == O (sn_dwconv_*) are argument errors.  fwd: bias fp32 [O] or NULL, optional ReLU; out_f32 writes fp32 with the
 * same pitch (plain kernel).  dgrad adds `accumulate` (may be NULL / alias dx).  wgrad accumulates (+=) into fp32
 * dw [O][KH*KW][C/groups] through per-block partials in `ws` summed in block order (deterministic, no atomics). */
int sn_gconv_fwd(const void *x, const void *w, const float *bias, void *y, int N, int H, int W, int C, int in_pix_stride, int O,
                 int out_pix_stride, int groups, int KH, int KW, int stride, int pad, int dil, int relu, int out_f32,
                 sn_stream_t stream);
int sn_gconv_dgrad(const void *dy, const void *w, const void *accumulate, void *dx, int N, int H, int W, int C, int O,
                   int dy_pix_stride, int acc_pix_stride, int dx_pix_stride, int groups, int KH, int KW, int stride, int pad, int dil,
                   sn_stream_t stream);
size_t sn_gconv_wgrad_workspace_bytes(int N, int H, int W, int C, int O, int groups, int KH, int KW, int stride, int pad, int dil);
int sn_gconv_wgrad(const void *dy, const void *x, float *dw, int N, int H, int W, int C, int O, int dy_pix_stride, int x_pix_stride,
                   int groups, int KH, int KW, int stride, int pad, int dil, void *ws, size_t ws_bytes, sn_stream_t stream);
/* Grouped deformable convolution (DeformableConvolution with num_group > 1; the ResNeXt stage-4 3x3 with num_group = 64,
 * num_deformable_group = 4), channels-last fp16 with pixel pitches, fp32 accumulation, compact [O][9][C/groups] fp16 weights.
 * The bilinear sample of sn_deform_im2col is taken in registers and fed to the matrix cores: no column buffer in the forward pass
 * or the weight gradient.  offset (N,Ho,Wo,>=2*9*deformable_groups) with its pixel pitch, offset_dtype 0 = fp16, 1 = fp32.
 * One path only -- C/groups == O/groups in {4, 8, 16, 32}, C % 32 == 0, (C / deformable_groups) % 32 == 0, a 3x3 kernel, square
 * stride >= 1 / pad / dilation; anything else (groups == 1 included) is an argument error naming the condition.
 * fwd: bias fp32 [O] or NULL, optional ReLU.  dcol (M, 9, C) fp16 = sum_o dy[m][o] * w[o][t][ci], the input of sn_deform_col2im
 * (which needs M * 9 * C < 2^31).  wgrad accumulates (+=) into fp32 dw [O][9][C/groups] through per-block partials in `ws` summed
 * in block order (deterministic, no atomics). */
int sn_gdeform_fwd(const void *x, const void *offset, const void *w, const float *bias, void *y, int N, int H, int W, int C,
                   int in_pix_stride, int O, int out_pix_stride, int groups, int deformable_groups, int KH, int KW, int stride, int pad,
                   int dil, int offset_pix_stride, int offset_dtype, int relu, sn_stream_t stream);
int sn_gdeform_dcol(const void *dy, const void *w, void *dcol, int N, int H, int W, int C, int O, int dy_pix_stride, int groups, int KH,
                    int KW, int stride, int pad, int dil, sn_stream_t stream);
size_t sn_gdeform_wgrad_workspace_bytes(int N, int H, int W, int C, int O, int groups, int KH, int KW, int stride, int pad, int dil);
int sn_gdeform_wgrad(const void *dy, const void *x, const void *offset, float *dw, int N, int H, int W, int C, int O,
                     int dy_pix_stride, int x_pix_stride, int groups, int deformable_groups, int KH, int KW, int stride, int pad,
                     int dil, int offset_pix_stride, int offset_dtype, void *ws, size_t ws_bytes, sn_stream_t stream);
/* clip(lo, hi) (mx.sym.clip; relu6) forward, or backward = (lo <= ref <= hi ? a : 0) [+ accumulate]. */
int sn_clip_f16(const void *a, const void *ref, const void *accumulate, void *y, long rows, int C, int ps_a, int ps_ref, int ps_acc,
                int ps_y, float lo, float hi, int backward, sn_stream_t stream);

/* fp16 channels-last element-wise: mode 0 relu(a), 1 a+b, 2 relu-backward (ref>0 ? a : 0) [+ b]. */
int sn_ew_f16(const void *a, const void *b, const void *ref, void *y, long rows, int C, int ps_a, int ps_b, int ps_ref, int ps_y,
              int mode, sn_stream_t stream);
/* fp32 element-wise: op 0 a-b, 1 a+b, 2 a*b, 3 a*scalar, 4 fill(scalar). */
int sn_ew_f32(const float *a, const float *b, float *out, long n, int op, float scalar, sn_stream_t stream);
/* Max pooling, channels-last fp16: x (N,H,W,C) -> y (N,Ho,Wo,C), Ho = (H + 2 pad - k) / stride + 1; C % 8 == 0 and the window
 * within the padded input (Ho > 0 && Wo > 0), else SN_ERR_ARG before any launch.  A window with no finite value yields -65504. */
int sn_maxpool_fwd(const void *x, void *y, int N, int H, int W, int C, int k, int stride, int pad, sn_stream_t stream);
/* Gradient of sn_maxpool_fwd, channels-last fp16: x (N,H,W,C) the pool's input, dy (N,Ho,Wo,C), dx (N,H,W,C).  The pooled output
 * is not an argument: the decision is re-derived from x.
 *  - Window order: a window is scanned row-major over its valid positions; padding is never a candidate.
 *  - Tie rule: the window's whole dy goes to the FIRST position in that order whose value equals the window maximum (torch's
 *    CPU rule): p wins w iff x[p] > every earlier valid element of w and x[p] >= every later one.  Unlike torch, a NaN never
 *    wins a window (sn_maxpool_fwd's fmaxf skips it too); a window of NaNs alone goes to its first valid position.
 *  - Arithmetic: dx[p] = fp16(sum of float(dy[w]) over the windows p wins (+ float(accumulate[p]))), summed in fp32, rounded once.
 *  - Ownership: a gather.  Every dx element is written exactly once by exactly one thread: no atomics, no zero fill before it,
 *    bitwise reproducible.  accumulate: NULL, or fp16 of dx's geometry, may alias dx.
 *  - Accepted: C % 8 == 0, 1 <= stride <= k <= 7, 0 <= pad <= k / 2 (torch's own limit), the window within the padded input;
 *    anything else, or a NULL dy / x / dx, is SN_ERR_ARG before any launch.  3x3 / stride 2 / pad 1 has a kernel of its own. */
int sn_maxpool_bwd(const void *dy, const void *x, const void *accumulate, void *dx, int N, int H, int W, int C, int k, int stride,
                   int pad, sn_stream_t stream);
/* Pooling(pool_type='avg', global_pool=True) over a channels-last fp16 tensor x (N, HW, C) -> y (N, C) fp32 (the R-FCN
 * vote over the position-sensitive bins, BASELINE config C4), and its gradient dx = dy / HW (fp16, overwritten). */
int sn_avgpool_global_fwd(const void *x, float *y, int N, int HW, int C, sn_stream_t stream);
int sn_avgpool_global_bwd(const float *dy, void *dx, int N, int HW, int C, sn_stream_t stream);
/* out[b][c][r] = in[b][r][c] with dtype conversion (NHWC <-> NCHW); batch <= 65535 and rows <= 65535 * 32 (grid limits). */
int sn_transpose_batched(const void *in, void *out, int batch, int rows, int cols, long in_batch_stride, long out_batch_stride,
                         int in_ld, int out_ld, int in_dtype, int out_dtype, sn_stream_t stream);
int sn_copy2d(const void *in, void *out, long rows, int cols, int in_ld, int out_ld, int in_dtype, int out_dtype,
              sn_stream_t stream);

/* SoftmaxOutput (:279-281,310-311): data viewed as (outer, K, inner) fp32. */
int sn_softmax_fwd(const float *x, float *p, long outer, int K, long inner, sn_stream_t stream);
int sn_softmax_output_bwd(const float *p, const float *label, float *grad, long outer, int K, long inner, float ignore_label,
                          int use_ignore, float grad_scale, int normalize_valid, int *ws, sn_stream_t stream);
/* weight * smooth_l1(pred - target) and the MakeLoss gradient (:317-319,330-334). */
int sn_smooth_l1_loss(const float *pred, const float *target, const float *weight, float *loss, float *dpred, long n, float sigma,
                      float grad_scale, sn_stream_t stream);

/* BoxAnnotatorOHEM (lib/operator_py/box_annotator_ohem.py:27-78; TRAIN.ENABLE_OHEM): per image keep the roi_per_img RoIs of largest
 * classification + box loss and ignore the rest.  cls_score (B,R,C), bbox_pred / bbox_targets / bbox_weights (B,R,box_dim),
 * labels (B,R): fp32, dense, device.  Outputs labels_ohem (B,R), bbox_weights_ohem (B,R,box_dim) and fg_labels (B,R) or NULL are
 * OVERWRITTEN (every element written exactly once: no fill before the call) and may not alias the inputs.  Per image:
 *   valid = label >= 0
 *   loss  = valid ? -log(softmax(score)[label] + 1e-14) + sum_j w_j * smooth_l1(pred_j - target_j, sigma = 1) : 0
 *           (fp32, max-subtracted log-sum-exp; a label >= C reads class C-1, nothing is read out of bounds)
 *   the roi_per_img RoIs of largest loss are kept: weights unchanged, label unchanged (a label < 0 is written as -1);
 *   every other RoI gets label -1 and weights 0.  fg_labels = labels_ohem with 0 replaced by -1.
 * Order, where numpy's argsort leaves it open: descending loss, equal losses by ascending RoI index; a NaN loss ranks above every
 * number (np.argsort puts NaN last, the reference reverses the order).
 * roi_per_img >= R keeps everything.  Refused before any launch: a NULL tensor other than fg_labels, B < 1, R < 1,
 * R > SN_OHEM_MAX_ROIS (the keys of one image are ranked in the 64 KB of LDS a workgroup gets without an opt-in), C < 2,
 * box_dim < 1, roi_per_img < 1.
 * One launch (one workgroup per image), no workspace, no atomics, no host read-back, the same bits every run.  No gradient. */
#define SN_OHEM_MAX_ROIS 16384
int sn_box_annotator_ohem(const float *cls_score, const float *bbox_pred, const float *labels, const float *bbox_targets,
                          const float *bbox_weights, float *labels_ohem, float *bbox_weights_ohem, float *fg_labels /* or NULL */,
                          int B, int R, int C, int box_dim, int roi_per_img, sn_stream_t stream);

/* COCO box evaluation (lib/dataset/pycocotools/cocoeval.py:163-272 evaluateImg, :312-365 accumulate; IoU = bbIou,
 * lib/dataset/pycocotools/maskApi.c:98-109).  float64 and integer counts throughout: `precision` and `recall` are the reference's
 * bits.  A PROBLEM is one (category, image) pair with at least one detection or one box; the P problems are stored category-major,
 * then by image.  All tensors are device pointers except h_max_dets.
 *   dt        (ND,6) f64   x, y, w, h, score, area, a problem's detections contiguous in arrival order;  dt_off (P+1) i32
 *   gt        (NG,5) f64   x, y, w, h, area;  gt_flags (NG) u8, bit 0 = iscrowd, bit 1 = ignore;           gt_off (P+1) i32
 *   kp_off    (P+1) i32    prefix sum of min(D_p, max_det): where a problem's KEPT detections sit in the NK-long outputs
 *   cat_off   (K+1) i32    the first problem of every category (cat_off[k] == cat_off[k+1]: the category is absent)
 *   iou_thrs (T) f64, area_rng (A,2) f64 (both bounds inclusive), rec_thrs (R) f64, h_max_dets (M) i32 in HOST memory.
 * sn_coco_match, one launch, per problem: ranks the detections by descending score (equal scores by arrival order), keeps the first
 * max_det, and runs the greedy matching of every (area range, threshold) over them:
 *   dt_rank   (NK) i32      arrival index of the r-th kept detection
 *   dt_match  (A,T,NK) i32  1 + arrival index (within the problem) of the matched box, 0 = unmatched
 *   dt_ignore (A,T,NK) u8   the matched box is ignored, or the detection is unmatched and its area lies outside the range
 *   gt_match  (A,T,NG) i32  1 + rank of the (last) detection that matched the box, 0 = unmatched
 *   gt_ignore (A,NG) u8     iscrowd | ignore | area < lo | area > hi
 * A detection qualifies for a box when IoU >= min(t, 1 - 1e-10); the best IoU wins, on equal IoU the LATER box; boxes that are not
 * ignored and not matched are searched first, ignored boxes only if none of those qualifies, and an ignored box that is already
 * matched is skipped unless it is a crowd.
 * sn_coco_accumulate, three launches: precision (T,R,K,A,M) f64 and recall (T,K,A,M) f64, every element written (-1 where the
 * category is absent or has no box that the area range keeps).  Detections of a category are ordered by (descending score, position
 * in the concatenation of the problems) -- what a stable mergesort of -score yields.  From the first recall threshold whose
 * searchsorted index is past the last detection onward, precision stays 0 (the reference's try/except).
 * max_dt_per_problem, max_gt_per_problem, max_kept_per_category: the largest D_p, G_p and per-category kept count, which the caller
 * knows from building the offsets; the first two are checked against the limits, the last sizes the ordering launch.
 * Refused before any launch, by a message that names the condition: a NULL tensor; P < 1; T, A, M or R below 1 or above
 * SN_COCO_MAX_T / _A / _M / _R; K above 65535; max_det < 1; max_dets not ascending or its last entry != max_det; a problem with more
 * than SN_COCO_MAX_DT detections (their scores are ranked in LDS) or SN_COCO_MAX_GT boxes (four per lane, in registers); row counts
 * past 32-bit indexing; a workspace shorter than sn_coco_accumulate_workspace_bytes(NK, T, A).  sn_coco_match needs no workspace
 * (sn_coco_match_workspace_bytes() = 0).  sn_coco_limits: h_out8 (HOST) = {MAX_DT, MAX_GT, MAX_T, MAX_A, MAX_M, MAX_R, detections per
 * workgroup of the ordering launch, detections per chunk of the scans}.
 * No atomics, no host read-back, the same bits every run. */
#define SN_COCO_MAX_DT 1024
#define SN_COCO_MAX_GT 256
#define SN_COCO_MAX_T 16
#define SN_COCO_MAX_A 8
#define SN_COCO_MAX_M 4
#define SN_COCO_MAX_R 128
int sn_coco_limits(int32_t *h_out8);
/* Detections as the test run holds them, rows (x1, y1, x2, y2, score) float64 (rows_f32 = 0) or float32 (1), -> dt rows
 * (x1, y1, x2 - x1 + 1, y2 - y1 + 1, score, w * h) float64 WITHOUT the rounding of the reference's result file; output row j reads
 * input row src[j] (src (n) i32, or NULL for row j). */
int sn_coco_pack_rows(const void *rows, int rows_f32, const int32_t *src, long n, double *dt6, sn_stream_t stream);
size_t sn_coco_match_workspace_bytes(void);
int sn_coco_match(const double *dt, const int32_t *dt_off, const int32_t *kp_off, const double *gt, const uint8_t *gt_flags,
                  const int32_t *gt_off, const double *iou_thrs, const double *area_rng, int P, int T, int A, int max_det,
                  int max_dt_per_problem, int max_gt_per_problem, long NK, long NG, int32_t *dt_rank, int32_t *dt_match,
                  uint8_t *dt_ignore, int32_t *gt_match, uint8_t *gt_ignore, sn_stream_t stream);
size_t sn_coco_accumulate_workspace_bytes(long NK, int T, int A);
int sn_coco_accumulate(const double *dt, const int32_t *dt_off, const int32_t *kp_off, const int32_t *gt_off, const int32_t *cat_off,
                       const int32_t *dt_rank, const int32_t *dt_match, const uint8_t *dt_ignore, const uint8_t *gt_ignore,
                       const double *rec_thrs, const int32_t *h_max_dets, int P, int K, int T, int A, int M, int R, int max_det,
                       int max_kept_per_category, long NK, long NG, void *ws, size_t ws_bytes, double *precision, double *recall,
                       sn_stream_t stream);

/* COCO mask evaluation (cocoeval.py with useSegm = 1; the arithmetic of lib/dataset/pycocotools/maskApi.c: rleArea :72-75, rleToBbox
 * :111-124, rleIou :77-96 behind the bbIou gate of :98-109).  Integer counts and one float64 division per IoU: the matrices are the
 * reference's bits.  A MASK is a run of u32 counts in column-major order, zeros first (the first count may be 0); the N masks of a call
 * lie in one pool behind (N+1) i32 prefix offsets, with their sizes in hw (N,2) i32 = h, w.  All tensors are device pointers except
 * h_out5.  PRECONDITIONS, not checked on the device: every h and w is >= 1; the counts of a mask sum to h * w; only the first count of a
 * mask is 0 (what rleEncode, rleFrPoly and rleMerge produce; the reference's own walk stops early where two masks have an empty run at
 * the same position); the masks of a problem share their image's size (the caller compares them on the host); scores are finite.
 * sn_rle_stats, one launch, a wave per mask:
 *   rows6  (N,6) f64      x, y, w, h of rleToBbox (run END POINTS only, t = cc - j % 2, an odd last count dropped, an empty mask gives
 *                         four zeros), score[n] (0 where score is NULL), rleArea -- the rows sn_coco_match_iou and sn_coco_accumulate read
 *   cum2   (total,2) u32  per run: its end position and the 1-pixels up to and including it (what sn_rle_iou searches)
 *   total_runs = rle_off[N], max_hw = the largest h * w: known to the caller from building the pool, checked against 32-bit indexing.
 * sn_rle_iou, one launch, a wave per pair: iou (n_pairs) f64, problem p's D_p x G_p matrix at iou_off[p] (iou_off (P+1) i32,
 *   iou_off[p+1] - iou_off[p] = D_p * G_p), detection-major in arrival order.  An entry is 0 unless the two rleToBbox boxes overlap with
 *   positive width and height (bbIou > 0: NOT an optimisation -- a run that wraps into the next column makes rleToBbox understate the
 *   y-extent, and two masks that intersect can score 0); otherwise i / u with i the common 1-pixels and u = area_d + area_g - i, or
 *   u = area_d for a crowd (gt_flags bit 0); i = 0 gives 0.  The problems of a call may be a slice of a longer list: row r of dt_off /
 *   gt_off names mask r - dt_off[0] / r - gt_off[0] of the pools, rows and flags passed with it.
 * sn_coco_match_iou: sn_coco_match with the IoU of (detection d, box g) of problem p read from iou[iou_off[p] + d * G_p + g] instead of
 *   computed from boxes; gt_area (NG) f64 replaces the box rows; outputs, tie rules and limits are those of sn_coco_match, and
 *   sn_coco_accumulate takes them as they are.  Offsets are absolute row numbers of dt / gt_area / gt_flags and the outputs.
 * Refused before any launch, by a message that names the function and the condition: a NULL tensor; N or P below 1; h * w, the runs or
 * the pairs of a call past 32-bit indexing; T or A outside SN_COCO_MAX_T / _A; max_det < 1; a problem with more than SN_COCO_MAX_DT
 * detections or SN_COCO_MAX_GT masks of ground truth; A * T * NK or A * T * NG past 32 bits.  No workspace is needed.
 * sn_rle_limits: h_out5 (HOST) = {MAX_DT, MAX_GT, runs per scan step of sn_rle_stats and 1-runs per search step of sn_rle_iou (a wave),
 * masks / pairs per workgroup, threads per workgroup}; the last is also the workgroup of the polygon and paste kernels of mask_rle.hip:
 * boundary points, crossings and box columns per round of their block scans.  No atomics, no host read-back, the same bits every run. */
int sn_rle_limits(int32_t *h_out5);
/* The paste of mask probabilities into the image (mask_voc2coco, lib/mask/mask_voc2coco.py:39-49): detection i has an (M, M) f32 mask
 * and an i32 box x1, y1, x2, y2 (boxes (n,4): clipped to its image and rounded ON THE HOST, numpy float64, so that 0 <= x1 <= x2 < w and
 * 0 <= y1 <= y2 < h -- PRECONDITION, not checked on the device); hw (n,2) i32 its image's h, w; col_off (n+1) i32 the prefix of the box
 * widths x2 - x1 + 1.  The mask is resized to the box, compared >= binary_thresh (float32), zeros outside the box, and the whole image
 * is run-length encoded column-major (what rleEncode gives for that bitmap).  THE RESIZE IS SPECIFIED BY THIS PROJECT AND NOT PINNED TO
 * OPENCV: the float32 INTER_LINEAR path of the algorithm oracle/cv_resize.py documents for uint8 -- per axis scale = 1 / (b / M) in
 * double, coefficient f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s; x clamps at both ends (s < 0: s = 0, f = 0;
 * s >= M - 1: the value is S[M - 1]); y clips its two source rows to [0, M - 1] and keeps the coefficient; horizontal pass S[s] * (1 - f)
 * + S[s + 1] * f, then the vertical pass, in float32 without fused multiply-add; when both scales are exactly 2 the value is the area
 * average (((a + b) + c) + d) * 0.25f of the 2 x 2 block.
 * sn_rle_paste_count, one launch, a workgroup per detection: col_pre (total_cols) i32 = value changes before each box column, det_t
 *   (n) i32 = value changes per detection.  The caller reads det_t back -- the one read-back of this stage -- and builds rle_off (n+1)
 *   i32 with det_t[i] + 1 counts per detection.  sn_rle_paste, one launch: tpos (total_runs) u32 workspace, cnts (total_runs) u32.
 * Refused before any launch: a NULL tensor; n < 1; M outside [1, 1024] or n * M * M past 31 bits; columns or runs past 32-bit
 * indexing; h * w outside [1, 2^31). */
int sn_rle_paste_count(const float *masks, const int32_t *boxes, const int32_t *hw, const int32_t *col_off, int n, int M,
                       float binary_thresh, long total_cols, long max_hw, int32_t *col_pre, int32_t *det_t, sn_stream_t stream);
int sn_rle_paste(const float *masks, const int32_t *boxes, const int32_t *hw, const int32_t *col_off, const int32_t *col_pre,
                 const int32_t *rle_off, int n, int M, float binary_thresh, long total_cols, long total_runs, long max_hw,
                 uint32_t *tpos, uint32_t *cnts, sn_stream_t stream);
/* Polygons to masks: rleFrPoly (maskApi.c:139-179) per polygon, then the union of an annotation's parts (rleMerge, intersect = 0), on the
 * reference's counts.  xy (total_vertices,2) f64; poly_off (NP+1) i32 over vertices; poly_hw (NP,2) i32 = h, w of the polygon's image
 * (the parts of an annotation share it); ann_off (NA+1) i32 over polygons.  edge_pt_off (total_vertices+1) i32: prefix of the edges'
 * boundary-point counts max(|dx|, |dy|) + 1 of the 5x upsampled integer vertices (int)(5 * x + .5), edge e of a polygon running from its
 * vertex e to the next (the last back to the first); the caller builds it from the same float64 arithmetic, because it sizes the walk.
 * sn_rle_poly_cross, one launch, a workgroup per polygon: the boundary walk in closed form per point, float64 with the C casts that
 *   truncate toward zero, the x-change filter floor(xd) != xd || xd < 0 || xd > w - 1, the yd clamp to [0, h] and ceil.  With
 *   cross_off = NULL it counts: cross_count (NP) i32 = the kept points x * h + y below h * w (a point AT h * w shares the end with the
 *   reference's sentinel and never ends a run).  The caller reads the counts back -- the one read-back of this stage --, builds
 *   cross_off (NP+1) i32 and calls again: cross (total_cross) u32 in boundary order.  A zero-length edge (a repeated or an explicit
 *   closing vertex) has s = 0 / 0 in the reference, whose v is never read; it is not formed here.
 * sn_rle_from_polys, two launches: per polygon the distinct positions of odd multiplicity in ascending order -- what the reference's
 *   sort and sequential compaction leave: odd toggles, even cancels -- found by counting, without a sort (no LDS path, no size at which
 *   another path takes over; quadratic in the crossings of one polygon), written as counts; then per annotation a copy (one part) or
 *   the canonical RLE of the OR of the parts.  Pools with slack: polygon p's counts at part_runs[cross_off[p] + p ..), part_m[p] of
 *   them (at most its crossings + 1); annotation a's at runs[cross_off[q] + q ..) with q = ann_off[a], ann_m[a] of them.
 * There is no cap on vertices, boundary points or crossings beyond 32-bit indexing.  PRECONDITIONS, not checked on the device: finite
 * vertices with |5 * x + .5| below 2^31; every annotation has at least one polygon.  Refused before any launch: a NULL tensor; NP or NA
 * below 1; totals past 32-bit indexing; h * w outside [1, 2^31); a workspace shorter than sn_rle_from_polys_workspace_bytes(total_cross)
 * (0 for a refused total). */
int sn_rle_poly_cross(const double *xy, const int32_t *poly_off, const int32_t *edge_pt_off, const int32_t *poly_hw,
                      const int32_t *cross_off /* or NULL */, int NP, long total_vertices, long total_points, long max_hw,
                      int32_t *cross_count, uint32_t *cross, sn_stream_t stream);
size_t sn_rle_from_polys_workspace_bytes(long total_cross);
int sn_rle_from_polys(const uint32_t *cross, const int32_t *cross_off, const int32_t *poly_hw, const int32_t *ann_off, int NP, int NA,
                      long total_cross, void *ws, size_t ws_bytes, uint32_t *part_runs, int32_t *part_m, uint32_t *runs, int32_t *ann_m,
                      sn_stream_t stream);
int sn_rle_stats(const uint32_t *cnts, const int32_t *rle_off, const int32_t *hw, const double *score /* or NULL */, long N,
                 long total_runs, long max_hw, double *rows6, uint32_t *cum2, sn_stream_t stream);
int sn_rle_iou(const uint32_t *dt_cum2, const int32_t *dt_rle_off, const double *dt_rows6, const uint32_t *gt_cum2,
               const int32_t *gt_rle_off, const double *gt_rows6, const uint8_t *gt_flags, const int32_t *dt_off, const int32_t *gt_off,
               const int32_t *iou_off, int P, long n_pairs, double *iou, sn_stream_t stream);
int sn_coco_match_iou(const double *dt, const int32_t *dt_off, const int32_t *kp_off, const double *gt_area, const uint8_t *gt_flags,
                      const int32_t *gt_off, const double *iou, const int32_t *iou_off, const double *iou_thrs, const double *area_rng,
                      int P, int T, int A, int max_det, int max_dt_per_problem, int max_gt_per_problem, long NK, long NG,
                      int32_t *dt_rank, int32_t *dt_match, uint8_t *dt_ignore, int32_t *gt_match, uint8_t *gt_ignore,
                      sn_stream_t stream);

/* Compressed string counts: rleToString / rleFrString (maskApi.c:181-208), the `counts` of a results file.  Six bits per character
 * from chr(48): five of payload, 0x20 = another character of this count follows, 0x10 of a count's last character = its sign; from
 * the fourth count on the value coded is the difference to the count two before.  Integer arithmetic, exact bytes.
 * Masks are pooled as everywhere here: cnts (total_runs) u32 behind run_off (N+1) i32, characters (total_chars) u8 behind str_off
 * (N+1) i32, no terminator stored.  Each direction is two calls with a host scan between them: lengths, then the fill at the offsets
 * the caller built from them.  The offsets are given TWICE, on the device (what the kernels read) and as the HOST array they were
 * uploaded from (h_*, what the entry point checks before it launches).  One workgroup of one wave per mask, chunks of 64 counts /
 * characters with a carry; plain vector stores, no atomics, no workspace, one fixed order.
 * Encoding, count i of a mask: x = cnts[i] - (i > 2 ? cnts[i-2] : 0) in int64 takes the smallest k >= 1 with -2^(5k-1) <= x < 2^(5k-1)
 *   characters; character j is (((x >> 5j) & 0x1f) | (j < k-1 ? 0x20 : 0)) + 48.  k <= 7 for every pair of uint32 counts (the
 *   reference allocates six per count and is undefined where |x| >= 2^29).
 *   sn_rle_string_len: str_len (N) i32 = the bytes of every mask's string.  sn_rle_to_string: chars, mask n at str_off[n]; nothing is
 *   written outside [str_off[n], str_off[n+1]).
 * Decoding, modulo 2^32: payloads OR-ed at 5j, sign extension where the last character carries 0x10, then cnts[i] = x_i + cnts[i-2]
 *   for i > 2 -- two interleaved prefix sums, scanned.
 *   sn_rle_string_count: m (N) i32 = the counts of every string (its characters without 0x20), status (N) i32 = 0 ok | 1 the string
 *   ends inside a count | 2 a character outside chr(48) .. chr(111) | 3 a count of more than 7 characters; where several hold, 2
 *   comes before 1 before 3 (a foreign character makes the other bits meaningless).  sn_rle_from_string: cnts, string n at
 *   run_off[n]; a string whose status is not 0 writes nothing, and nothing is written outside [run_off[n], run_off[n+1]).
 * sn_rle_string_limits: h_out3 (HOST) = {threads per workgroup, counts / characters per chunk, the most characters of a count (7)}.
 * Refused before any launch: NULL operands; N < 1; offsets that do not start at 0, that decrease, or that do not end at the total
 * given; totals past 32-bit indexing. */
int sn_rle_string_limits(int32_t *h_out3);
int sn_rle_string_len(const uint32_t *cnts, const int32_t *run_off, const int32_t *h_run_off, long N, long total_runs, int32_t *str_len,
                      sn_stream_t stream);
int sn_rle_to_string(const uint32_t *cnts, const int32_t *run_off, const int32_t *h_run_off, const int32_t *str_off,
                     const int32_t *h_str_off, long N, long total_runs, long total_chars, uint8_t *chars, sn_stream_t stream);
int sn_rle_string_count(const uint8_t *chars, const int32_t *str_off, const int32_t *h_str_off, long N, long total_chars, int32_t *m,
                        int32_t *status, sn_stream_t stream);
int sn_rle_from_string(const uint8_t *chars, const int32_t *str_off, const int32_t *h_str_off, const int32_t *run_off,
                       const int32_t *h_run_off, const int32_t *status, long N, long total_chars, long total_runs, uint32_t *cnts,
                       sn_stream_t stream);

/* PASCAL VOC box evaluation (lib/dataset/pascal_voc_eval.py:116-181 voc_eval, :39-70 voc_ap).  float64 and integer counts
 * throughout: `rec`, `prec` and `ap07` are the reference's bits, `ap_area` is its sum in another order (each term >= 0, every partial
 * sum <= 1: within (n - 1) * 2^-53 of the exact sum for n recall changes).  A PROBLEM is one (class, image) pair with at least one
 * detection or one box; the P problems are stored class-major, then by image.  All tensors are device pointers except h_ap07_thrs.
 *   dt_box    (ND,4) f64   x1, y1, x2, y2 as the result file holds them (1-based), a problem's detections contiguous in arrival
 *                          order;  dt_score (ND) f64;  dt_off (P+1) i32
 *   gt_box    (NG,4) f64   x1, y1, x2, y2 as the annotation holds them;  gt_difficult (NG) u8;  gt_off (P+1) i32
 *   cat_off   (K+1) i32    the first problem of every class (cat_off[k] == cat_off[k+1]: the class has neither detections nor boxes)
 *   iou_thrs  (T) f64;  h_ap07_thrs (11) f64 in HOST memory: the values of np.arange(0., 1.1, 0.1).
 * PRECONDITIONS, not checked on the device: every row is finite with x2 >= x1 and y2 >= y1 (so that no union is 0), scores are
 * finite.
 * sn_voc_match, one launch, per problem.  IoU = iw * ih / ((area_d + area_g) - iw * ih) with iw = max(min(x2) - max(x1) + 1, 0) and
 * areas (x2 - x1 + 1) * (y2 - y1 + 1).  Per detection: ovmax and the FIRST box of maximal IoU (on equal IoU the EARLIER box,
 * np.argmax; the opposite of sn_coco_match); a problem without boxes gives ovmax = -inf.  The detections of a problem are ranked by
 * descending score, EQUAL SCORES BY ARRIVAL ORDER (the reference's np.argsort(-confidence) is not stable and leaves their order
 * undefined; this library defines it).  For every threshold t: ovmax > t (strict) and the box is difficult: neither tp nor fp;
 * ovmax > t, the box is not difficult and the detection is the first in rank among those claiming that box: tp, later claimants fp;
 * ovmax <= t: fp.  A detection never falls back to a second-best box.
 *   dt_best   (ND) i32      1 + arrival index (within the problem) of the argmax box, 0 = none
 *   dt_iou    (ND) f64      ovmax
 *   dt_tp, dt_fp (T,ND) u8
 *   gt_det    (T,NG) i32    1 + arrival index (within the problem) of the detection that took the box, 0 = none (always 0 for a
 *                           difficult box)
 * sn_voc_accumulate, two launches.  The detections of a class are ordered by (descending score, position in the concatenation of
 * the class's problems) -- what a stable sort of -score yields.  Per (t, class): inclusive integer scans of tp and fp,
 * rec = tp / (double)npos, prec = tp / max(tp + fp, 2^-52); ap07 = eleven sequential `ap += p / 11.` with p = the max of prec where
 * rec >= h_ap07_thrs[j], else 0; ap_area = the sum of (mrec[i+1] - mrec[i]) * mpre[i+1] over the recall changes, with the sentinels
 * and the reverse running max of voc_ap.  A class with detections and npos = 0 has rec = nan, ap07 = 0 and ap_area = nan, as the
 * reference; a class without detections has both APs 0.
 *   order     (ND) i32      order[c0 + r] = position in the detection list of the class's r-th detection (c0 = the class's first row)
 *   rec, prec (T,ND) f64    the curves, in sorted order
 *   npos      (K) i32       non-difficult boxes per class
 *   ap07, ap_area (T,K) f64
 * Every element of every output is written on every call.  max_dt_per_problem, max_gt_per_problem, max_dt_per_class: the largest
 * D_p, G_p and per-class detection count, which the caller knows from building the offsets; the first two are checked against the
 * limits, the last sizes the ordering launch.
 * Refused before any launch, by a message that names the function and the condition: a NULL tensor; P < 1; T below 1 or above
 * SN_VOC_MAX_T; K above 65535; a problem with more than SN_VOC_MAX_DT detections or SN_VOC_MAX_GT boxes (both live in LDS); row
 * counts past 32-bit indexing; a workspace shorter than sn_voc_accumulate_workspace_bytes(ND, T) (0 for a refused shape).
 * sn_voc_limits: h_out5 (HOST) = {MAX_DT, MAX_GT, MAX_T, detections per workgroup of the ordering launch, detections per chunk of
 * the scans}.  No float atomics (one integer min in LDS), no host read-back, the same bits every run. */
#define SN_VOC_MAX_DT 1024
#define SN_VOC_MAX_GT 256
#define SN_VOC_MAX_T 8
int sn_voc_limits(int32_t *h_out5);
int sn_voc_match(const double *dt_box, const double *dt_score, const int32_t *dt_off, const double *gt_box,
                 const uint8_t *gt_difficult, const int32_t *gt_off, const double *iou_thrs, int P, int T, int max_dt_per_problem,
                 int max_gt_per_problem, long ND, long NG, int32_t *dt_best, double *dt_iou, uint8_t *dt_tp, uint8_t *dt_fp,
                 int32_t *gt_det, sn_stream_t stream);
size_t sn_voc_accumulate_workspace_bytes(long ND, int T);
int sn_voc_accumulate(const double *dt_score, const int32_t *dt_off, const int32_t *gt_off, const int32_t *cat_off,
                      const uint8_t *gt_difficult, const uint8_t *dt_tp, const uint8_t *dt_fp, const double *h_ap07_thrs, int P, int K,
                      int T, int max_dt_per_class, long ND, long NG, void *ws, size_t ws_bytes, int32_t *order, double *rec,
                      double *prec, int32_t *npos, double *ap07, double *ap_area, sn_stream_t stream);

/* PASCAL VOC mask evaluation (lib/dataset/pascal_voc_eval.py:184-272 voc_eval_sds; lib/mask/mask_transform.py:40-70 mask_overlap):
 * the mask AP of the FCIS / DCN lineage (mAP^r).  Integer counts and one float64 division per overlap: the matrix, tp and fp are the
 * reference's, and sn_voc_accumulate -- AS IT IS, called with an all-zero gt_difficult, so that npos is the reference's num_pos --
 * gives rec, prec and ap07 (the number voc_eval_sds returns) on its bits and ap_area beside them.  (The entry points are named
 * sn_vocsds_* and not sn_voc_*: the box evaluation's tests own that prefix.)  A PROBLEM is one (class, image) pair with at least one
 * detection or one instance, class-major then by image: the layout of sn_voc_match.  All tensors are device pointers except h_out6.
 *   masks      (ND,M,M) f32  probability maps, a problem's detections contiguous in arrival order
 *   dt_box     (ND,4) i32    x1, y1, x2, y2 = np.round(box).astype(int), done ON THE HOST in float64.  A box may lie partly or wholly
 *                            at negative coordinates: nothing here knows an image size, as in the reference.
 *   dt_off     (P+1) i32
 *   gt_bits    (pool) u8     the instances' cropped bitmaps, one byte per pixel (0 / non-zero), row-major, (y2 - y1 + 1) x
 *                            (x2 - x1 + 1) of the instance's bound, instance r's at [gt_pix_off[r], gt_pix_off[r+1])
 *   gt_pix_off (NG+1) i64;  gt_bound (NG,4) i32 x1, y1, x2, y2 (np.round(mask_bound).astype(int));  gt_off (P+1) i32
 *   gt_area    (NG) i32      the bitmap's number of set pixels (the host counts it once)
 *   iou_off    (P+1) i32     as for sn_rle_iou: iou_off[p+1] - iou_off[p] = D_p * G_p
 * PRECONDITIONS, checked on the host and not on the device: x2 >= x1 and y2 >= y1 for every box and bound (a violated one yields
 * counts of 0, never an access out of bounds); coordinates below 2^30 in magnitude; the offsets are consistent prefix sums; scores
 * are finite.  An instance whose bitmap length is not its bound's area is never read and has overlap 0.
 * sn_vocsds_mask_iou, one launch, a workgroup per detection:
 *   dt_area (ND) i32       the pixels >= binary_thresh of the map resized to its box
 *   iou     (n_pairs) f64  detection-major in arrival order; for instance g of the detection's problem: 0 if the intersection
 *                          rectangle of the two integer boxes is empty; else inter = the pixels set in both inside it, union =
 *                          dt_area + gt_area - inter, 0 if union < 1, else (double)inter / (double)union.
 *   THE RESIZE AND THE THRESHOLD ARE THE PASTE'S -- the float32 path documented at sn_rle_paste above, the exact-2x area average
 *   included, compared >= binary_thresh in float32 -- SPECIFIED BY THIS PROJECT AND NOT PINNED TO OPENCV (the reference calls
 *   cv2.resize); one copy of that arithmetic serves both (csrc/paste_bit.h).  Everything else here is pinned to the reference.
 * sn_vocsds_match_iou, one launch, a workgroup per problem.  Per detection cur = -1000.0 and the FIRST instance with ov > cur in
 *   ascending arrival order is its candidate: an instance of overlap 0 is a candidate, a problem without instances has none.
 *   Detections are ranked by descending score, EQUAL SCORES BY ARRIVAL ORDER (this library's rule, as sn_voc_match).  For every
 *   threshold t: cur >= t (NOT strict, unlike sn_voc_match) and the detection is the first in rank among those claiming that
 *   instance: tp; later claimants (already_detect): fp; cur < t or no candidate: fp.  There is no difficult flag.
 *   dt_best (ND) i32 1 + arrival index of the candidate, 0 = none;  dt_iou (ND) f64 cur (-1000 without a candidate);
 *   dt_tp, dt_fp (T,ND) u8;  gt_det (T,NG) i32 1 + arrival index of the detection that took the instance, 0 = none.
 * Every element of every output is written on every call; no float atomics (integer adds and one integer min in LDS), no host
 * read-back, the same bits every run.  max_box_pixels = the largest bw * bh, n_pairs = iou_off[P], max_*_per_problem: known to the
 * caller from building the tables, checked against the limits.
 * Refused before any launch, by a message that names the function and the condition: a NULL tensor; P < 1; for the overlaps ND < 1
 * or M < 1; M above SN_VOCSDS_MAX_M (the map is staged in LDS); T outside [1, SN_VOC_MAX_T]; a problem with more than
 * SN_VOC_MAX_DT detections or SN_VOC_MAX_GT instances; bw * bh, ND, NG or the pairs of a call at or above 2^31; T * ND or T * NG
 * past 32 bits.  No workspace is needed.
 * sn_vocsds_limits: h_out6 (HOST) = {MAX_DT, MAX_GT, MAX_T, MAX_M, threads per workgroup = box columns per round of
 * sn_vocsds_mask_iou, the largest bw * bh (2^31 - 1)}. */
#define SN_VOCSDS_MAX_M 64
int sn_vocsds_limits(int32_t *h_out6);
int sn_vocsds_mask_iou(const float *masks, const int32_t *dt_box, const int32_t *dt_off, const uint8_t *gt_bits,
                       const int64_t *gt_pix_off, const int32_t *gt_bound, const int32_t *gt_area, const int32_t *gt_off,
                       const int32_t *iou_off, int P, int M, float binary_thresh, int max_gt_per_problem, long ND, long NG,
                       long n_pairs, long max_box_pixels, int32_t *dt_area, double *iou, sn_stream_t stream);
int sn_vocsds_match_iou(const double *dt_score, const int32_t *dt_off, const int32_t *gt_off, const double *iou,
                        const int32_t *iou_off, const double *iou_thrs, int P, int T, int max_dt_per_problem,
                        int max_gt_per_problem, long ND, long NG, int32_t *dt_best, double *dt_iou, uint8_t *dt_tp, uint8_t *dt_fp,
                        int32_t *gt_det, sn_stream_t stream);

/* Proposal roidb (lib/dataset/imdb.py:81-204, 291-419): what turns an RPN proposals pickle into the roidb of the negative-chip run.
 * Ragged batches of I images through (I+1) i32 prefix offsets; all tensors are device pointers except h_out6.  PRECONDITIONS, not
 * checked on the device: rows are finite with x2 >= x1 and y2 >= y1 (so that no union is 0).
 * sn_prop_nms -- nmsp, lib/nms/nms.py:48-86 (called from imdb.py:102-112 load_rpn_data).  rows (total,5) f32 x1, y1, x2, y2, score,
 *   unsorted, image b's at [off[b], off[b+1]).  Per image: order by descending score, EQUAL SCORES THE LATER ROW FIRST (the
 *   reference's argsort()[::-1] on an unstable sort leaves their order undefined; this is what a reversed stable argsort gives), walk
 *   the order and suppress a row whose IoU with an earlier kept row is > thresh.  float32 throughout with the + 1 convention,
 *   inter / (area_i + area_j - inter).  Three launches.
 *     keep   (total) i32   at off[b]: the image's kept row indices (inside the image) in keep order, then -1
 *     nkeep  (I) i32
 *   max_n: the largest image.  ws: sn_prop_nms_workspace_bytes(total) (0 for a refused total).
 * sn_prop_assign -- create_roidb_from_box_list, imdb.py:168-191.  boxes (total,4) f64, gt_box (NG,4) f64, gt_classes (NG) i32.
 *   bbox_overlaps_cython (lib/bbox/bbox.pyx:35-56) in float64, iw * ih / ((bw * bh) + box_area - iw * ih), 0 when iw <= 0 or ih <= 0;
 *   per box the row maximum and the FIRST index that attains it (np.argmax).  One launch.
 *     max_ov  (total) f32  the maximum cast to float32 (0 in an image without ground truth)
 *     max_cls (total) i32  gt_classes[argmax] when the maximum is > 0, else 0
 *     argmax  (total) i32  index inside the image's ground truth, -1 in an image without
 * sn_prop_recall -- the matching of evaluate_recall, imdb.py:329-374.  One problem = one (image, area range) pair.  gt_mask (NG) u8:
 *   bit a set = the row belongs to range a (the host decides membership in the arrays' own dtype); thrs (T) f64.  Per problem with
 *   N > 0 boxes and G_a rows of the range: min(N, G_a) rounds, each takes the largest remaining overlap among unused boxes and unused
 *   rows, ties by LOWEST ROW then LOWEST BOX (the argmax(axis=0) / max(axis=0).argmax() pair), records it and retires both.  One
 *   launch (and two memsets of the counters).
 *     gt_ov   (A,NG) f64   at [a][gt_off[i] ..): the image's recorded values in round order, then zeros up to its G rows; the
 *                          first G_a slots are the reference's _gt_overlaps (an image with N = 0 contributes none)
 *     num_pos (A) i32      rows per range, images with N = 0 included
 *     hits    (A,T) i32    the number of the G_a slots (the zeros of unplayed rounds included, as in the reference) >= thrs[t],
 *                          over the images with N > 0; integer atomics: the same bytes every run
 * max_g: the largest G of an image, refused above SN_PROP_MAX_GT (the boxes of an image live in LDS / registers); N has no cap.
 * Refused before any launch, by a message that names the function and the condition: a NULL tensor; I < 1 (sn_prop_nms: I above
 * 65535); A outside 1 .. 8; T outside 1 .. SN_PROP_MAX_T; max_g above the limit; max_n above total; row counts past 32-bit
 * indexing; a short workspace.
 * sn_prop_limits: h_out6 (HOST) = {MAX_GT, MAX_T, boxes per workgroup of the assign launch, threads (= columns per pass) of the
 * recall workgroup, candidates per step of the NMS walk, rows per workgroup of the ordering launch}. */
#define SN_PROP_MAX_GT 512
#define SN_PROP_MAX_T 32
int sn_prop_limits(int32_t *h_out6);
size_t sn_prop_nms_workspace_bytes(long total);
int sn_prop_nms(const float *rows, const int32_t *off, int I, int max_n, long total, float thresh, void *ws, size_t ws_bytes,
                int32_t *keep, int32_t *nkeep, sn_stream_t stream);
int sn_prop_assign(const double *boxes, const int32_t *box_off, const double *gt_box, const int32_t *gt_classes,
                   const int32_t *gt_off, int I, int max_n, int max_g, long total, long NG, float *max_ov, int32_t *max_cls,
                   int32_t *argmax, sn_stream_t stream);
int sn_prop_recall(const double *boxes, const int32_t *box_off, const double *gt_box, const uint8_t *gt_mask, const int32_t *gt_off,
                   const double *thrs, int I, int A, int T, int max_g, long total, long NG, double *gt_ov, int32_t *num_pos,
                   int32_t *hits, sn_stream_t stream);

/* MultiProposal (:347-355) / MultiProposalTarget (:283-284).  cls_prob (B,2,A*Fh,Fw), bbox_pred (B,4A,Fh,Fw),
 * im_info (B,3), gt_boxes (B,G,5), valid_ranges (B,2), base_anchors (A,4): all fp32 device. */
size_t sn_proposal_workspace_bytes(int B, int A, int Fh, int Fw, int pre_nms_top_n, int post_nms_top_n);
int sn_multi_proposal(const float *cls_prob, const float *bbox_pred, const float *im_info, const float *base_anchors, int B, int A,
                      int Fh, int Fw, int feat_stride, int pre_nms_top_n, int post_nms_top_n, float nms_thresh, float min_size, void *ws,
                      float *rois, float *scores, sn_stream_t stream);
int sn_multi_proposal_target(const float *cls_prob, const float *bbox_pred, const float *im_info, const float *gt_boxes,
                             const float *valid_ranges, const float *base_anchors, int B, int A, int Fh, int Fw, int feat_stride, int G,
                             int pre_nms_top_n, int post_nms_top_n, float nms_thresh, float min_size, float fg_thresh,
                             const float *bbox_stds4, void *ws, float *rois, float *label, float *bbox_target,
                             float *bbox_weight, sn_stream_t stream);

/* Mask branch (symbols/faster/resnet_mx_101_e2e_mask.py:317-318,374-405; fork operators, semantics = DESIGN.md / oracle/nn.py).
 * sn_multi_proposal_target_mask: sn_multi_proposal_target plus, per chip, the first num_mask_rois foreground RoIs
 *   (mask_rois (B*num_mask_rois, 5), padded with [b,0,0,0,0]) and the gt_boxes row each matched (mask_ids, -1 = padding);
 *   match_ws = B * post_nms_top_n floats of scratch.
 * sn_mask_rcnn_target: the matched object's polygons (mask_polys (B, max_gts, max_len), rows as lib/data_utils/mask_utils.py
 *   :22-46 encodes them) rasterised into each RoI's mask_size^2 grid -> targets (N, ms, ms) in {1, 0, -1 = ignore}, cls (N).
 * sn_depth_to_space2 / sn_space_to_depth2: (N,H,W,4C) <-> (N,2H,2W,C) fp16, channel (a*2+b)*C + c <-> pixel (2h+a, 2w+b): the
 *   2x2 / stride-2 Deconvolution is a 1x1 convolution to 4C channels followed by this shuffle (relu fused on the way out).
 * sn_pick_fwd / sn_pick_bwd: pick(axis=1, keepdims) on a channels-last fp16 tensor (N, HW, C) with one index per n. */
int sn_multi_proposal_target_mask(const float *cls_prob, const float *bbox_pred, const float *im_info, const float *gt_boxes,
                                  const float *valid_ranges, const float *base_anchors, int B, int A, int Fh, int Fw, int feat_stride,
                                  int G, int pre_nms_top_n, int post_nms_top_n, float nms_thresh, float min_size, float fg_thresh,
                                  const float *bbox_stds4, void *ws, float *match_ws, int num_mask_rois, float *rois, float *label,
                                  float *bbox_target, float *bbox_weight, float *mask_rois, float *mask_ids, sn_stream_t stream);
int sn_mask_rcnn_target(const float *rois, const float *mask_polys, const float *mask_ids, int N, int rois_per_image, int max_gts,
                        int max_len, int mask_size, float *targets, float *cls, sn_stream_t stream);
int sn_depth_to_space2(const void *in, void *out, int N, int H, int W, int C, int relu, sn_stream_t stream);
int sn_space_to_depth2(const void *in, void *out, int N, int H, int W, int C, sn_stream_t stream);
int sn_pick_fwd(const void *x, const float *index, void *y, int N, int HW, int C, sn_stream_t stream);
int sn_pick_bwd(const void *dy, const float *index, void *dx, int N, int HW, int C, int accumulate, sn_stream_t stream);

/* Mask head at test time (semantics ours, like the rest of the mask branch): the foreground probability of
 * every RoI's OWN class from the output of mask_deconv_relu, in one launch -- mask_out's 1x1 convolution restricted to the two maps
 * the class reads, the two picks, the concatenation and the 2-way softmax of the stock chain.
 *   x (N, HW, C) fp16 channels-last; w16 (2K, C) fp16, rows [Cout][Cin] (mask_out's compute copy); bias (2K) fp32 or NULL;
 *   cls (N) fp32 class index per RoI, as sn_pick_fwd takes its index; prob (N, HW) fp32.
 *   neg = clip((int)cls[n], 0, 2K-1), pos = clip((int)cls[n] + K, 0, 2K-1)            (sn_pick_fwd's clipping on 2K channels)
 *   z_neg = sum_k x[n,p,k] * w[neg,k] + bias[neg], z_pos likewise: fp16 operands, fp32 accumulation, NOT rounded to fp16
 *   prob[n,p] = channel 1 of softmax(z_neg, z_pos), max subtracted first, the statements of sn_softmax_fwd for a K = 2 row.
 * One launch, no atomics, no workspace, no host read-back, the same bits every run.  Refused before any launch: a NULL x, w16,
 * cls or prob; N, HW, C or K below 1; C not a multiple of 8; N*HW*C past 32-bit indexing; x or w16 not 16-byte aligned. */
int sn_mask_class_prob(const void *x, const void *w16, const float *bias, const float *cls, float *prob, int N, int HW, int C, int K,
                       sn_stream_t stream);

/* DeformablePSROIPooling, group_size 1 (:286-293).  data (B,H,W,C) fp16, rois (R,5), trans (R,2,P,P) or NULL,
 * out (R,P,P,C) fp16.  Backward: d_data (B,H,W,C) fp16 (d_data_f32 = 0) or fp32 and d_trans (R,2,P,P) fp32 are
 * OVERWRITTEN (every element written exactly once, no atomics); ws = sn_dpsroi_bwd_workspace_bytes(R). */
int sn_dpsroi_pool_fwd(const void *data, const float *rois, const float *trans, void *out, int R, int H, int W, int C, int pooled,
                       int sample_per_part, float spatial_scale, float trans_std, sn_stream_t stream);
/* ... with the number of images B of `data` (every RoI's image index in [0, B)): the same launch.  (An (image, 64-channel
 * slab)-stationary kernel behind it measured 1.6x slower at R = 6000, profiles/r06_kab_dpsroi.txt, and was removed.) */
int sn_dpsroi_pool_fwd_images(const void *data, const float *rois, const float *trans, void *out, int R, int B, int H, int W, int C,
                              int pooled, int sample_per_part, float spatial_scale, float trans_std, sn_stream_t stream);
size_t sn_dpsroi_bwd_workspace_bytes(int R);
int sn_dpsroi_pool_bwd(const void *dout, const void *data, const float *rois, const float *trans, void *d_data, int d_data_f32,
                       float *d_trans, int R, int B, int H, int W, int C, int pooled, int sample_per_part, float spatial_scale,
                       float trans_std, void *ws, sn_stream_t stream);

/* Position-sensitive variant (group_size G > 1: the R-FCN head of BASELINE config C4; msracver Deformable R-FCN's
 * DeformablePSROIPooling(group_size=7)).  data (B,H,W,C = output_dim*G*G) fp16 in the operator's channel order
 * c = (d*G + gh)*G + gw, out (R,P,P,output_dim) fp16; bin (ph,pw) of output channel d reads channel
 * (d*G + floor(ph*G/P))*G + floor(pw*G/P).  trans (R,2,P,P) class-agnostic or NULL.  Backward as above (overwrites).
 * group_major = 1: the map (and d_data) is laid out (gh*G + gw)*output_dim + d instead -- a bin's output_dim channels are one
 * contiguous run, so a wave's gathers coalesce (the operator order pulls the whole 7.9 KB pixel of a 7*7*81 map through L2 for every
 * bin: 7.5 ms per forward at 16 x 300 RoIs; group-major 50x less).  The caller owns the permutation: the executor applies it to the
 * OUTPUT CHANNELS of the convolution that produces the map (engine/ops.py DPSROIPoolStep), which costs nothing at run time. */
int sn_psroi_pool_fwd(const void *data, const float *rois, const float *trans, void *out, int R, int H, int W, int output_dim,
                      int group_size, int pooled, int sample_per_part, float spatial_scale, float trans_std, int group_major,
                      sn_stream_t stream);
int sn_psroi_pool_bwd(const void *dout, const void *data, const float *rois, const float *trans, void *d_data, int d_data_f32,
                      float *d_trans, int R, int B, int H, int W, int output_dim, int group_size, int pooled, int sample_per_part,
                      float spatial_scale, float trans_std, int group_major, void *ws, sn_stream_t stream);

/* DeformableConvolution sampling (:124-128): column buffer (M, KH*KW, C) fp16 for the 1x1 GEMM, and its backward:
 * d_data (N,H,W,C) fp16/fp32 and d_offset (same layout/dtype as offset) are OVERWRITTEN; either may be NULL.  ws: 16 bytes of
 * device scratch (the launch's max |offset| prunes the data gradient's candidate scan) or NULL (full scan). */
int sn_deform_im2col(const void *data, const void *offset, void *col, int N, int H, int W, int C, int KH, int KW, int stride,
                     int pad, int dil, int deformable_groups, int offset_pix_stride, int offset_dtype, sn_stream_t stream);
int sn_deform_col2im(const void *dcol, const void *data, const void *offset, void *d_data, int d_data_f32, void *d_offset, int N,
                     int H, int W, int C, int KH, int KW, int stride, int pad, int dil, int deformable_groups,
                     int offset_pix_stride, int offset_dtype, void *ws, sn_stream_t stream);

/* Multi-precision SGD with momentum (lib/train_utils/utils.py:26-33). */
int sn_sgd_mom_update(float *w32, const float *grad, float *mom, void *w16, long n, float lr, float wd, float momentum,
                      float rescale, sn_stream_t stream);
/* Same, with lr/wd/momentum/rescale read from device memory d_hyper[4] (for launches captured in a hipGraph):
 * lr = d_hyper[0]*lr_mult, wd = d_hyper[1]*wd_mult. */
int sn_sgd_mom_update_dev(float *w32, const float *grad, float *mom, void *w16, long n, const float *d_hyper, float lr_mult,
                          float wd_mult, sn_stream_t stream);
/* The gradient guard of the optimizer pass: skip a step whose gradients hold inf / NaN, clip by global norm, report the norm -- on the
 * device, inside the captured optimizer graph, no host synchronisation.
 * sn_grad_guard: one pass over d_grad (n fp32, 4-byte aligned; peeled to a 16-byte boundary, then 16-byte loads) and a single-block
 *   finalize launch.  An element g is non-finite iff !(fabsf(g) <= FLT_MAX): counted and left out of the sum; finite elements add
 *   (double)g * (double)g (exact) to fp64 sums per thread, wave, block; one partial per block goes to d_ws
 *   (sn_grad_guard_workspace_bytes(n, max_blocks) bytes, 8-byte aligned) and the finalize adds the partials in index order.  No
 *   atomics: for a given (n, max_blocks, alignment of d_grad) the same bits every run.  max_blocks: 0 = the library's grid, a fixed
 *   function of n; > 0 caps the grid (<= 65535).  d_hyper: the four floats of sn_sgd_mom_update_dev; d_hyper[3] = rescale_grad is read.
 *   d_state, eight doubles (8-byte aligned; the caller zeroes them ONCE, [4..6] are read-modify-write by the finalize block only):
 *     [0] norm   = sqrt(sumsq) * fabs((double)d_hyper[3]): the norm of rescale_grad * grad over the finite elements
 *     [1] coef   = clip_global_norm > 0 ? min(1, clip_global_norm / (norm + 1e-6)) : 1   (torch.nn.utils.clip_grad_norm_; fp64)
 *     [2] skip   = skip_nonfinite && nonfinite > 0   (0 or 1)
 *     [3] non-finite elements of this step      [4] steps seen (+1)      [5] steps skipped (+skip)
 *     [6] consecutive skipped steps (skip ? old + 1 : 0)                 [7] sumsq
 * sn_grad_guard_limits: h_out4 (HOST) = {threads per block, floats per thread per trip, the default grid cap, doubles of state}.
 * sn_sgd_mom_update_guarded_dev: sn_sgd_mom_update_dev behind that state (same head / four-wide body / tail split).  Every thread
 *   reads coef (rounded to float) and skip once.  skip: w32, mom and w16 are NOT WRITTEN.  coef == 1 and clip_gradient <= 0: the
 *   statement of sn_sgd_mom_update_dev, bit-identical results.  Else u = rescale * (coef * grad[i]); with clip_gradient > 0
 *   u = clamp(u, -clip_gradient, +clip_gradient) (mx 'sgd': rescale_grad * grad is clipped, before weight decay); g = u + wd * w;
 *   m = momentum * mom - lr * g; w += m; w16 = half(w).
 * Refused before any launch: null pointers, n < 0, a negative or NaN clip_global_norm, a NaN clip_gradient, max_blocks outside
 * 0 .. 65535, misaligned d_grad / d_ws / d_state. */
int sn_grad_guard_limits(int32_t *h_out4);
size_t sn_grad_guard_workspace_bytes(long n, int max_blocks);
int sn_grad_guard(const float *d_grad, long n, const float *d_hyper, float clip_global_norm, int skip_nonfinite, int max_blocks,
                  void *d_ws, double *d_state, sn_stream_t stream);
int sn_sgd_mom_update_guarded_dev(float *w32, const float *grad, float *mom, void *w16, long n, const float *d_hyper, float lr_mult,
                                  float wd_mult, float clip_gradient, const double *d_state, sn_stream_t stream);
/* Dynamic loss scaling of the fp16 training step: the scale lives on the device, the loss-gradient kernels of the captured
 * forward/backward read it, the guard of the captured optimizer pass unscales with it and moves it.  No host synchronisation.
 * d_ls, eight doubles (8-byte aligned; the caller writes [0] ONCE -- a power of two within 2^-126 .. 2^127 -- and zeroes the rest):
 *     [0] scale: what the loss kernels of the NEXT forward multiply with; always a power of two
 *     [1] scale_used: the scale the gradients just judged carry ([0] as it was before this step's finalize)
 *     [2] clean steps since the scale last changed      [3] growths so far (the scale went up)      [4] back-offs so far (it went down)
 *     [5] steps at which growth was due but max_scale held it (S * growth_factor > max_scale)
 *     [6] steps at which back-off was due but min_scale held it (S * backoff_factor < min_scale)      [7] reserved (0)
 * sn_softmax_output_bwd_scaled: sn_softmax_output_bwd with grad_scale * (float)d_ls[0] in place of grad_scale (every thread reads
 *   d_ls[0] once); both paths, chosen by the same rule.  sn_fill_scaled_f32: out[i] = value * (float)d_ls[0], the MakeLoss gradient.
 *   For d_ls[0] = S both give the bits of the plain kernels called with grad_scale * S (S is a power of two).
 * sn_grad_guard_scaled: the partial pass of sn_grad_guard (the same kernel, grid, workspace), then a single-block finalize.  With
 *   S = d_ls[0] on entry it writes d_state as sn_grad_guard does, except
 *     [0] norm = sqrt(sumsq) * fabs((double)d_hyper[3]) / S  (true units)
 *     [1] coef = c / S, c = clip_global_norm > 0 ? min(1, clip_global_norm / (norm + 1e-6)) : 1 -- what sn_sgd_mom_update_guarded_dev
 *         (used unchanged) multiplies the gradients with: it clips and unscales in one product
 *     [2] skip = nonfinite > 0 (dynamic scaling implies skip_nonfinite);      [7] sumsq stays in arena units
 *   and then moves the scale: d_ls[1] = S; skip: scale = max(S * backoff_factor, min_scale), clean = 0; else clean += 1 and, if
 *   growth_interval > 0 and clean == growth_interval, scale = min(S * growth_factor, max_scale), clean = 0 (growth_interval 0: never).
 *   Refused before any launch: what sn_grad_guard refuses; a factor or a bound that is not a positive power of two; growth_factor < 1;
 *   backoff_factor > 1; min_scale > max_scale or either outside 2^-126 .. 2^127; growth_interval < 0; a null or misaligned d_ls.
 * sn_aux_shadow: desc = DEVICE table of n_desc records {float *ptr; int32_t off; int32_t n} (16 bytes each, 8-byte aligned), the
 *   vectors a training forward writes as a side effect (moving_mean / moving_var of every batch-statistics BatchNorm).  mode 0 saves:
 *   d_shadow[off + i] = ptr[i], i < n.  mode 1 restores: if d_state[2] != 0 (the guard skipped the step) ptr[i] = d_shadow[off + i],
 *   else nothing is written.  One launch, one block per record; nothing outside the named ranges is read or written; n_desc = 0: no launch. */
int sn_softmax_output_bwd_scaled(const float *p, const float *label, float *grad, long outer, int K, long inner, float ignore_label,
                                 int use_ignore, float grad_scale, int normalize_valid, int *ws, const double *d_ls, sn_stream_t stream);
int sn_fill_scaled_f32(float *out, long n, float value, const double *d_ls, sn_stream_t stream);
int sn_grad_guard_scaled(const float *d_grad, long n, const float *d_hyper, float clip_global_norm, int max_blocks, int growth_interval,
                         double growth_factor, double backoff_factor, double min_scale, double max_scale, void *d_ws, double *d_state,
                         double *d_ls, sn_stream_t stream);
int sn_aux_shadow(const void *desc, int n_desc, float *d_shadow, int mode, const double *d_state, sn_stream_t stream);
/* Gradient accumulation: the gradient arena of one micro-batch copied into, or added onto, a second arena, so that the guard and the
 * update above run once per k micro-batches on the sum (what k data-parallel ranks and a summing all-reduce compute).
 * sn_grad_accumulate: one launch over n fp32.  d_grad [0, n) is read; d_acc [0, n) is written, and read first unless `first`; nothing
 *   else is touched.  first != 0: d_acc[i] = d_grad[i] as a copy of the 32 bits (NaN payloads and -0 included).  first == 0:
 *   d_acc[i] = d_acc[i] + d_grad[i], one IEEE binary32 addition rounded to nearest even; subnormal inputs and results are kept, not
 *   flushed; inf and NaN propagate (inf + -inf = NaN), which is how the guard sees a poisoned micro-batch at the end of the window.
 *   Both pointers need 4-byte alignment only and may sit at DIFFERENT offsets from a 16-byte boundary.  The split follows d_acc: its
 *   0-3 elements in front of a 16-byte boundary one at a time, then 16-byte stores (and loads of d_acc), then a tail of 0-3.  d_grad
 *   is read 16 bytes wide where it has d_acc's offset modulo 16 bytes, otherwise with four 4-byte loads per 16-byte store.
 *   Grid-stride loop; max_blocks: 0 = the library's grid, a fixed function of n; > 0 caps the grid (<= 65535).  No atomics, no LDS, no
 *   workspace: every element belongs to one thread, so the bits are the same for every grid, alignment and run -- those of the
 *   statement above (the copy exactly; the sum exactly where it is not NaN, some NaN where it is).
 *   Refused before any launch: a null pointer with n > 0, n < 0, a pointer that is not 4-byte aligned, max_blocks outside
 *   0 .. 65535, and ranges [d_acc, d_acc + n) and [d_grad, d_grad + n) that overlap.  n == 0: no launch, success.
 * sn_grad_accumulate_limits: h_out3 (HOST) = {threads per block, floats per thread per trip, the default grid cap}. */
int sn_grad_accumulate_limits(int32_t *h_out3);
int sn_grad_accumulate(float *d_acc, const float *d_grad, long n, int first, int max_blocks, sn_stream_t stream);
/* Per-tensor statistics of a flat arena: where in the gradient arena a non-finite value sits, and the norms
 * mx.mon.Monitor prints -- one read of the arena, deterministic, capturable.
 * sn_tensor_stats_limits: h_out6 (HOST) = {fp32 elements per block trip, elements per chunk, the largest T, doubles per record (8),
 *   fp16 elements per block trip, the default grid cap of the pass}.
 * sn_tensor_stats_plan (HOST only, no device call): h_segs = T records {int64 off; int64 n} (16 bytes each, offsets in ELEMENTS):
 *   disjoint, in any order, n = 0 allowed.  A work item is a chunk of at most `elements per chunk` elements of ONE tensor; a tensor of
 *   n elements has ceil(n / chunk) items (none for n = 0), in ascending order, tensor after tensor in table order.  h_plan == NULL:
 *   the table is checked and *h_n_items = the number of items; else the plan is also written to h_plan (8-byte aligned,
 *   plan_bytes >= sn_tensor_stats_plan_bytes(T, n_items)): n_items 32-byte items {int64 off; int64 off_in_tensor; int32 len;
 *   int32 tensor; 8 bytes of zeros}, then T 16-byte tensors {int64 n; int32 first_item; int32 items}.  The caller uploads it once per
 *   table.  Refused with a message: T outside 0 .. the limit, a negative off or n, off + n past 2^63 - 1, overlapping segments, more
 *   than 2^31 - 1 items, a plan buffer that is too small.
 * sn_tensor_stats_workspace_bytes(T, n_items): the bytes of d_ws (one 64-byte partial record per item), 0 for arguments out of range.
 * sn_tensor_stats: two launches on `stream`, no host copy, no wait.  d_x: the arena (dtype 0 = fp16, 1 = fp32; aligned to its
 *   element size: every item is peeled to a 16-byte boundary, then read with 16-byte loads; elements between segments are never part
 *   of a record).  d_plan: the uploaded plan.  max_blocks: 0 = the library's grid cap, > 0 caps the grid of the pass (<= 65535).
 *   d_out, (1 + T, 8) float64, 8-byte aligned: a header row, then one record per tensor in table order.
 *     header [0] 1.0: this launch wrote the records   [1] d_guard_state[4] (the guard's step counter), 0 without a state   [2] T
 *            [3] tensors with a non-finite element    [4] the table index of the first such tensor, -1 if none          [5..7] 0
 *     record, an element x being finite iff fabsf(x) <= FLT_MAX (the guard's rule):
 *            [0] sumsq: sum of (double)x * x over the finite elements       [1] sum of (double)x over the finite elements
 *            [2] non-finite elements (exact)    [3] index inside the tensor of the first non-finite element, -1 if none (exact)
 *            [4] max |x| over the finite elements, 0 if none (exact)        [5] elements equal to zero, -0.0 included (exact)
 *            [6] n                              [7] 0
 *   The two float sums are fp64 per thread, wave, block and item (one block reduces one item in a fixed order), and a tensor's item
 *   partials are added in item order: no floating-point atomics, and for a given table, dtype and d_x modulo 16 bytes the same bits
 *   every run and for EVERY max_blocks.
 *   only_if_skipped != 0 (needs d_guard_state, the eight doubles of sn_grad_guard): every block of both launches reads
 *   d_guard_state[2] (skip) before its first load and returns when it is 0: d_out and d_ws are then left untouched, bit for bit.
 *   Refused before any launch: null d_x / d_plan / d_ws / d_out, a dtype other than 0 / 1, T or max_blocks out of range, n_items < 0,
 *   only_if_skipped without a state, misaligned pointers. */
int sn_tensor_stats_limits(int32_t *h_out6);
int sn_tensor_stats_plan(const int64_t *h_segs, int T, void *h_plan, size_t plan_bytes, int32_t *h_n_items);
size_t sn_tensor_stats_plan_bytes(int T, int n_items);
size_t sn_tensor_stats_workspace_bytes(int T, int n_items);
int sn_tensor_stats(const void *d_x, int dtype, const void *d_plan, int n_items, int T, int max_blocks, const double *d_guard_state,
                    int only_if_skipped, void *d_ws, double *d_out, sn_stream_t stream);
/* fp32 [O][T][I] -> fp16 [I][T][O_pad] (weights for sn_conv_dgrad; O_pad = O rounded up to 8, zero filled). */
int sn_weight_transpose(const float *w_oti, void *wt_ito_f16, int O, int T, int I, int O_pad, sn_stream_t stream);
/* The same transposition for MANY weights in one launch (the optimizer step re-emits every data-gradient copy).  desc is a
 * device array of n_desc 48-byte records {const float *src; void *dst; int O, T, I, O_pad, tile0, tiles_o, tiles_i, pad}
 * with tiles_o = ceil(O_pad / 64), tiles_i = ceil(I / 64), tile0 = running sum of T * tiles_o * tiles_i (ascending);
 * total_tiles = the final sum. */
int sn_weight_transpose_batched(const void *desc, int n_desc, int total_tiles, sn_stream_t stream);

/* Detections drawn into images (lib/data_utils/visualization.py:21-57 draws with matplotlib -- the raster here
 * is THIS PROJECT'S, in integer arithmetic, stated in full in that section and restated in numpy by tests/render_ref.py).  One launch
 * renders a batch of I images: tiles x images, no atomics, no workspace, no host read-back, the same bits every run.
 *   form    SN_RENDER_UINT8: src is uint8 HWC RGB, image i at byte 3 * pix_off[i], hw[i] = (h, w) rows of 3 * w bytes.
 *           SN_RENDER_TENSOR: src is float32, image i at element 3 * pix_off[i] as three planes of h * w (a (B, 3, Hm, Wm) network
 *           input has pix_off[i] = i * Hm * Wm); channel j of a pixel is x + mean_j in float32, truncated toward zero and CLAMPED to
 *           0 .. 255 (numpy's astype(uint8) of the reference wraps instead).
 *   hw (I,2) i32, pix_off (I+1) i64 in pixels, out uint8 HWC RGB with the same offsets; max_h / max_w: the largest h and w (they
 *   size the grid); total_pixels = pix_off[I].
 *   Items of image i: item_off[i] .. item_off[i+1] (at most SN_RENDER_MAX_ITEMS = max_items of the largest image), each with
 *     rects (n,4) i32 x1, y1, x2, y2 inclusive, anywhere (coordinates are clamped to +-2^29); colors (n,3) u8 RGB;
 *     mask_idx (n) i32: a row of masks (n_masks, M, M) f32 or -1 -- the mask is pasted into rect by the arithmetic of sn_rle_paste
 *     with binary_thresh, so rect must then be that paste's box (0 <= x1 <= x2 < w, likewise y: the caller's precondition);
 *     text_off (n+1) i32 into text (total_text) i32, glyph indices into atlas (G, gh, gw) u8 coverage.  h_text: the same indices in
 *     HOST memory or NULL -- given, every index outside [0, G) is refused; not given, that is the caller's precondition (the kernel
 *     skips such a glyph, it never reads outside the atlas).
 *   Layers per pixel: source; mask fill p = (p * (256 - mask_alpha) + c * mask_alpha + 128) >> 8; outline (inside rect, not inside rect
 *   shrunk by line_width; opaque, later items over earlier); label (a box of len * gw + 2 by gh + 2 at x1, above rect when its top
 *   y1 - (gh + 2) >= 0 and at y1 + line_width otherwise: the blend with 128, then glyph pixels toward white by cov + (cov >> 7)).
 * Refused before any launch, by a message that names the function and the condition: a NULL tensor where one is needed (masks only
 * when n_masks > 0, text and atlas only when total_text > 0, the item tables only when total_items > 0); an unknown form; I outside
 * 1 .. 65535; max_items above SN_RENDER_MAX_ITEMS; M outside 1 .. 1024; mask_alpha outside 0 .. 256; line_width outside 1 .. 65536; an
 * atlas cell outside 1 .. 256 per side; a glyph index of h_text outside [0, G); sizes past 32-bit indexing.
 * sn_render_limits: h_out5 (HOST) = {SN_RENDER_MAX_ITEMS, tile width, tile height, items per culling round (the LDS list), threads
 * per workgroup}. */
#define SN_RENDER_MAX_ITEMS 4096
#define SN_RENDER_UINT8 0
#define SN_RENDER_TENSOR 1
int sn_render_limits(int32_t *h_out5);
int sn_render_dets(int form, const void *src, const int32_t *hw, const int64_t *pix_off, int I, int max_h, int max_w,
                   long total_pixels, const int32_t *item_off, int max_items, long total_items, const int32_t *rects,
                   const uint8_t *colors, const int32_t *mask_idx, const int32_t *text_off, const int32_t *text,
                   const int32_t *h_text, long total_text, const uint8_t *atlas, int G, int gh, int gw, const float *masks,
                   int n_masks, int M, float binary_thresh, int mask_alpha, int line_width, float mean0, float mean1, float mean2,
                   uint8_t *out, sn_stream_t stream);

/* PNG encoding of a batch of pictures: the row filters, and a deflate coder of many byte buffers that is public
 * on its own.  Integer arithmetic, exact bytes, the same every run; no global atomics, no host read-back inside any call.
 * Deflate: S streams pooled in data behind offsets (S+1) i64 -> one zlib stream (RFC 1950: 78 01, deflate blocks, big-endian
 *   Adler-32) per input stream.  A stream is cut into blocks of B = 32768 bytes (an empty stream has one empty block); one workgroup
 *   codes one block.  Tokens, inside a block: every maximal run of equal bytes [s, e) is a literal at s, then its remaining e - s - 1
 *   bytes in pieces of 258 from the left -- a piece of >= 3 bytes is a match (length, distance 1), a piece of 1 or 2 bytes that many
 *   literals.  Per block a dynamic Huffman code (BTYPE 2), lengths limited to 15 bits (code lengths: 7), complete, ties by symbol
 *   index; all 286 literal/length lengths and one distance length (1, or 0 in a block without matches) are sent without repeat
 *   symbols.  A dynamic block that is not the last of its stream is followed by an empty stored block (byte alignment); a block whose
 *   coded bytes would exceed len + 5 is stored (BTYPE 0).  For a stream of n bytes in nb = ceil(n / B) blocks the output is at most
 *   sn_deflate_bound(n) = n + 5 * (nb + 1) + 6 bytes.
 *   The offsets are given twice, as everywhere here: on the device (what the kernels read) and as the HOST array they were uploaded
 *   from (h_offsets, what the entry point checks).  The calls, in order:
 *     sn_deflate_plan   blk_first (S+1) i32 = the running block count; n_blocks = blk_first[S] is known to the host from h_offsets.
 *     sn_deflate_code   per block: blk_code (n_blocks, code_words) u32 -- the code, the header bits, the Adler-32 partial sums -- and
 *                       blk_size (n_blocks) i64 = the block's bytes in the output, the 2 header bytes of a stream's first block and the
 *                       4 Adler-32 bytes of its last one included.
 *     (caller)          blk_pos (n_blocks) i64 = the exclusive prefix sum of blk_size: the streams come out compact, stream s at
 *                       blk_pos[blk_first[s]].
 *     sn_deflate_write  the bytes; out has room for `capacity` bytes and nothing is written at or past out + capacity.
 *   Refused before any launch, by a message that names the function and the condition: NULL pointers; S outside 1 .. 65535; offsets
 *   that do not start at 0, are not ascending or do not end at `total`; n_blocks other than the offsets give; a capacity below the sum
 *   of sn_deflate_bound over the streams.
 * sn_deflate_limits: h_out6 (HOST) = {B, threads per workgroup, the largest S, code_words, LDS bytes of the code kernel, LDS bytes of
 *   the write kernel (dynamic)}.
 * sn_png_filter: pictures as sn_render_dets writes them (uint8 HWC RGB, picture i at byte 3 * pix_off[i], hw[i] = (h, w)) -> the
 *   filtered stream of picture i at out + stream_off[i]: per row one filter-type byte and 3 * w bytes.  All five filters of the PNG
 *   specification (bpp = 3; the row above the first and the pixels left of the first are zero; Average floors the 9-bit sum; Paeth
 *   breaks ties a, b, c); the filter with the smallest sum of min(v, 256 - v) over the row's filtered bytes is kept, ties to the
 *   lowest type.  h_hw: the sizes on the HOST; total_pixels and total_stream = sum of h * (3 * w + 1) must match them. */
int sn_deflate_limits(int32_t *h_out6);
long sn_deflate_bound(long n);
int sn_deflate_plan(const int64_t *offsets, const int64_t *h_offsets, long S, long total, int32_t *blk_first, sn_stream_t stream);
int sn_deflate_code(const uint8_t *data, const int64_t *offsets, const int64_t *h_offsets, long S, long total,
                    const int32_t *blk_first, long n_blocks, uint32_t *blk_code, int64_t *blk_size, sn_stream_t stream);
int sn_deflate_write(const uint8_t *data, const int64_t *offsets, const int64_t *h_offsets, long S, long total,
                     const int32_t *blk_first, long n_blocks, const uint32_t *blk_code, const int64_t *blk_pos, uint8_t *out,
                     long capacity, sn_stream_t stream);
int sn_png_filter(const uint8_t *pix, const int32_t *hw, const int32_t *h_hw, const int64_t *pix_off, const int64_t *stream_off, int I,
                  long total_pixels, long total_stream, uint8_t *out, sn_stream_t stream);

/* Baseline JPEG decoding of a batch of files: compressed bytes in, (H, W, 3) uint8 BGR pictures out, bit for
 * bit what libjpeg's slow-integer IDCT with fancy upsampling gives.  Integer arithmetic, the same bytes every run; plain vector stores;
 * the only atomic is the OR of a non-zero status into its image's word.  The host finds the markers and builds three tables; as
 * everywhere here each comes twice, on the device (what the kernels read) and as the HOST array it was uploaded from (h_*, what the
 * entry point checks before any launch).
 *   img (I, 16) i32: W, H, components (1, or 3 = YCbCr), luma sampling hs, vs (1x1, 2x1 or 2x2; chroma is 1x1), MCU columns, MCU rows,
 *     blocks per MCU, first segment, segments, first block (in the coefficient buffer), first byte of its planes (16-byte aligned),
 *     first byte of its stream in `data`, length of its stream, table bits (bit 2c: the DC table of component c, bit 2c + 1: its AC
 *     table), restart interval in MCUs (0: none).  Images follow one another in segments and blocks without gaps.
 *   seg (S, 8) i32: image, first byte and end byte of the segment's entropy-coded data inside the image's stream (a segment is a
 *     restart interval, or the whole scan), first subsequence, subsequences = max(1, ceil(bytes / sub_bytes)); three unused.
 *   dht (I, 4, 272) u8: the tables DC 0, DC 1, AC 0, AC 1 as a DHT segment holds them (16 counts, then the values), zero where absent.
 *   qtab (I, 3, 64) u16: the quantisation table of each component in natural (row-major) order.
 * sn_jpeg_entropy: one workgroup per segment.  phases bit 0: the self-synchronising rounds over subsequences of sub_bytes bytes (lane
 *   i decodes from the guess "a block starts here", then takes the exit state of the subsequence before it as its entry and decodes
 *   again only where that entry changed, until a round changes nothing -- at most as many rounds as the segment has subsequences) and
 *   the exclusive scan of the completed-block counts; rounds (S) i32 gets the rounds each segment took.  phases bit 1: the pass that
 *   writes the coefficients from the exact entries: coef (n_blocks, 64) i16, blocks in scan order, natural order inside a block, DC as
 *   differences -- into a buffer the caller has ZEROED.  3 runs both in one launch; 2 needs the state a call with 1 left.
 *   state (3, n_sub, 2) u32 and counts (2, n_sub) i32 are scratch.  status (I) i32, zeroed by the caller, collects per image:
 *   1 no code matches / a category too large, 2 a run past coefficient 63, 4 a symbol past the end of its segment, 8 a segment
 *   with another number of blocks than the header says, 16 a DC value outside int16, 32 samples outside the range in which all
 *   libjpeg IDCT forms agree, 64 a missing or wrong restart marker.  Nothing is read past a stream or written past a segment's blocks
 *   whatever the data holds.
 * sn_jpeg_dc: the running sum of the DC differences per component inside each segment, in place.
 * sn_jpeg_pixels: dequantise, IDCT into component planes (scratch, plane_bytes >= the sum of 64-byte-aligned 64 * blocks), upsample,
 *   convert, and write picture i to out_ptrs[i] (device addresses, u64; H * W * 3 bytes each, 4-byte aligned).  MCU padding is never
 *   written to a picture.
 * sn_jpeg_limits: h_out8 (HOST) = {default sub_bytes (SNIPER_JPEG_SUB), threads per workgroup, the largest I, the most blocks per MCU,
 *   LDS bytes of the four decoding tables, fields per image, fields per segment, the smallest sub_bytes}.
 * Refused before any launch, by a message that names the function and the condition: NULL pointers; I outside 1 .. 65535; sizes,
 *   samplings, MCU grids, segment counts or offsets that do not follow from one another; a stream or a segment outside `data`; a
 *   subsequence table other than sub_bytes gives; sub_bytes outside 16 .. 4096; a segment of more than 16384 subsequences (its
 *   rounds are one workgroup's: such scans are the host's); totals of 2^31 bytes or 2^25 blocks and more. */
int sn_jpeg_limits(int32_t *h_out8);
int sn_jpeg_entropy(const uint8_t *data, long total_bytes, const int32_t *img, const int32_t *h_img, int I, const int32_t *seg,
                    const int32_t *h_seg, int S, const uint8_t *dht, int sub_bytes, long n_sub, long n_blocks, uint32_t *state,
                    int32_t *counts, int16_t *coef, int32_t *rounds, int32_t *status, int phases, sn_stream_t stream);
int sn_jpeg_dc(const int32_t *img, const int32_t *h_img, int I, const int32_t *seg, const int32_t *h_seg, int S, long n_blocks,
               int16_t *coef, int32_t *status, sn_stream_t stream);
int sn_jpeg_pixels(const int32_t *img, const int32_t *h_img, int I, const uint16_t *qtab, const int16_t *coef, long n_blocks,
                   uint8_t *planes, long plane_bytes, const uint64_t *out_ptrs, int32_t *status, sn_stream_t stream);

/* Baseline JPEG encoding of a batch of pictures: pictures in, the entropy-coded scans of .jpg files out, byte
 * for byte the scans libjpeg writes at the same quality and sampling (scaled Annex K quantisation tables, slow-integer forward DCT,
 * Annex K Huffman tables, one interleaved scan, no restart markers).  Integer arithmetic, the same bytes every run; plain vector
 * stores and 32-bit atomic ORs into zeroed words.  The host writes the headers around the scans (sniper_amd/jpeg_encode.py).
 * One call takes I pictures of one kind: ncomp 3 (uint8 HWC RGB, as sn_render_dets writes them) or 1 (uint8 grey); picture i has
 *   hw[i] = (h, w), 1 <= h, w <= 65535, and starts at byte ncomp * pix_off[i] of pix; pix_off (I+1) i64 is the running sum of h * w.
 *   sampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (the luma factors (1,1), (2,1), (2,2); ignored for ncomp 1); quality 1 .. 100.
 *   Blocks are counted in scan order: MCUs in raster order, inside an MCU the luma blocks row-major, then Cb, then Cr.  blk_off (I+1)
 *   i64 is the running sum of ceil(w / 8hs) * ceil(h / 8vs) * (hs * vs + ncomp - 1).  hw, pix_off, blk_off are device arrays;
 *   h_hw, h_pix_off, h_blk_off (HOST) are the same values, which the entry points check against one another.
 * sn_jpeg_enc_blocks: coef (n_blocks, 64) i16 = the quantised coefficients of every block, zig-zag order inside a block, the DC not
 *   differenced; a dummy block of an edge MCU (beyond the component's real blocks) has the DC of the last real luma block before it
 *   in its MCU and no AC.
 * sn_jpeg_enc_size: bits (n_blocks) i32 = the length of every block's Huffman code.  status (1) i32, zeroed by the caller, collects
 *   1: a store that had no room, 2: a coefficient no baseline code holds (never, for coefficients sn_jpeg_enc_blocks made).
 * The caller scans: bit_excl (n_blocks) i64 = the exclusive running sum of bits over the call; pic_first_bit (I) = bit_excl at each
 *   picture's first block; raw_len (I) i64 = a picture's bits rounded up to bytes; chunk_off (I+1) i64 = the running sum of
 *   ceil(raw_len / 64): picture i's raw (unstuffed) stream starts at byte 64 * chunk_off[i] of raw.
 * sn_jpeg_enc_write: every block's code at its bit of raw, MSB first; a picture's last block adds the 1-bits that fill its last byte.
 *   raw has raw_capacity bytes, ZEROED by the caller, a multiple of 64 and at least the sum over the pictures of (208 * blocks + 1)
 *   rounded up to 64: a block's code is at most 22 + 63 * 26 bits.  Nothing is written at or past raw + raw_capacity, nor into
 *   another picture's chunks, whatever the scanned arrays hold.
 * sn_jpeg_enc_stuff: n_chunks >= chunk_off[I] chunks of 64 bytes.  phase 1: cnt (n_chunks) i32 = the bytes of each chunk after a 00
 *   is put behind every FF (0 for chunks behind the last).  phase 2: the chunks' stuffed bytes at out + out_pos[chunk] (the caller's
 *   exclusive running sum of cnt: the pictures' scans lie back to back).  out has `capacity` >= 128 * n_chunks bytes; nothing is
 *   written at or past out + capacity.
 * sn_jpeg_enc_limits: h_out8 (HOST) = {threads per workgroup, the largest I, the most blocks per call, raw bytes per block (208),
 *   bytes per chunk (64), LDS bytes of the blocks kernel, LDS bytes of the size and write kernels, stuffed bytes per raw byte (2)}.
 * Refused before any launch, by a message that names the function and the condition: NULL pointers; I outside 1 .. 65535; h or w
 *   outside 1 .. 65535; ncomp, sampling, quality or phase outside their values; offsets or totals that do not follow from the
 *   sizes; more than 2^22 blocks; capacities below their bounds. */
int sn_jpeg_enc_limits(int32_t *h_out8);
int sn_jpeg_enc_blocks(const uint8_t *pix, long total_pixels, const int32_t *hw, const int32_t *h_hw, const int64_t *pix_off,
                       const int64_t *h_pix_off, const int64_t *blk_off, const int64_t *h_blk_off, int I, long n_blocks, int ncomp,
                       int sampling, int quality, int16_t *coef, sn_stream_t stream);
int sn_jpeg_enc_size(const int16_t *coef, const int32_t *hw, const int32_t *h_hw, const int64_t *blk_off, const int64_t *h_blk_off,
                     int I, long n_blocks, int ncomp, int sampling, int32_t *bits, int32_t *status, sn_stream_t stream);
int sn_jpeg_enc_write(const int16_t *coef, const int32_t *hw, const int32_t *h_hw, const int64_t *blk_off, const int64_t *h_blk_off,
                      int I, long n_blocks, int ncomp, int sampling, const int64_t *bit_excl, const int64_t *pic_first_bit,
                      const int64_t *chunk_off, uint32_t *raw, long raw_capacity, int32_t *status, sn_stream_t stream);
int sn_jpeg_enc_stuff(const uint32_t *raw, long raw_capacity, const int64_t *chunk_off, const int64_t *raw_len, int I, long n_chunks,
                      int phase, int32_t *cnt, const int64_t *out_pos, uint8_t *out, long capacity, sn_stream_t stream);

/* PNG decoding of a batch of files: zlib streams inflated on the device -- public on its own, the counterpart
 * of sn_deflate_* -- then the row filters undone and the pixels expanded.  Integer arithmetic, exact bytes, the same every run; no
 * global atomics, no host read-back inside any call.
 * sn_inflate: S zlib streams (RFC 1950 / 1951: stored, fixed and dynamic blocks, distances up to 32768) pooled in data (total_in
 *   bytes).  tab (S, 4) i64 = {in_off, in_len, out_off, out_cap} per stream, given twice as everywhere here: on the device (what the
 *   kernel reads) and as the HOST array it was uploaded from (h_tab, what the entry point checks).  One wave decodes one stream into
 *   out + out_off, never at or past out_cap bytes.  meta (S, 2) i32 = {bytes produced, status}; status is 0 or ONE of: 1 bad zlib
 *   header (CM != 8, window above 32 KiB, FDICT, check bits), 2 block type 3, 4 stored LEN != ~NLEN, 8 bad or over-subscribed code
 *   lengths (an incomplete set passes only as one code of length 1, as in zlib), 16 invalid symbol (286, 287, distance 30 / 31, a
 *   code no symbol has), 32 distance beyond the start of the output, 64 input ended early, 128 output over capacity, 256 Adler-32
 *   mismatch, 512 bytes left after the Adler-32.  A damaged stream ends after a bounded number of steps with its status; what it
 *   produced before the damage is in out.
 * sn_inflate_limits: h_out6 (HOST) = {the largest S, the most bytes of a stream and of its output, LDS bytes per wave, the window
 *   (32768), lanes per stream (64), the bytes after which the window is stored (16384)}.
 * Images: img (I, 8) i32 = {w, h, bit depth, colour type, row bytes = ceil(w * channels * depth / 8), bpp = max(1, channels * depth
 *   / 8), palette entries, 0}, raw_off (I) i64 = where the image's h * (row bytes + 1) inflated bytes start in raw; both given on
 *   the device and on the HOST.  Stream i of the sn_inflate call is image i: meta is the same array.
 * sn_png_unfilter: the five row filters undone in place (the row above the first and the bytes left of the first pixel are zero,
 *   Average floors the 9-bit sum, Paeth breaks ties a, b, c).  An image whose status is not 0 is left alone; one whose stream gave
 *   another length than h * (row bytes + 1) gets status 2048, one with a filter type above 4 status 1024.
 * sn_png_expand: the images whose status is 0 -> the tensors out_ptrs (I) names.  mode 0: (h, w, 3) uint8 BGR, what PIL's
 *   convert('RGB') gives reversed (grey of depth 1 / 2 / 4 times 255 / 85 / 17, palette entries from pal (I, 768) with (0, 0, 0)
 *   beyond `palette entries`, the high byte of 16-bit samples, alpha dropped).  mode 1: (h, w) uint8, the palette index or the grey
 *   sample scaled to 8 bits; colour types 0 and 3 only.
 * Refused before any launch, by a message that names the function and the condition: NULL pointers; S or I outside 1 .. 65535;
 *   streams or outputs that leave their buffers, overlap or exceed the largest stream; sizes, depths, colour types, row bytes or bpp
 *   that do not fit together; a mode other than 0 / 1. */
int sn_inflate_limits(int32_t *h_out6);
int sn_inflate(const uint8_t *data, long total_in, const int64_t *tab, const int64_t *h_tab, long S, uint8_t *out, long out_total,
               int32_t *meta, sn_stream_t stream);
int sn_png_unfilter(uint8_t *raw, long raw_total, const int32_t *img, const int32_t *h_img, const int64_t *raw_off,
                    const int64_t *h_raw_off, int I, int32_t *meta, sn_stream_t stream);
int sn_png_expand(const uint8_t *raw, long raw_total, const int32_t *img, const int32_t *h_img, const int64_t *raw_off,
                  const int64_t *h_raw_off, int I, const uint8_t *pal, const uint64_t *out_ptrs, const int32_t *meta, int mode,
                  sn_stream_t stream);

/* The ground truth of the VOC mask evaluation from index maps (the reference's parse_inst): obj_ptrs / cls_ptrs
 * (I) u64 name contiguous (h, w) uint8 maps on the device, hw (I, 2) i32 = (h, w) on the device and on the HOST.
 * sn_vocgt_scan: inst (I, 256, 6) i32 = per instance id {x1, y1, x2, y2 (min / max column / row of the id's pixels), the smallest
 *   class under them, 1 where they carry more than one class}; x2 = -1 for an id the image does not hold, and for id 0.
 * sn_vocgt_crop: rec (N, 6) i32 = {image, id, x1, y1, bound width, bound height}, pool_off (N + 1) i64 = the running sum of width *
 *   height (both on the device and on the HOST) -> pool[pool_off[n] + y * width + x] = 1 where the object map holds the id.
 * Refused before any launch: NULL pointers; I outside 1 .. 65535, N outside 1 .. 65535; empty maps; a bound that leaves its map;
 *   offsets that are not the running sum. */
int sn_vocgt_scan(const uint64_t *obj_ptrs, const uint64_t *cls_ptrs, const int32_t *hw, const int32_t *h_hw, int I, int32_t *inst,
                     sn_stream_t stream);
int sn_vocgt_crop(const uint64_t *obj_ptrs, const int32_t *hw, const int32_t *h_hw, int I, const int32_t *rec, const int32_t *h_rec,
                     const int64_t *pool_off, const int64_t *h_pool_off, long N, uint8_t *pool, long pool_total, sn_stream_t stream);

/* Box voting after the test-time NMS (TEST.BBOX_VOTE; ours, modelled on Detectron's box_utils.box_voting).
 * Problem q = image * nc + class owns rows [d_off[q], d_off[q+1]) of BOTH arrays: d_all_rows holds the (n_a, 5) f32 rows
 * [x1,y1,x2,y2,score] handed to the NMS (a copy taken before it, read only), d_top_rows what the NMS left in place -- its first
 * d_top_count[q] rows are the kept boxes with their post-NMS scores; rows past the count are never read or written.
 * sn_box_vote: every kept row t is replaced by the score-weighted mean of the rows a of d_all_rows with overlap(t, a) >= thresh
 *   (the float64 +1-pixel overlap of lib/bbox/bbox.pyx from the float32 coordinates; weights = the PRE-NMS scores; float64 sums
 *   added in ascending row order, divided, narrowed to float32).  A row without a voter (non-positive width or height) or with a
 *   weight sum that is not > 0 stays untouched.  method 0 'ID': the score stays; 1 'AVG': (float)(sum s / voters); 2 'IOU_AVG':
 *   (float)(sum iou * s / sum iou).  In place, order and counts unchanged; no atomics, no workspace, the same bits every run.
 *   d_tiles (n_tiles, 2) i32 = {problem, first kept row} for every sn_box_vote_limits()[0] rows of every problem's PRE-NMS size (an
 *   upper bound of its kept rows, known on the host; a tile at or beyond d_top_count[q] returns) -- no host read of the counts.
 * sn_box_vote_limits: h_out2 (HOST) = {kept rows per tile, pre-NMS rows per LDS chunk}.
 * Refused before any launch, by a message that names the function and the condition: NULL pointers; P < 0; n_tiles < 0; thresh
 *   outside (0, 1] or NaN; a method other than 0 / 1 / 2; arrays not aligned to 4 bytes; d_top_rows == d_all_rows.  P == 0 or
 *   n_tiles == 0: nothing is launched. */
int sn_box_vote_limits(int32_t *h_out2);
int sn_box_vote(float *d_top_rows, const float *d_all_rows, const int32_t *d_off, const int32_t *d_top_count, const int32_t *d_tiles,
                int n_tiles, int P, double thresh, int method, sn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SNIPER_HIP_H */
